#!/usr/bin/env python3
"""Adversarial training of the DiffDelGRU generator against one of the critics, on the device: the reference's third training
command (code/train-adversarial.py) with its command line,

    python tools/train_adversarial.py [--load_config N] [--DRY_RUN]

N from configs/AdversarialConfig.py (0-7 and 10; default '10'), restated in ntm_amd.adversarial.load_config.  The loop itself is
ntm_amd.adversarial.Trainer; this file builds what the script builds around it: the training set in segments of `segment_length`
and the validation set in segments of `val_segment_length` (SegmentFeeder), three independently shuffled batch streams per epoch
(generator input, critic input, critic target), validation at batch 10, DiffDelRNN(hidden_size=hid_size, skip=False) with
Adam(lr=gen_lr, betas=(0.5, 0.9)), and critics.get_critic(crit, crit_pars, device, crit_lr=gen_lr, test_in_len=tbptt_length) --
it is gen_lr that the script hands to get_critic; the configurations' `crit_lr: 0` is never read.  Per epoch, as there: the
running checkpoint, the validation pass, the best checkpoints, then one epoch of training.  Checkpoints go to
MODEL_PATH/UnpairedTraining_N/ (`running{epoch}.pth`, `{key}best.pt`); --DRY_RUN writes nothing.  One JSON line per epoch on stdout:
the validation losses, the keys whose best epoch this is, the mean critic and generator loss, the seconds.

Extra flags of this build: --AUDIO_PATH / --DATASET_DIR (where the data is), --MODEL_PATH (default: the configuration's),
--EPOCHS (the reference loops 10 000), --MAX_ITERS (iterations per epoch), --FRACTION, --SEED."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ntm_amd  # noqa: E402
from ntm_amd import adversarial, critics, evaluation  # noqa: E402
from ntm_amd.feeder import SegmentFeeder  # noqa: E402

V_BS = 10           # the reference's validation batch size (code/train-adversarial.py:118)


def parser():
    p = argparse.ArgumentParser(description='''This is a script that runs adversarial training''')
    p.add_argument('--load_config', '-l', help="Config Number, will load from adversarial.load_config and overwrite defaults",
                   default='10')
    p.add_argument('--DRY_RUN', action='store_true', default=False)
    # this build's own
    p.add_argument('--AUDIO_PATH', type=str, default="../audio/")
    p.add_argument('--DATASET_DIR', type=str, default=None, help="the dataset directory itself (overrides AUDIO_PATH/dataset_path)")
    p.add_argument('--MODEL_PATH', type=str, default=None, help="where the checkpoints go (default: the configuration's model_path)")
    p.add_argument('--EPOCHS', type=int, default=10000)
    p.add_argument('--MAX_ITERS', type=int, default=None, help="at most this many iterations per epoch")
    p.add_argument('--FRACTION', type=float, default=1.0)
    p.add_argument('--SEED', type=int, default=None, help="seed of the three shuffles and of the critic's initial weights")
    return p


def collate(items):
    """[(input (C, L), target (C, L), meta)] -> the reference's batch: (input (B, C, L), target (B, C, L), meta with the delay
    trajectories (B, L) in seconds)."""
    return (torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items]),
            {"delay_trajectory": torch.stack([it[2]["delay_trajectory"] for it in items])})


def batches(dataset, batch_size, order, max_iters=None):
    """The items of `dataset` in `order`, collated `batch_size` at a time (the last batch may be smaller, as a DataLoader's)."""
    starts = range(0, len(order), batch_size)
    for b0 in (starts if max_iters is None else list(starts)[:max_iters]):
        yield collate([dataset[i] for i in order[b0:b0 + batch_size]])


def main(argv=None):
    a = parser().parse_args(argv)
    print("\nArguments:")
    print(a)
    lc = a.load_config
    cfg = adversarial.load_config(int(lc))
    lr, tbptt_len = cfg['gen_lr'], cfg['tbptt_length']

    # Model save info
    model_path = os.path.join(a.MODEL_PATH if a.MODEL_PATH is not None else cfg['model_path'], "UnpairedTraining_" + str(lc))
    if not a.DRY_RUN:
        os.makedirs(model_path, exist_ok=True)
    if not torch.cuda.is_available():
        raise RuntimeError("train_adversarial: HIP device only (no CPU fallback): no device is available")
    device = torch.device("cuda:0")

    # Data
    dataset_path = a.DATASET_DIR if a.DATASET_DIR is not None else os.path.join(a.AUDIO_PATH, cfg['dataset_path'])
    print("\nDataset for training:")
    dataset_train = SegmentFeeder(dataset_path, subset="train", length=cfg['segment_length'], fraction=a.FRACTION)
    print("\nDataset for validation:")
    dataset_val = SegmentFeeder(dataset_path, subset="val", length=cfg['val_segment_length'], fraction=a.FRACTION)
    assert dataset_train.fs == dataset_val.fs, "Sampling rates don't match"
    fs = dataset_train.fs
    d_min, d_max = adversarial.delay_range(dataset_train)
    _, val_d_max = adversarial.delay_range(dataset_val)

    if a.SEED is not None:
        torch.manual_seed(a.SEED)
    Generator = ntm_amd.DiffDelRNN(hidden_size=cfg['hid_size'], skip=False).to(device=device)
    optG = torch.optim.Adam(Generator.parameters(), lr=lr, betas=(0.5, 0.9))
    Critic, optC = critics.get_critic(cfg['crit'], cfg['crit_pars'], device=device, crit_lr=lr, test_in_len=tbptt_len)
    trainer = adversarial.Trainer(Generator, Critic, optG, optC, tbptt_len, fs, d_min, d_max, model_path=model_path, dry_run=a.DRY_RUN)
    evaluator = evaluation.val_loss_supervised(device=device)
    shuffle = torch.Generator()
    if a.SEED is not None:
        shuffle.manual_seed(a.SEED)

    for epoch in range(0, a.EPOCHS):
        start = time.time()
        val_batches = batches(dataset_val, V_BS, list(range(len(dataset_val))), a.MAX_ITERS)
        n_val = max(1, len(range(0, len(dataset_val), V_BS)) if a.MAX_ITERS is None else min(a.MAX_ITERS, len(range(0, len(dataset_val), V_BS))))
        trainer.validate(val_batches, evaluator, val_d_max, epoch=epoch)
        orders = [torch.randperm(len(dataset_train), generator=shuffle).tolist() for _ in range(3)]
        crit_losses, gen_losses = trainer.train_epoch(*[batches(dataset_train, cfg['batch_size'], o, a.MAX_ITERS) for o in orders])
        mean = lambda v: sum(v) / len(v) if v else None      # noqa: E731
        print(json.dumps({"epoch": epoch, "val": {k: v / n_val for k, v in evaluator.losses.items()},
                          "best": [k for k, b in evaluator.bst_losses.items() if b[0] == epoch],
                          "loss_critic": mean(crit_losses), "loss_gen": mean(gen_losses), "windows": len(gen_losses),
                          "seconds": round(time.time() - start, 3)}), flush=True)
    return trainer


if __name__ == "__main__":
    main()
