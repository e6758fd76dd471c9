#!/usr/bin/env python3
"""Training of the diffusion generators (the tape-hiss net and the delay-trajectory nets) on the device: the reference's command
(code/train-diffusion.py) with its command line,

    python tools/train_diffusion.py --MODE noise|trajectories|toy_trajectories

Any other MODE is a NotImplementedError, as there.  The mode picks the configuration (configs/conf_noise.yaml,
conf_trajectories.yaml, conf_toytrajectories.yaml, restated in ntm_amd.diffusion.load_config) and the dataset class
(TapeHissdset for noise, ToyTrajectories for both others), as `_main` does.  The loop is ntm_amd.diffusion.EDMTrainer's
training_loop; this file builds what `_main` builds around it, in its order: the dataset (which seeds `random` and
`np.random`), the network, Adam with the configuration's betas and eps, the batch source, then the trainer's
torch.manual_seed(np.random.randint(1 << 31)), the resume if train.resume asks for one, and the loop.  The batches draw from the
two generators after that, in ONE process: the reference's `num_workers: 2` forks two copies of the seeded dataset whose draws
interleave as torch's worker seeding has it; this driver reproduces the single-process order (num_workers=0).  Checkpoints go
to {model_dir}/{exp_name}-{it}.pt.  One JSON line per logged iteration on stdout: it, loss.

Extra flags of this build:
  --CONFIG      a YAML file of the configurations' layout instead of the mode's own
  --DSET_PATH   the folder of training files (default: the configuration's dset.path)
  --MODEL_DIR   where the checkpoints go (default: the configuration's model_dir); created if missing
  --MAX_IT      the last iteration number that runs (default: none -- the reference loops for ever)
  --BACKEND     hip (default): the network as HIP graph nodes, HIP device only | torch: forward_torch, any device
  --OPTIMIZER   fused (default): optim.FusedAdam, clip + Adam + EMA as launches over tensor lists | adam: torch.optim.Adam
  --FEEDER      device (default): datasets_diffusion.DeviceSegmentFeeder, the files in a bank on the device | host: the
                reference's loader (a DataLoader with num_workers=0 over the dataset, get_batch's upload and resample)
  --DEVICE      default: cuda if there is one, else cpu, as the reference chooses; on the CPU only
                --BACKEND torch --OPTIMIZER adam --FEEDER host runs -- nothing falls back on its own
  --SEED        seeds the dataset (the classes' default, 42) and torch before the network is initialised; the reference
                leaves torch unseeded there, so its initial weights differ from run to run
  --LOG_EVERY   print every n-th iteration (default 1, as the reference prints; reading the loss synchronises)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntm_amd import datasets_diffusion, diffusion, optim  # noqa: E402

# mode -> (configuration, dataset class): code/train-diffusion.py main() and _main()
MODES = {"noise": ("noise", datasets_diffusion.TapeHissdset), "trajectories": ("trajectories", datasets_diffusion.ToyTrajectories),
         "toy_trajectories": ("toytrajectories", datasets_diffusion.ToyTrajectories)}


def parser():
    p = argparse.ArgumentParser()
    p.add_argument('--MODE', type=str, default=None)
    # this build's own
    p.add_argument('--CONFIG', type=str, default=None)
    p.add_argument('--DSET_PATH', type=str, default=None)
    p.add_argument('--MODEL_DIR', type=str, default=None)
    p.add_argument('--MAX_IT', type=int, default=None)
    p.add_argument('--BACKEND', choices=("hip", "torch"), default="hip")
    p.add_argument('--OPTIMIZER', choices=("fused", "adam"), default="fused")
    p.add_argument('--FEEDER', choices=("device", "host"), default="device")
    p.add_argument('--DEVICE', type=str, default=None)
    p.add_argument('--SEED', type=int, default=42)
    p.add_argument('--LOG_EVERY', type=int, default=1)
    return p


def build(a):
    """-> the EDMTrainer of the command line `a`, resumed if the configuration asks for it."""
    if a.MODE not in MODES:
        raise NotImplementedError
    name, dataset_class = MODES[a.MODE]
    args = diffusion.load_config(a.CONFIG if a.CONFIG is not None else name)
    if a.DSET_PATH is not None:
        args.dset.path = a.DSET_PATH
    if a.MODEL_DIR is not None:
        args.model_dir = a.MODEL_DIR
    args.exp.model_dir = args.model_dir
    device = torch.device(a.DEVICE if a.DEVICE is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    if device.type != "cuda" and (a.BACKEND, a.OPTIMIZER, a.FEEDER) != ("torch", "adam", "host"):
        raise RuntimeError(f"train_diffusion: --BACKEND hip, --OPTIMIZER fused and --FEEDER device are HIP device only (no CPU "
                           f"fallback) and the device is {device}; the CPU runs --BACKEND torch --OPTIMIZER adam --FEEDER host")

    dataset_obj = dataset_class(args.dset, seed=a.SEED)
    torch.manual_seed(a.SEED)
    network = diffusion.UNet1D(args, device).to(device)
    betas = (args.train.optimizer.beta1, args.train.optimizer.beta2)
    adam = optim.FusedAdam if a.OPTIMIZER == "fused" else torch.optim.Adam
    optimizer = adam(network.parameters(), lr=args.train.lr, betas=betas, eps=args.train.optimizer.eps)
    if a.FEEDER == "device":
        dset = datasets_diffusion.DeviceSegmentFeeder(dataset_obj, args.train.batch, args.exp.sample_rate, device)
    else:
        dset = iter(torch.utils.data.DataLoader(dataset=dataset_obj, batch_size=args.train.batch, num_workers=0))
    torch.manual_seed(np.random.randint(1 << 31))              # the reference's Trainer.__init__
    trainer = diffusion.EDMTrainer(args, network, optimizer, device, backend=a.BACKEND, dset=dset)
    if args.train.resume:
        path = args.train.get("resume_checkpoint", "None")
        resuming = trainer.resume_from_checkpoint(checkpoint_path=path) if path != "None" else trainer.resume_from_checkpoint()
        if resuming:
            print("Resuming from iteration {}".format(trainer.it))
        else:
            print("Could not resume from checkpoint")
            print("training from scratch")
            trainer.it, trainer.latest_checkpoint = 0, None
    return trainer


def main(argv=None):
    a = parser().parse_args(argv)
    trainer = build(a)
    args = trainer.args
    os.makedirs(args.model_dir, exist_ok=True)
    print()
    print('Training options:')
    print()
    print(f'Output directory:        {args.model_dir}')
    print(f'Batch size:              {args.train.batch}')
    print()

    def log(it, loss):
        if it % a.LOG_EVERY == 0:
            print(json.dumps({"it": it, "loss": float(loss)}), flush=True)

    trainer.training_loop(max_it=a.MAX_IT, log=log)
    return trainer


if __name__ == "__main__":
    main()
