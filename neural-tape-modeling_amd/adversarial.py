"""The adversarial training loop of the reference (code/train-adversarial.py) on the device: `load_config` restates
configs/AdversarialConfig.py, `Trainer` runs the loop of code/train-adversarial.py:123-317 on a DiffDelRNN generator and one of
ntm_amd.critics' critics.  Both losses are training.AdvHeadFn (csrc/advhead_kernels.hip), one graph node per call.

What the loop computes is the reference's, statement for statement, with three deliberate differences:

 1. The fakes of the critic phase are made under torch.no_grad(), where the reference uses torch.inference_mode().  The engine
    returns float32 where the reference's delay line returns float64, so the script's `.float()` copies nothing, and an
    inference tensor cannot be saved for backward by the graph nodes of the waveform critics.  The numbers are the same: under
    no_grad the generator takes the inference kernels, whose outputs and carried state are bit-identical to the grad-mode
    forward's.  The critic phase's warm-up runs under no_grad as well: its graph is never used (the reference builds and drops it).
 2. One critic pass per window over torch.cat([fake, real]) (2 B streams) instead of a pass over each (`stacked=True`, the
    default; `stacked=False` is the two-call form).  The critics' kernels give a stream the same output whatever its batch, so
    the outputs and the loss terms are the same bits; the weight gradient is one sum over 2 B streams instead of two
    accumulated sums.
 3. In the generator phase the critic's parameter gradients are not computed (its parameters are switched to
    requires_grad=False for the step, which the conv stacks' backward entry points honour with NULL outputs).  In the reference
    they land in `.grad` and are zeroed by the next `Critic.zero_grad()` before any optimizer reads them; here the critic's
    `.grad` keeps the critic phase's sums until then.

One property of the reference is kept although it looks unintended: `sample_offset` is set to `train_init` in front of both
window loops and never advanced (code/train-adversarial.py:266-280, :307-317), so every window of a segment reads the SAME
tbptt_len samples behind the warm-up while the generator's state moves on.  `Trainer.advance_windows = True` walks through the
segment instead."""
import os

import torch

from . import critics, training

CONFIGS = (0, 1, 2, 3, 4, 5, 6, 7, 10)

_DATASETS = {"chowtape": "ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER",
             "akai": "ReelToReel_Dataset_MiniPulse100_AKAI_IPS[7.5]_MAXELL"}


def _spec_crit(scales, kernel_sizes, hop_sizes, tf_rep):
    return {"crit": "MultiSpecCrit",
            "crit_pars": {"scales": list(scales), "kernel_sizes": list(kernel_sizes), "hop_sizes": list(hop_sizes), "layers": 4,
                          "chan_in": 16, "chan_fac": 4, "stride": 1, "g_fac": 16, "tf_rep": tf_rep, "log": True},
            "crit_lr": 0}


def load_config(n):
    """The dict configs/AdversarialConfig.py: main(n) returns, restated: configurations 0-3 train on the CHOWTAPE wow-and-flutter
    set and 4-7 on the AKAI set with, in turn, the MelGAN critic, the spectral critic, the mel-spectral critic and the dilated
    time-domain critic; 10 is the CHOWTAPE set with the three-scale spectral critic.  A fresh dict per call (get_critic writes
    `test_in_len` into `crit_pars`).  Any other n: ValueError."""
    if isinstance(n, bool) or not isinstance(n, int) or n not in CONFIGS:
        raise ValueError(f"load_config: configuration {n!r} is not defined; built: {', '.join(str(c) for c in CONFIGS)}")
    d = {"segment_length": 44100 * 2, "tbptt_length": 8192 * 2, "val_segment_length": 44100 * 10, "gen_lr": 0.0001, "val_freq": 1,
         "hid_size": 64, "batch_size": 16, "model_path": "../models/"}
    d["dataset_path"] = _DATASETS["chowtape" if n in (0, 1, 2, 3, 10) else "akai"]
    critic = 5 if n == 10 else n % 4
    if critic == 0:
        crit = {"crit": "MelGanCrit", "crit_pars": {"num_D": 3, "ndf": 16, "n_layers": 4, "downsampling_factor": 4}, "crit_lr": 0}
    elif critic in (1, 2):
        crit = _spec_crit([128, 256, 512, 1024], [21, 21, 21, 17], [32, 64, 128, 128], "spec" if critic == 1 else "mel")
    elif critic == 3:
        crit = {"crit": "DilatedConvDisc", "crit_pars": {}, "crit_lr": 0}
    else:
        crit = _spec_crit([512, 1024, 2048], [21, 17, 7], [64, 64, 64], "spec")
    d.update(crit)
    return d


def delay_range(dataset):
    """(d_min, d_max) in seconds as `Trainer` takes them: `min_d` / `max_d` of the reference's VADataset (0-dim tensors), or
    `min_delay` / `max_delay` of a SegmentFeeder (floats)."""
    if hasattr(dataset, "min_d"):
        return dataset.min_d, dataset.max_d
    return dataset.min_delay, dataset.max_delay


def critic_heads(critic, D):
    """The tensors of a critic's output that its losses read, as a list: a MultiSpecCrit's list itself, [D] of a
    DilatedConvDisc, the last layer's output of every discriminator of a MelGCrit."""
    if isinstance(critic, critics.MelGCrit):
        return [scale[-1] for scale in D]
    if isinstance(critic, critics.MultiSpecCrit):
        return list(D)
    if isinstance(critic, critics.DilatedConvDisc):
        return [D]
    raise RuntimeError(f"adversarial: {type(critic).__name__} is not one of ntm_amd.critics' critics ({critics.SUPPORTED})")


class Trainer:
    """The loop of code/train-adversarial.py:123-317 around `generator` (DiffDelRNN(1, 64, 1, skip=False)), `critic` (from
    critics.get_critic) and their optimizers, all on a HIP device (RuntimeError otherwise: there is no CPU path).

    tbptt_len: samples per window; fs: sampling rate; d_min, d_max: the shortest and longest delay of the training set in SECONDS
    (`delay_range(dataset)`: tensors or floats; the arithmetic below runs on them as given, as in the reference):
        train_d_min = d_min * fs - 1,  train_d_max = d_max * fs + 1,
        train_init = max(int(train_d_max - train_d_min) + 2, 1024)   samples of warm-up AND the generator's delay-line length,
        d_traj_offset = int(train_d_min) - 1                         subtracted from every delay.
    Batches: the reference's (input, target, meta) with meta['delay_trajectory'] (B, T) in seconds, or SegmentFeeder.batches'
    (input, target, d_seconds (B, 1, T), metas); only the audio channel (channel 0) is kept.  The delays are formed as the
    reference forms them, `traj.unsqueeze(1) * fs - d_traj_offset` in the trajectory's own dtype, with its two range asserts.

    stacked: one critic pass over cat([fake, real]) per window (default) or the reference's two passes (module docstring).
    log(dict, step=None): called where the reference calls wandb.log (wandb is neither needed nor imported).
    model_path: the directory of the checkpoints `validate` writes; dry_run=True (or no model_path) writes nothing.
    On construction the generator's parameters are set to requires_grad."""

    advance_windows = False         # False: every window reads the samples right behind the warm-up, as the reference does

    def __init__(self, generator, critic, optG, optC, tbptt_len, fs, d_min, d_max, stacked=True, log=None, model_path=None,
                 dry_run=False):
        for what, module in (("generator", generator), ("critic", critic)):
            for p in module.parameters():
                if not p.is_cuda:
                    raise RuntimeError(f"adversarial.Trainer: the {what}'s parameters are on '{p.device}': HIP device only "
                                       "(no CPU fallback)")
        generator._check_trainable("adversarial.Trainer")
        if not isinstance(critic, (critics.MelGCrit, critics.MultiSpecCrit, critics.DilatedConvDisc)):
            critic_heads(critic, None)              # raises: not one of the built families
        self.generator, self.critic, self.optG, self.optC = generator, critic, optG, optC
        self.tbptt_len, self.fs = int(tbptt_len), fs
        self.train_d_min, self.train_d_max = d_min * fs - 1, d_max * fs + 1
        self.train_init = max(int(self.train_d_max - self.train_d_min) + 2, 1024)
        self.d_traj_offset = int(self.train_d_min) - 1
        self.stacked = bool(stacked)
        self.log = log if log is not None else (lambda values, step=None: None)
        self.model_path, self.dry_run = model_path, bool(dry_run) or model_path is None
        self.crit_step = 0
        self.gen_step = 0
        self.device = generator.GRU.weight_hh_l0.device
        for p in generator.parameters():
            p.requires_grad_(True)

    # ---- batches
    @staticmethod
    def _trajectory(batch):
        """The delay trajectory of a batch in seconds as (B, 1, T): `meta['delay_trajectory'].unsqueeze(1)` of the reference's
        batches, channel 0 of SegmentFeeder.batches' d_seconds."""
        extra = batch[2]
        if isinstance(extra, dict):
            return extra["delay_trajectory"].unsqueeze(1)
        if extra is None:
            raise RuntimeError("adversarial.Trainer: the batch carries no delay trajectory")
        return extra[:, :1, :]

    @staticmethod
    def _audio(x):
        """Only consider audio for training: channel 0."""
        return x[:, :1, :] if x.shape[1] > 1 else x

    def _train_inputs(self, batch):
        """(input, delays in samples) of a training batch on the device, after the reference's two range asserts."""
        x = self._audio(batch[0])
        d_traj = self._trajectory(batch) * self.fs - self.d_traj_offset
        assert self.train_init > torch.max(d_traj), f"{self.train_init} > {torch.max(d_traj)}"
        assert 0 < torch.min(d_traj)
        return x.to(self.device), d_traj.to(self.device)

    def _windows(self, T):
        """The sample ranges of the whole windows behind the warm-up."""
        n = (T - self.train_init) // self.tbptt_len
        step = self.tbptt_len if self.advance_windows else 0
        return [slice(self.train_init + k * step, self.train_init + k * step + self.tbptt_len) for k in range(max(n, 0))]

    # ---- the two steps
    def critic_step(self, fake, real):
        """One `Critic.train_crit(fake, real, optC)`: forward, hinge loss, backward, optC.step() -- no zero_grad (the caller zeroes
        once per batch, so the gradients accumulate over the windows of a batch, as in the reference).  -> the loss as a float."""
        fake, real = fake.float(), real.float()
        if self.stacked:
            outs = critic_heads(self.critic, self.critic(torch.cat([fake, real])))
        else:
            outs = [torch.cat(pair) for pair in zip(critic_heads(self.critic, self.critic(fake)),
                                                    critic_heads(self.critic, self.critic(real)))]
        loss_D = training.AdvHeadFn.apply("crit", fake.shape[0], *outs)
        loss_D.backward()
        self.optC.step()
        return loss_D.item()

    def generator_step(self, x_win, d_win):
        """One window of the generator phase: grad-mode `generator(x_win, d_win)`, the critic on its output, `Critic.train_gen`'s
        loss, backward, optG.step(), generator.detach_hidden(), generator.zero_grad().  -> the loss as a float."""
        gen_out_mini, _ = self.generator(x_win, d_win)
        frozen = [p for p in self.critic.parameters() if p.requires_grad]
        for p in frozen:
            p.requires_grad_(False)
        try:
            outs = critic_heads(self.critic, self.critic(gen_out_mini.float()))
        finally:
            for p in frozen:
                p.requires_grad_(True)
        loss_G = training.AdvHeadFn.apply("gen", 0, *outs)
        loss_G.backward()
        self.optG.step()
        self.generator.detach_hidden()
        self.generator.zero_grad()
        return loss_G.item()

    # ---- one epoch of training
    def train_epoch(self, inp_gen, inp_crit, tgt_crit):
        """code/train-adversarial.py:232-317 over the three loaders zipped: per iteration the critic phase (Critic.zero_grad(); the
        generator re-initialised and warmed up on the first train_init samples; per whole window the fakes and a critic_step
        against the same window of `tgt_crit`'s targets), then the generator phase (re-initialised; warmed up WITH grad, as in
        the reference: the first window's backward reaches the warm-up; zero_grad; per window a generator_step).  Windows per
        segment: (T - train_init) // tbptt_len.  -> (critic losses, generator losses), one float per window in order."""
        G = self.generator
        crit_losses, gen_losses = [], []
        for b_gen, b_crit, b_tgt in zip(inp_gen, inp_crit, tgt_crit):
            # Train Critic
            self.critic.zero_grad()
            crit_in, d_traj_cin = self._train_inputs(b_crit)
            crit_tgt = self._audio(b_tgt[1]).to(self.device)
            G.initialize_hidden(crit_in.shape[0], self.train_init)
            with torch.no_grad():
                G(crit_in[:, :, :self.train_init], d_traj_cin[:, :, :self.train_init], warmup=True)
            G.zero_grad()
            for sl in self._windows(crit_in.shape[-1]):
                with torch.no_grad():
                    crit_in_mini, _ = G(crit_in[:, :, sl], d_traj_cin[:, :, sl])
                loss_crit = self.critic_step(crit_in_mini, crit_tgt[:, :, sl])
                self.log({"loss/critic": loss_crit}, step=self.crit_step)
                self.crit_step += 1
                crit_losses.append(loss_crit)

            # Train Generator
            G.zero_grad()
            gen_in, d_traj_gin = self._train_inputs(b_gen)
            G.initialize_hidden(gen_in.shape[0], self.train_init)
            G(gen_in[:, :, :self.train_init], d_traj_gin[:, :, :self.train_init], warmup=True)
            G.zero_grad()
            for sl in self._windows(gen_in.shape[-1]):
                loss_gen = self.generator_step(gen_in[:, :, sl], d_traj_gin[:, :, sl])
                self.log({"loss/gen": loss_gen}, step=self.gen_step)
                self.gen_step += 1
                gen_losses.append(loss_gen)
        return crit_losses, gen_losses

    # ---- validation and checkpoints
    @torch.no_grad()
    def validate(self, loader, evaluator, d_max, epoch=None):
        """code/train-adversarial.py:136-169: per batch the generator is re-initialised with a delay line of
        val_d_max = d_max * fs + 1 samples (d_max: the validation set's longest delay in SECONDS) and no warm start, the delays are
        `traj * fs`, the segment is forwarded and `evaluator.add_loss(pred.squeeze().float(), target.squeeze().float())` is
        called.  -> (pred, pre_d) of the last batch.
        A float64 trajectory is handed to the delay line in float64 (DiffDelRNN.forward_f64_delays), as the reference's delay
        line sees it; the training windows round their delays to float32, which the graph nodes take.
        The reference forwards the segment in chunks of tbptt_len; here it is ONE forward per batch (chunked == one-shot bit
        for bit, state carried either way).  Its chunk count is the ceiling of T / tbptt_len when tbptt_len does not divide T and
        DOUBLE that quotient when it does -- the surplus chunks are then empty slices; the ceiling is what is computed here.
        With `epoch` given the bookkeeping around the pass runs too (:132-134, :205-214): `running{epoch}.pth` is written before
        it, `evaluator.end_val(epoch)` is called after it, every loss is logged, and `{key}best.pt` is written for every key
        whose best epoch is this one.  Nothing is written with dry_run=True or without a model_path."""
        G = self.generator
        if epoch is not None and not self.dry_run:
            os.makedirs(self.model_path, exist_ok=True)
            torch.save(G.state_dict(), os.path.join(self.model_path, "running") + str(epoch) + ".pth")
        val_d_max = d_max * self.fs + 1
        pred = pre_d = None
        for batch in loader:
            input, target = self._audio(batch[0]), self._audio(batch[1])
            d_traj = self._trajectory(batch) * self.fs
            input, target, d_traj = input.to(self.device), target.to(self.device), d_traj.to(self.device)
            G.initialize_hidden(input.shape[0], val_d_max)
            # a float64 trajectory (the reference's VADataset(double=True)) keeps its precision down to the interpolation weights
            pred, pre_d = G.forward_f64_delays(input, d_traj) if d_traj.dtype == torch.float64 else G(input, d_traj)
            evaluator.add_loss(pred.squeeze().float(), target.squeeze().float())
        if epoch is not None:
            evaluator.end_val(epoch)
            for key in evaluator.bst_losses:
                n = "loss/" + key
                value = evaluator.losses[key]
                self.log({n: value, "epoch": epoch})
                if evaluator.bst_losses[key][0] == epoch:
                    self.log({"best_" + n: value, "epoch": epoch})
                    if not self.dry_run:
                        torch.save(G.state_dict(), os.path.join(self.model_path, key + "best.pt"))
        return pred, pre_d
