#!/usr/bin/env python3
"""Golden g24: one epoch of the reference's own DiffDelRNN.train_epoch (code/model.py:426-511) on DiffDelGRU-HS[64], run here by
importing the reference as tools/make_goldens_train.py does (whose ESR / DCPreESR restatements and RecordingAdam are reused).
The model starts from the exported DiffDelGRU-HS[64] checkpoint (weights.W_DIFFDEL) with max_delay = 551, so its delay buffer
holds D = 552 samples; the dataset shim gives fs = 44100 and an analyser max_delay of 441 samples, so TBPTT_INIT = 512 < D (the
first window's taps also read buffer entries that are the initial zeros, with no gradient).  Two batches of (4, 1, 512 + 3 * 2048)
input / target pairs: six windows of 2048 samples.  The four streams of a batch carry four kinds of delay trajectory (in
seconds; the delays are the fp32 product with fs, as the reference forms them), all within [0, D]:
  0  smooth wow + flutter;
  1  piecewise-constant whole samples (weights exactly 0 and 1), with jumps up and down;
  2  a sawtooth that rises faster than one sample per sample (so q = n - floor(d) is not monotone) and drops fast, with
     stretches of slope ~1 where one buffer position receives many terms;
  3  one that sits at d = D.
Run once with ESR and once with DCPreESR.  Nothing of the reference travels: only inputs and outputs.
usage: python tools/make_goldens_train_diffdel.py [/root/reference]
    -> tests/golden/g24_train_diffdel_inputs.npz, g24_train_diffdel_esr.npz, g24_train_diffdel_dcpreesr.npz"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens_train as g23  # noqa: E402  (imports the reference's model module)

from ntm_amd import weights  # noqa: E402

ROOT = g23.ROOT
SEED, N_BATCHES, B, INIT, WIN, NWIN = 24, 2, 4, 512, 2048, 3
T = INIT + NWIN * WIN
FS = 44100
MAX_DELAY = 551                  # the model's max_delay: D = 552
ANALYSER_MAX_S = 441.0 / FS      # nextpow2(int(441.0000x)) = 512
LR = 1e-3


def _exact_seconds(v):
    """An fp32 s with fp32(s) * fs == v, or None (not every whole number of samples has one)."""
    s0 = np.float32(v / FS)
    for c in [s0] + [np.float32(s0 + k * np.spacing(s0)) for k in (-3, -2, -1, 1, 2, 3)]:
        if c * np.float32(FS) == np.float32(v):
            return c
    return None


def seconds_for(samples):
    """fp32 seconds s with fp32(s) * fs == samples exactly where that exists (whole samples and d = D), nearest otherwise,
    and never above D."""
    s = (samples.astype(np.float64) / FS).astype(np.float32)
    for idx in zip(*np.nonzero(samples == np.round(samples))):
        e = _exact_seconds(float(samples[idx]))
        if e is not None:
            s[idx] = e
    while (s * np.float32(FS) > MAX_DELAY + 1).any():
        s = np.where(s * np.float32(FS) > MAX_DELAY + 1, np.nextafter(s, np.float32(-np.inf)), s)
    return s.astype(np.float32)


def trajectories(rng):
    n = np.arange(T, dtype=np.float64)
    D = MAX_DELAY + 1
    ph = rng.uniform(0, 2 * np.pi, 3)
    wow = 300 + 150 * np.sin(2 * np.pi * n / 5000 + ph[0]) + 3.0 * np.sin(2 * np.pi * n / 300 + ph[1])
    exact = np.array([v for v in range(D + 1) if _exact_seconds(float(v)) is not None])
    assert exact[-1] == D
    steps = rng.choice(exact, T // 700 + 1)
    steps[1] = D
    whole = steps[(n // 700).astype(int)].astype(np.float64)
    saw = np.zeros(T)
    v = 50.0
    for i in range(T):
        phase = i % 900
        if phase < 150:
            v += 1.7                     # faster than one sample per sample: q falls
        elif phase < 600:
            v += 0.999                   # one buffer position collects many terms
        else:
            v -= 1.9                     # falls fast
        v = min(max(v, 0.0), D - 0.5)
        saw[i] = v
    at_d = np.clip(300 + 320 * np.sin(2 * np.pi * n / 3000 + ph[2]), 5.0, D)     # flat at D (exact) for a while
    d = np.stack([wow, whole, saw, at_d])
    assert d.min() >= 0 and d.max() <= D
    return seconds_for(d)


class Shim(list):
    """A list of batches with the attributes the reference's train_epoch reads from dataloader.dataset."""

    class _DS:
        fs = FS

        class delay_analyzer:
            max_delay = ANALYSER_MAX_S

    dataset = _DS


def data():
    rng = np.random.default_rng(SEED)
    out = []
    for _ in range(N_BATCHES):
        x = rng.uniform(-0.5, 0.5, (B, 1, T)).astype(np.float32)
        t = (0.6 * np.tanh(2.0 * x) + 0.05 * np.roll(x, 3, axis=2) + 0.01 * rng.standard_normal(x.shape)).astype(np.float32)
        out.append((x, t, trajectories(rng)))
    return out


def main():
    batches = data()
    inp = {"x": np.stack([b[0] for b in batches]), "t": np.stack([b[1] for b in batches]), "traj_s": np.stack([b[2] for b in batches]),
           "meta": np.array([SEED, N_BATCHES, B, T, INIT, WIN, MAX_DELAY, FS]), "analyser_max_delay_s": np.array(ANALYSER_MAX_S),
           "lr": np.array(LR), "R": np.array(g23.R, dtype=np.float32)}
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g24_train_diffdel_inputs.npz"), **inp)
    d = torch.from_numpy(inp["traj_s"]) * FS
    print("delay range", float(d.min()), float(d.max()), "D", MAX_DELAY + 1)
    sd0 = weights.load_state_dict(weights.W_DIFFDEL)
    for name, fn in (("esr", g23.esr), ("dcpreesr", g23.dcpre_esr)):
        torch.manual_seed(0)
        m = g23.ref_model.DiffDelRNN(1, 64, 1, max_delay=MAX_DELAY)
        m.load_state_dict(sd0)
        opt = g23.RecordingAdam(m.parameters(), lr=LR)
        losses = []

        def loss_fcn(p, t):
            v = fn(p, t)
            losses.append(float(v.detach()))
            return v

        loader = Shim((torch.from_numpy(x), torch.from_numpy(t), {"delay_trajectory": torch.from_numpy(tr)}) for x, t, tr in batches)
        epoch = m.train_epoch(loader, loss_fcn, opt)
        out = {"epoch_loss": np.array(epoch), "losses": np.array(losses, dtype=np.float64)}
        keys = [k for k, _ in m.named_parameters()]
        out["keys"] = np.array(keys)
        for k in keys:
            out[f"grad__{k}"] = np.stack([g[keys.index(k)].numpy() for g in opt.grads]).astype(np.float32)
        for k, v in m.state_dict().items():
            out[f"final__{k}"] = v.numpy().copy()
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", f"g24_train_diffdel_{name}.npz"), **out)
        print(name, "epoch loss", epoch, "windows", len(losses), [f"{v:.6f}" for v in losses])


if __name__ == "__main__":
    main()
