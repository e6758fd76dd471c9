#!/usr/bin/env python3
"""Golden g23: one epoch of the reference's own RNN.train_epoch (code/model.py:90-161) on GRU-HS[64], run here by importing the
reference (torchaudio / soundfile / librosa stubbed as in tools/make_goldens.py).  The model starts from the exported
GRU-HS[64] checkpoint (weights.W_GRU); the epoch is two batches of seeded (4, 1, 4096) input / target pairs, so three TBPTT
windows of 1024 samples per batch behind the 1024-sample warm-up; the optimizer is torch.optim.Adam(lr=1e-3) (code/train.py:181),
subclassed to record every p.grad just before step().  Run once with ESR and once with DCPreESR; both losses are restated in
torch here (the reference's own come from un-vendored packages): the definitions of ntm_amd.ESRLoss / ntm_amd.DCPreESR, with
fp64 sums.  Nothing of the reference travels: only inputs and outputs.
usage: python tools/make_goldens_train.py [/root/reference]
    -> tests/golden/g23_train_inputs.npz, g23_train_esr.npz, g23_train_dcpreesr.npz"""
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for name in ("torchaudio", "soundfile", "librosa", "librosa.filters"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["librosa.filters"].mel = lambda *a, **k: None
sys.modules["librosa"].filters = sys.modules["librosa.filters"]
sys.path.insert(0, os.path.join(REF, "code"))
sys.path.insert(0, ROOT)
import model as ref_model  # noqa: E402

from ntm_amd import weights  # noqa: E402

SEED, N_BATCHES, B, T = 23, 2, 4, 4096
R = float(np.float32(0.995))        # the pole as the kernels hold it (fp32)
LR = 1e-3


def esr(output, target):
    """ntm_amd.ESRLoss: mean (t - y)^2 / (mean t^2 + 1e-5) over the whole tensor, fp64 sums, fp32 result."""
    y, t = output.double(), target.double()
    n = y.numel()
    return ((((t - y) ** 2).sum() / n) / ((t ** 2).sum() / n + 1e-5)).float()


def _dc_matrix(n):
    """The DC blocker (1 - z^-1)/(1 - R z^-1) from zero state as a lower-triangular Toeplitz matrix (impulse response
    h[0] = 1, h[k] = R^(k-1) (R - 1)), fp64."""
    k = np.arange(n)
    h = np.where(k == 0, 1.0, R ** np.maximum(k - 1, 0) * (R - 1.0))
    d = k[:, None] - k[None, :]
    return torch.from_numpy(np.where(d >= 0, h[np.maximum(d, 0)], 0.0))


def dcpre_esr(output, target):
    """ntm_amd.DCPreESR(dc_pre=True): the ESR of the DC-blocked signals (zero state at the start of the tensor)."""
    M = _dc_matrix(output.shape[-1])
    y, t = output.double() @ M.T, target.double() @ M.T
    n = y.numel()
    return ((((t - y) ** 2).sum() / n) / ((t ** 2).sum() / n + 1e-5)).float()


class RecordingAdam(torch.optim.Adam):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.grads = []

    def step(self, closure=None):
        self.grads.append([p.grad.detach().clone() for g in self.param_groups for p in g["params"]])
        return super().step(closure)


def data():
    rng = np.random.default_rng(SEED)
    out = []
    for _ in range(N_BATCHES):
        x = rng.uniform(-0.5, 0.5, (B, 1, T)).astype(np.float32)
        t = (0.6 * np.tanh(2.0 * x) + 0.05 * np.roll(x, 3, axis=2) + 0.01 * rng.standard_normal(x.shape)).astype(np.float32)
        out.append((x, t))
    return out


def main():
    batches = data()
    inp = {"x": np.stack([b[0] for b in batches]), "t": np.stack([b[1] for b in batches]),
           "meta": np.array([SEED, N_BATCHES, B, T]), "lr": np.array(LR), "R": np.array(R, dtype=np.float32)}
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g23_train_inputs.npz"), **inp)
    sd0 = weights.load_state_dict(weights.W_GRU)
    for name, fn in (("esr", esr), ("dcpreesr", dcpre_esr)):
        torch.manual_seed(0)
        m = ref_model.RNN(1, 64, 1)
        m.load_state_dict(sd0)
        opt = RecordingAdam(m.parameters(), lr=LR)
        losses = []

        def loss_fcn(p, t):
            v = fn(p, t)
            losses.append(float(v.detach()))
            return v

        loader = [(torch.from_numpy(x), torch.from_numpy(t), None) for x, t in batches]
        epoch = m.train_epoch(loader, loss_fcn, opt)
        out = {"epoch_loss": np.array(epoch), "losses": np.array(losses, dtype=np.float64)}
        keys = [k for k, _ in m.named_parameters()]
        out["keys"] = np.array(keys)
        for k in keys:
            out[f"grad__{k}"] = np.stack([g[keys.index(k)].numpy() for g in opt.grads]).astype(np.float32)
        for k, v in m.state_dict().items():
            out[f"final__{k}"] = v.numpy().copy()
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", f"g23_train_{name}.npz"), **out)
        print(name, "epoch loss", epoch, "windows", len(losses), [f"{v:.6f}" for v in losses])


if __name__ == "__main__":
    main()
