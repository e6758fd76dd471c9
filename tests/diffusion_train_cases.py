"""What tests/test_diffusion_train_cpu.py and tests/test_gpu_diffusion_train.py share: the g30 goldens
(tools/make_goldens_diffusion_train.py: the reference's EDM training, three iterations of B = 4 x 512 on its UNet1D with the
toytrajectories configuration, in float32 and float64), the network and trainer built on the exported initialisation, the
replay and the error bar.

The bar of a float32 result is diffusion_cases': 3 x the reference's own float32-against-float64 distance, both in max norm
relative to max |ref64| -- computed here from the golden, never from the code under test."""
import functools
import os

import numpy as np
import torch

from ntm_amd import diffusion

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("g30_diffusion_train.npz", "g30_diffusion_train_grads64.npz", "g30_diffusion_train_ref32.npz",
         "g30_diffusion_train_final64.npz")
B, T, ITERS = 4, 512, 3


@functools.lru_cache(None)
def arrays():
    """name -> array; the gradients of the two runs as grad64_<key> / grad32_<key>."""
    out = {}
    for f in FILES:
        with np.load(os.path.join(GOLDEN, f)) as z:
            for k in z.files:
                name = k
                if k.startswith("grad_") and f != FILES[0]:
                    name = ("grad64_" if "grads64" in f else "grad32_") + k[5:]
                out[name] = z[k]
    return out


def param_keys():
    return str(arrays()["param_keys"]).split(";")


def trained_keys():
    """The parameters that receive a gradient (RFF_freq is frozen)."""
    return [k for k in param_keys() if "grad64_" + k in arrays()]


def init_state(dtype=torch.float32):
    a = arrays()
    return {k: torch.from_numpy(a["init_" + k].copy()).to(dtype) if a["init_" + k].dtype != np.int64 else torch.from_numpy(a["init_" + k].copy())
            for k in str(a["keys"]).split(";")}


def final(kind, tag, key):
    """kind "net" | "ema", tag "32" | "64" -> the recorded parameter after the third iteration, float64."""
    a = arrays()
    return a["init_" + key].astype(np.float64) + a[f"{kind}{tag}d_{key}"].astype(np.float64)


def config():
    return diffusion.load_config("toytrajectories")


def network(device="cpu", dtype=torch.float32):
    net = diffusion.UNet1D(config(), device)
    net.load_state_dict(init_state())
    return net.to(dtype)


def trainer(device="cpu", dtype=torch.float32, backend="torch"):
    args, net = config(), network(device, dtype)
    opt = torch.optim.Adam(net.parameters(), lr=args.train.lr, betas=(args.train.optimizer.beta1, args.train.optimizer.beta2),
                           eps=args.train.optimizer.eps)
    return diffusion.EDMTrainer(args, net, opt, device, backend=backend)


def batch(i, device="cpu", dtype=torch.float32):
    """-> x (B, T), draws = (a (B,), noise (B, T)) of iteration i."""
    a = arrays()
    return (torch.from_numpy(a["x"][i]).to(device, dtype),
            (torch.from_numpy(a["a"][i]).to(dtype), torch.from_numpy(a["noise"][i]).to(dtype)))


def replay(tr, device="cpu", dtype=torch.float32):
    """Iteration 0's gradients from a step of its own, then the three iterations -> dict of what g30 records."""
    x, draws = batch(0, device, dtype)
    tr.optimizer.zero_grad()
    error, sigma = tr.loss_fn(x, draws)
    error.mean().backward()
    out = {"grads": {k: p.grad.detach().double().cpu().numpy().copy() for k, p in tr.network.named_parameters() if p.grad is not None},
           "sigma0": sigma.detach().double().cpu().numpy(), "loss": [], "lr": [], "grad_norm": []}
    for i in range(ITERS):
        x, draws = batch(i, device, dtype)
        out["loss"].append(float(tr.iteration(x, draws)))
        out["lr"].append(tr.lr)
        out["grad_norm"].append(float(tr.grad_norm))
    out["net"] = {k: p.detach().double().cpu().numpy() for k, p in tr.network.named_parameters()}
    out["ema"] = {k: p.detach().double().cpu().numpy() for k, p in tr.ema.named_parameters()}
    return out


def rel_err(got, ref64):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref64 = np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    return float(np.max(np.abs(got.astype(np.float64) - ref64)) / np.max(np.abs(ref64)))


def bar_of(ref32, ref64):
    ref64 = np.asarray(ref64, np.float64)
    return 3.0 * float(np.max(np.abs(np.asarray(ref32).astype(np.float64) - ref64)) / np.max(np.abs(ref64)))


def hold(what, got, ref32, ref64, worst=None):
    """Print the figure in diffusion_cases.check's format, then hold it against the bar.  A reference that is identically zero
    asks for exact zeros.  worst: a dict that keeps the largest ratio seen per kind of tensor (the first word of `what`)."""
    ref64 = np.asarray(ref64, np.float64)
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    if not np.any(ref64):
        print(f"{what}: the reference is identically zero")
        assert not np.any(got), what
        return 0.0
    e, b = rel_err(got, ref64), bar_of(ref32, ref64)
    ratio = 3.0 * e / b if b > 0 else (0.0 if e == 0 else float("inf"))
    print(f"{what}: error {e:.3e}, bar {b:.3e}, ratio to the reference's own float32 error {ratio:.2f}")
    if worst is not None:
        kind = what.split()[0]
        worst[kind] = max(worst.get(kind, 0.0), ratio)
    assert e <= b, (what, e, b)
    return e
