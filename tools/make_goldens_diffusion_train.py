#!/usr/bin/env python3
"""Golden g30: the reference's EDM training (code/train-diffusion.py) on the CPU.

Dev-only script: it reads the reference's script from a checkout given on the command line, executes it as it stands (its
`main` is guarded) and never travels.  What is not installed where this runs gets stand-ins: torchaudio (the Resample of
tools/make_goldens_diffusion.py: torchaudio's own rule on ntm_amd.diffusion's filters), soundfile, omegaconf, and the empty
package edm.torch_utils (training_stats.report returns its value).  The class EDM runs unchanged; Trainer is the reference's with
get_batch() alone replaced (the batch comes from here, in the run's dtype, not from a DataLoader through torch.Tensor), and its
train_step / update_ema / `it += 1` run as the reference's training_loop orders them.  Printing is swallowed.

Case: the reference's UNet1D with the toytrajectories configuration under torch.manual_seed(30); the CombinerUp 1x1s, which the
reference initialises to zero (so that at first only they receive a gradient), are redrawn with Conv1d's default rule under the
same seed -- every parameter then has a gradient from iteration 0.  Adam as _main builds it.  B = 4, T = 512, three iterations.
torch.rand / torch.randn are replaced, while a step runs, by the recorded draws a (B,) and noise (B, T) of that iteration.
Everything runs twice: in float32 as the reference stands (ref32) and with the modules, the batch and the draws in float64 holding
the same float32 values (ref64).

Recorded (tests/golden/, each file below 1 MiB):
  g30_diffusion_train.npz          init_<key> the initial state dict; x (3, B, T), a (3, B), noise (3, B, T); per iteration and
                                   run: loss, sigma, grad_norm (before clipping), lr; keys / param_keys; net_out of iteration 0;
                                   ema32d_<key>
  g30_diffusion_train_grads64.npz  grad_<key>: every parameter's gradient at iteration 0, before clipping, float64
  g30_diffusion_train_ref32.npz    grad_<key> of the float32 run; net32d_<key>
  g30_diffusion_train_final64.npz  net64d_<key>, ema64d_<key>
  The final network and EMA parameters are stored as float32 DIFFERENCES from the initial value (three steps at a learning
  rate below 1e-6 move a weight by ~1e-6: the float32 rounding of the difference is ~1e-13 of the weight, far below any bar).

usage: python tools/make_goldens_diffusion_train.py <reference checkout>"""
import contextlib
import io
import math
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("NTM_REFERENCE", "")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
SCRIPT = os.path.join(REF, "code", "train-diffusion.py")
if not os.path.isfile(SCRIPT):
    sys.exit(__doc__)
sys.path.insert(0, ROOT)
from ntm_amd import diffusion as D  # noqa: E402

SEED, B, T, ITERS = 30, 4, 512, 3


class Resample(torch.nn.Module):
    def __init__(self, orig_freq, new_freq):
        super().__init__()
        g = math.gcd(int(orig_freq), int(new_freq))
        self.o, self.n = int(orig_freq) // g, int(new_freq) // g
        kernel, self.width = D.sinc_resample_kernel(self.o, self.n)
        self.register_buffer("kernel", kernel)

    def forward(self, x):
        return D.apply_resample_kernel(x, self.kernel, self.o, self.n, self.width)


def module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


ta = module("torchaudio", transforms=module("torchaudio.transforms", Resample=Resample),
            functional=module("torchaudio.functional", resample=lambda x, o, n: x if int(o) == int(n) else Resample(o, n)(x)))
module("soundfile")
module("omegaconf", OmegaConf=type("OmegaConf", (), {"load": staticmethod(D.load_config)}))
module("edm", torch_utils=module("edm.torch_utils", training_stats=module("edm.torch_utils.training_stats",
                                                                           report=lambda name, value: value)))
sys.path.insert(0, os.path.join(REF, "code"))
ref = types.ModuleType("ref_train_diffusion")
ref.__file__ = SCRIPT
with open(SCRIPT) as f:
    exec(compile(f.read(), SCRIPT, "exec"), ref.__dict__)      # __name__ is not "__main__": nothing runs

torch.set_num_threads(8)
rs = np.random.RandomState(SEED)
args = D.load_config("toytrajectories")
# the batch: sums of slow sinusoids at the data's scale (sigma_data), one batch per iteration
t = np.arange(T) / args.exp.sample_rate
x_all = np.zeros((ITERS, B, T))
for _ in range(6):
    f, ph, amp = rs.uniform(0.2, 8.0, (ITERS, B, 1)), rs.uniform(0, 2 * np.pi, (ITERS, B, 1)), rs.standard_normal((ITERS, B, 1))
    x_all += amp * np.sin(2 * np.pi * f * t + ph)
x_all = (args.diff_params.sigma_data * x_all / np.sqrt(3.0)).astype(np.float32)
a_all = rs.uniform(0, 1, (ITERS, B)).astype(np.float32)
noise_all = rs.standard_normal((ITERS, B, T)).astype(np.float32)


def initial_network():
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        net = ref.UNet1D(args, "cpu")
    for m in net.modules():
        if type(m).__name__ == "CombinerUp":
            torch.nn.init.kaiming_uniform_(m.conv1x1.weight, a=math.sqrt(5))
    return net


class Trainer(ref.Trainer):
    def get_batch(self):
        return next(self.dset)


def run(dt):
    net = initial_network().to(dt)
    init = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt = torch.optim.Adam(net.parameters(), lr=args.train.lr, betas=(args.train.optimizer.beta1, args.train.optimizer.beta2),
                           eps=args.train.optimizer.eps)
    batches = iter([torch.from_numpy(x).to(dt) for x in x_all])
    rec = {"loss": [], "sigma": [], "grad_norm": [], "lr": [], "grads": [], "net_out": []}
    with contextlib.redirect_stdout(io.StringIO()):
        trainer = Trainer(args, batches, net, opt, ref.EDM(args), "cpu")
    real = (torch.rand, torch.randn, torch.nn.utils.clip_grad_norm_, trainer.diff_params.loss_fn, opt.step)

    def clip(params, max_norm, *a, **k):
        params = list(params)
        rec["grads"].append([None if p.grad is None else p.grad.detach().clone() for p in params])
        norm = real[2](params, max_norm, *a, **k)
        rec["grad_norm"].append(float(norm))
        return norm

    def loss_fn(network, x):
        outs = []
        error, sigma = real[3](lambda inp, cn: (outs.append(network(inp, cn)), outs[-1])[1], x)
        rec["loss"].append(float(error.detach().mean()))
        rec["sigma"].append(sigma.detach().double().numpy().copy())
        rec["net_out"].append(outs[0].detach().clone())
        return error, sigma

    def step(*a, **k):
        rec["lr"].append(float(opt.param_groups[0]["lr"]))
        return real[4](*a, **k)

    trainer.diff_params.loss_fn, opt.step = loss_fn, step
    for i in range(ITERS):
        torch.rand = lambda n, i=i: torch.from_numpy(a_all[i]).to(dt)
        torch.randn = lambda shape, i=i: torch.from_numpy(noise_all[i]).to(dt)
        torch.nn.utils.clip_grad_norm_ = clip
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                trainer.train_step()
                trainer.update_ema()
                trainer.it += 1
        finally:
            torch.rand, torch.randn, torch.nn.utils.clip_grad_norm_ = real[:3]
    names = [k for k, _ in net.named_parameters()]
    return {"init": init, "names": names, "rec": rec, "net": dict(net.named_parameters()), "ema": dict(trainer.ema.named_parameters())}


r32, r64 = run(torch.float32), run(torch.float64)
names = r32["names"]
for k, v in r32["init"].items():
    assert torch.equal(v.double(), r64["init"][k]), k
main = {"init_" + k: v.numpy() for k, v in r32["init"].items()}
main.update(x=x_all, a=a_all, noise=noise_all, keys=np.array(";".join(r32["init"])), param_keys=np.array(";".join(names)))
for tag, r in (("ref32", r32), ("ref64", r64)):
    main["loss_" + tag] = np.array(r["rec"]["loss"], np.float64)
    main["sigma_" + tag] = np.stack(r["rec"]["sigma"])
    main["grad_norm_" + tag] = np.array(r["rec"]["grad_norm"], np.float64)
    main["lr_" + tag] = np.array(r["rec"]["lr"], np.float64)
    main["net_out_" + tag] = r["rec"]["net_out"][0].numpy()


def delta(r, what, k):
    return (r[what][k].detach().double() - r32["init"][k].double()).float().numpy()


grads64 = {"grad_" + k: g.numpy() for k, g in zip(names, r64["rec"]["grads"][0]) if g is not None}      # RFF_freq is frozen
ref32 = {"grad_" + k: g.numpy() for k, g in zip(names, r32["rec"]["grads"][0]) if g is not None}
final64 = {}
for k in names:
    ref32["net32d_" + k] = delta(r32, "net", k)
    main["ema32d_" + k] = delta(r32, "ema", k)
    final64["net64d_" + k], final64["ema64d_" + k] = delta(r64, "net", k), delta(r64, "ema", k)
    for what, r in (("net", r64), ("ema", r64)):       # the stored difference gives the float64 value back far below any bar
        back = r32["init"][k].double() + torch.from_numpy(delta(r, what, k)).double()
        assert float((back - r[what][k].detach()).abs().max()) <= 1e-12 * max(float(r[what][k].abs().max()), 1e-30) + 1e-15, (what, k)

total = 0
for fname, arrays in (("g30_diffusion_train.npz", main), ("g30_diffusion_train_grads64.npz", grads64),
                      ("g30_diffusion_train_ref32.npz", ref32), ("g30_diffusion_train_final64.npz", final64)):
    path = os.path.join(GDIR, fname)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    total += size
    print(f"{path}: {size} bytes, {len(arrays)} arrays")
    assert size < (1 << 20), "a fixture must stay below 1 MiB"
print(f"total {total} bytes; parameters {sum(v.numel() for k, v in r32['net'].items())}")
print("loss32", main["loss_ref32"], "loss64", main["loss_ref64"], "lr", main["lr_ref64"], "norm", main["grad_norm_ref64"])
worst = lambda a, b: float(np.max(np.abs(a.astype(np.float64) - b)) / max(np.max(np.abs(b)), 1e-300))      # noqa: E731
print("E32 loss", worst(main["loss_ref32"], main["loss_ref64"]), "net_out", worst(main["net_out_ref32"], main["net_out_ref64"]))
print("E32 grads, worst over tensors", max(worst(ref32["grad_" + k], grads64["grad_" + k]) for k in names if "grad_" + k in grads64))
print("E32 final net (difference from init, relative to the weights)",
      max(float(np.max(np.abs(ref32["net32d_" + k].astype(np.float64) - final64["net64d_" + k]))) /
          float(r64["net"][k].abs().max()) for k in names))
