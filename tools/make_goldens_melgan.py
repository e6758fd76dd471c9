#!/usr/bin/env python3
"""Golden g27: the reference's own `MelGCrit` (code/critics.py:18-122) on the CPU -- what a seeded construction builds and where
it leaves the generator, and one forward / backward of a small instance through EVERY layer's output.

Dev-only script: it imports the reference's `critics` module at run time from a checkout given on the command line (with empty
stand-ins for torchaudio / soundfile / librosa, which that module imports and this class never uses) and never travels.  It
writes tests/golden/g27_melgan_crit.npz:
  small instance  torch.manual_seed(0); MelGCrit(num_D=2, ndf=8, n_layers=2, downsampling_factor=1)   (3188 parameters)
      sd_<key>         the state_dict
      skeys            its keys in order (';' between them)
      after            torch.rand(3) drawn right after construction
      printed          what the constructor printed (nothing)
      x                (3, 1, 40) fp32 input; out_<d>_<l> = layer l's output of discriminator d (2 x 5)
      gx, g_<key>      the gradients of sum_disc -scale[-1].mean()
  configuration 0  torch.manual_seed(0); MelGCrit(num_D=3, ndf=16, n_layers=4, downsampling_factor=4)
      keys, shapes     the state_dict keys in order and their shapes (as a string, ';' between keys)
      n_params         16 924 086
      c0_after         torch.rand(3) drawn right after construction
      c0_<key>         the tensors of layer_0 and layer_6 of disc_0 and disc_2

Usage:  python tools/make_goldens_melgan.py <reference checkout>
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("NTM_REFERENCE", "")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
if not os.path.isfile(os.path.join(REF, "code", "critics.py")):
    sys.exit(__doc__)

for m in ["torchaudio", "soundfile", "librosa", "librosa.filters"]:
    sys.modules[m] = types.ModuleType(m)
sys.modules["librosa.filters"].mel = lambda *a, **k: None
sys.modules["librosa"].filters = sys.modules["librosa.filters"]
sys.path.insert(0, os.path.join(REF, "code"))

import torch  # noqa: E402
import critics as refcritics  # noqa: E402  (the reference's code/critics.py)

torch.set_num_threads(4)
out = {}

torch.manual_seed(0)
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    D = refcritics.MelGCrit(num_D=2, ndf=8, n_layers=2, downsampling_factor=1)
out["after"] = torch.rand(3).numpy()
out["printed"] = np.array(buf.getvalue())
sd = D.state_dict()
out["skeys"] = np.array(";".join(sd))
for k, v in sd.items():
    out["sd_" + k] = v.numpy().copy()
assert sum(p.numel() for p in D.parameters()) == 3188
x = torch.from_numpy(np.random.default_rng(27).uniform(-1.0, 1.0, (3, 1, 40)).astype(np.float32)).requires_grad_(True)
res = D(x)
loss = 0
for scale in res:
    loss += -scale[-1].mean()
loss.backward()
out["x"], out["gx"] = x.detach().numpy(), x.grad.numpy()
for d, scale in enumerate(res):
    assert len(scale) == 5
    for l, t in enumerate(scale):
        out[f"out_{d}_{l}"] = t.detach().numpy().copy()
for k, p in D.named_parameters():
    out["g_" + k] = p.grad.numpy().copy()

torch.manual_seed(0)
D = refcritics.MelGCrit(num_D=3, ndf=16, n_layers=4, downsampling_factor=4)
out["c0_after"] = torch.rand(3).numpy()
sd = D.state_dict()
out["keys"] = np.array(";".join(sd))
out["shapes"] = np.array(";".join(",".join(str(n) for n in v.shape) for v in sd.values()))
out["n_params"] = np.array(sum(p.numel() for p in D.parameters()))
for k, v in sd.items():
    if k.startswith(("model.disc_0.model.layer_0.", "model.disc_0.model.layer_6.", "model.disc_2.model.layer_0.",
                     "model.disc_2.model.layer_6.")):
        out["c0_" + k] = v.numpy().copy()

path = os.path.join(GDIR, "g27_melgan_crit.npz")
np.savez_compressed(path, **out)
print(f"{path}: {os.path.getsize(path)} bytes, {int(out['n_params'])} parameters, printed {buf.getvalue()!r}")
