#!/usr/bin/env python3
"""Golden g26: the reference's own `DilatedConvDisc` (code/critics.py:262-331) on the CPU -- what a seeded construction builds
and where it leaves the generator, and one forward / backward of a small instance.

Dev-only script: it imports the reference's `critics` module at run time from a checkout given on the command line (with empty
stand-ins for torchaudio / soundfile / librosa, which that module imports and this class never uses) and never travels.  It
writes tests/golden/g26_dilated_disc.npz:
  small instance  torch.manual_seed(0); DilatedConvDisc(layers=4, conv_channels=8, test_in_len=100)
      sd_<key>         the state_dict
      after            torch.rand(3) drawn right after construction
      x                (3, 1, 100) fp32 input, out = D(x), gx and g_<key> = the gradients of -D(x).mean()
  default instance  torch.manual_seed(0); DilatedConvDisc(test_in_len=8263)
      line             what the constructor printed
      keys, shapes     the state_dict keys in order and their shapes (as a string, ';' between keys)
      first_<name>, last_<name>   the tensors of layers.0 and layers.22

Usage:  python tools/make_goldens_dilated_disc.py <reference checkout>
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
with contextlib.redirect_stdout(io.StringIO()):
    D = refcritics.DilatedConvDisc(layers=4, conv_channels=8, test_in_len=100)
out["after"] = torch.rand(3).numpy()
for k, v in D.state_dict().items():
    out["sd_" + k] = v.numpy().copy()
x = torch.from_numpy(np.random.default_rng(26).uniform(-1.0, 1.0, (3, 1, 100)).astype(np.float32)).requires_grad_(True)
y = D(x)
(-y.mean()).backward()
out["x"], out["out"], out["gx"] = x.detach().numpy(), y.detach().numpy(), x.grad.numpy()
for k, p in D.named_parameters():
    out["g_" + k] = p.grad.numpy().copy()

torch.manual_seed(0)
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    D = refcritics.DilatedConvDisc(test_in_len=8263)
sd = D.state_dict()
out["line"] = np.array(buf.getvalue())
out["keys"] = np.array(";".join(sd))
out["shapes"] = np.array(";".join(",".join(str(n) for n in v.shape) for v in sd.values()))
for name in ("bias", "weight_g", "weight_v"):
    out["first_" + name] = sd[f"layers.0.{name}"].numpy().copy()
    out["last_" + name] = sd[f"layers.22.{name}"].numpy().copy()

path = os.path.join(GDIR, "g26_dilated_disc.npz")
np.savez_compressed(path, **out)
print(f"{path}: {os.path.getsize(path)} bytes, line {buf.getvalue()!r}")
