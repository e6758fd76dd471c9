#!/usr/bin/env python3
"""tests/golden/mfma2_step_bits.npz: the output BITS of the exact-fp32 matrix-pipe GRU kernel (kernel_variant "mfma2") at the
smallest batches it accepts, recorded from the build that is being replaced before a change that must not move a bit (a
re-ordering of the step's instructions, say).  Needs the MI355X and a built libntm.so.

Inputs: tests/mfma2_step_cases.py (fixed numpy seed).  Per batch size B in SMALL_B the run of T_MAX = 200 steps from the seeded
state is stored (y_<B>, h_<B>); every shorter T of STEP_T is run as well and must reproduce the prefix of that output bit for
bit -- the kernel's step does the same arithmetic in every compile-time copy -- so the one array pins all of them.

Usage:  python tools/make_goldens_mfma2_bits.py [output.npz]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ntm_amd  # noqa: E402
from mfma2_step_cases import SMALL_B, STEP_T, T_MAX, inputs  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "mfma2_step_bits.npz")
m = ntm_amd.harness.build_model(ntm_amd.weights.W_GRU)
m.kernel_variant = "mfma2"
out = {}
for B in SMALL_B:
    for T in sorted(STEP_T, reverse=True):
        x, h0 = inputs(B, T)
        m.hidden = torch.from_numpy(h0).cuda().view(1, B, 64)
        y = m.forward(torch.from_numpy(x).cuda().unsqueeze(1))[:, 0].cpu().numpy()
        if T == T_MAX:
            out[f"y_{B}"], out[f"h_{B}"] = y, m.hidden[0].cpu().numpy()
        assert np.array_equal(y, out[f"y_{B}"][:, :T]), (B, T)
np.savez(out_path, **out)
print(f"{out_path}: {os.path.getsize(out_path)} bytes, " + ", ".join(f"{k} {v.shape}" for k, v in out.items()))
