"""CPU: the host side of the STFT-sums adjoint (ntm_stft_grad) and of MRSTFTLoss as a graph node -- symbols, argument checks
(they run before anything touches a device), refusals, and the build-time DPP check of the source that holds the new kernels."""
import os
import re
import subprocess
import sys

import pytest
import torch

import ntm_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ntm_stft_grad_workspace_floats", "ntm_stft_grad")


def test_entry_points_are_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    for s in SYMS:
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
    assert re.search(r"#define\s+NTM_ABI_VERSION\s+9\b", header)
    L = ntm_amd._lib.lib()
    assert L.ntm_abi_version() == 9
    for s in SYMS:
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1]
    assert len(ntm_amd._lib._SIGNATURES["ntm_stft_grad"][1]) == 14


def test_workspace_size_and_host_side_refusals():
    L = ntm_amd._lib.lib()
    assert L.ntm_stft_grad_workspace_floats(32, 2048, 0, 1024, 120) == 32 * (1 + 2048 // 120) * 1024
    assert L.ntm_stft_grad_workspace_floats(3, 1100, 37, 512, 50) == 3 * (1 + 1063 // 50) * 512
    assert L.ntm_stft_grad_workspace_floats(0, 10, 0, 512, 50) == 0
    for args in ((1, 256, 0, 512, 50), (1, 1024, 0, 2048, 240), (1, 600, 0, 500, 50), (1, 600, 0, 512, 0), (-1, 600, 0, 512, 50),
                 (1, 600, 601, 512, 50)):
        assert L.ntm_stft_grad_workspace_floats(*args) == -1, args

    def call(B=1, T=600, skip=0, n_fft=512, hop=50, win=240, eps=1e-8):
        return L.ntm_stft_grad(None, None, B, T, skip, n_fft, hop, win, eps, None, None, None, 0, None)

    for kw in ({}, dict(n_fft=100), dict(n_fft=4096), dict(hop=0), dict(win=0), dict(win=513), dict(T=256), dict(skip=344), dict(eps=0.0),
               dict(B=-1), dict(skip=-1)):
        assert call(**kw) == -1, kw                                       # ({}: null pointers)
        assert L.ntm_last_error().decode().startswith("ntm_stft_grad:"), (kw, L.ntm_last_error())
    assert call(B=0) == 0                                                 # B == 0: NTM_OK without looking at the pointers


def test_stft_kernels_run_dpp_with_full_exec():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_exec.py"),
                        os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "stft_kernels.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_a_target_that_requires_grad_is_refused():
    y = torch.zeros(2, 1, 2048, requires_grad=True)
    t = torch.zeros(2, 1, 2048, requires_grad=True)
    for call in (ntm_amd.MRSTFTLoss(), ntm_amd.MRSTFTLoss().per_segment):
        with pytest.raises(RuntimeError, match="target must not require grad"):
            call(y, t)


@pytest.mark.parametrize("requires_grad", [False, True])
def test_a_cpu_tensor_is_refused_as_esrloss_refuses_it(requires_grad):
    y = torch.zeros(2, 1, 2048, requires_grad=requires_grad)
    t = torch.zeros(2, 1, 2048)
    with pytest.raises(Exception) as want:
        ntm_amd.ESRLoss()(y, t)
    for call in (ntm_amd.MRSTFTLoss(), ntm_amd.MRSTFTLoss().per_segment):
        with pytest.raises(type(want.value), match="HIP device"):
            call(y, t)
    assert "HIP device" in str(want.value)
