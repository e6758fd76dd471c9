"""CPU: the host side of the adjoints of the resample + combine steps (ntm_unet_down_combine_backward,
ntm_unet_up_combine_backward under training.DownCombineFn / UpCombineFn): the declarations, every documented refusal (made before
anything touches a device, so they run here with made-up non-null pointers), the HIP-only refusal of the nodes, and the case
module that the GPU tests use -- its numpy adjoints against torch autograd in float64, torch's own float32 autograd against the
derived bound, and the magnitudes of the exact-integer cases."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ntm_amd
from ntm_amd import diffusion, training
import resample_adjoint_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"ntm_unet_down_combine_backward": 15, "ntm_unet_up_combine_backward_partials": 1, "ntm_unet_up_combine_backward": 16}
P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(16)]     # made-up device pointers: a refusal never looks at them


def test_new_symbols_are_declared_bound_and_built():
    L = ntm_amd._lib.lib()
    with open(os.path.join(ROOT, "include", "ntm.h")) as f:
        header = f.read()
    for s, nargs in SYMS.items():
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1] and len(ntm_amd._lib._SIGNATURES[s][1]) == nargs, s
    assert "unet_resample_train.hip" in open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "Makefile")).read()
    assert hasattr(training, "DownCombineFn") and hasattr(training, "UpCombineFn")


def test_constants_mirror_the_kernels():
    with open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "unet_resample_train.hip")) as f:
        src = f.read()
    assert f"constexpr int kRTile = {R.R_TILE};" in src and f"constexpr int kRSeg = {R.R_SEG};" in src
    assert "constexpr int kRStage = kRTile + 64 + 16;" in src and R.R_STAGE == R.R_TILE + 64 + 16
    # what a tile of the down adjoint stages, at the worst S and taps the entry point takes
    assert max((R.R_TILE + taps - 2) // S + 2 for S in range(1, 65) for taps in range(S, R.MAX_TAPS + 1)) <= R.R_STAGE
    L = ntm_amd._lib.lib()
    for Fr in (1, R.R_TILE - 1, R.R_TILE, R.R_TILE + 1, 65536):
        assert L.ntm_unet_up_combine_backward_partials(Fr) == -(-Fr // R.R_TILE)
    assert L.ntm_unet_up_combine_backward_partials(0) == -1
    assert L.ntm_last_error().decode().startswith("ntm_unet_up_combine_backward_partials")


def down(L, pd=P[0], ker=P[1], wc=P[2], g_xo=P[3], g_po=P[4], B=2, C=8, F=100, S=4, width=25, taps=54, g_x=P[5], g_pyr=P[6], part=P[7]):
    return L.ntm_unet_down_combine_backward(pd, ker, wc, g_xo, g_po, B, C, F, S, width, taps, g_x, g_pyr, part, None)


def up(L, x=P[0], ker=P[1], wc=P[2], g_xo=P[3], g_po=P[4], B=2, C=8, F=100, S=4, width=7, taps=15, pyr_T=100, g_x=P[5], g_pyr=P[6],
       part=P[7]):
    return L.ntm_unet_up_combine_backward(x, ker, wc, g_xo, g_po, B, C, F, S, width, taps, pyr_T, g_x, g_pyr, part, None)


DOWN_REFUSED = {"both gradients null": (dict(g_xo=None, g_po=None), "both null"), "taps != 2 w + S": (dict(taps=53), "taps"),
                "C = 33": (dict(C=33), r"C must lie"), "taps = 65": (dict(taps=65, width=30, S=5), "taps"),
                "nothing to write": (dict(g_x=None, g_pyr=None, part=None), "nothing to write"),
                "B too large": (dict(B=65536), "B must lie"), "C F >= 2^31": (dict(C=32, F=1 << 27), "2.31"),
                "no filter": (dict(ker=None), "null pointer"), "no weights": (dict(wc=None), "null pointer"),
                "partials without pyr_d": (dict(pd=None), "null pointer")}
UP_REFUSED = {"both gradients null": (dict(g_xo=None, g_po=None), "both null"), "taps != 2 w + 1": (dict(taps=16), "taps"),
              "S = 1 with a filter": (dict(S=1, g_xo=None), "taps"), "S = 1 with ker": (dict(S=1, width=0, taps=0, g_xo=None), "S == 1"),
              "S = 1 with g_xo": (dict(S=1, width=0, taps=0, ker=None), "S == 1"),
              "pyr_T < F": (dict(pyr_T=99), "shorter than F"), "C = 33": (dict(C=33), r"C must lie"),
              "taps = 65": (dict(taps=65, width=32), "taps"),
              "nothing to write": (dict(g_x=None, g_pyr=None, part=None), "nothing to write"),
              "g_pyr without a pyramid": (dict(pyr_T=0), "g_pyr without"), "S F >= 2^31": (dict(F=1 << 29), "2.31"),
              "no filter": (dict(ker=None), "null pointer"), "no weights": (dict(wc=None), "null pointer"),
              "partials without x": (dict(x=None), "null pointer")}


@pytest.mark.parametrize("why", sorted(DOWN_REFUSED))
def test_down_backward_refuses_before_the_device(why):
    L = ntm_amd._lib.lib()
    kw, msg = DOWN_REFUSED[why]
    assert down(L, **kw) == -1, why
    assert re.match("ntm_unet_down_combine_backward: .*" + msg, L.ntm_last_error().decode()), (why, L.ntm_last_error().decode())


@pytest.mark.parametrize("why", sorted(UP_REFUSED))
def test_up_backward_refuses_before_the_device(why):
    L = ntm_amd._lib.lib()
    kw, msg = UP_REFUSED[why]
    assert up(L, **kw) == -1, why
    assert re.match("ntm_unet_up_combine_backward: .*" + msg, L.ntm_last_error().decode()), (why, L.ntm_last_error().decode())


def test_an_empty_batch_is_accepted_and_touches_nothing():
    L = ntm_amd._lib.lib()
    none = dict(ker=None, wc=None, g_xo=None, g_po=None, g_x=None, g_pyr=None, part=None)
    assert down(L, pd=None, B=0, **none) == 0 and up(L, x=None, B=0, pyr_T=0, **none) == 0


def test_no_cpu_fallback():
    case = R.CASES["down S=4 F=17 C=5 pyr=0"]
    op, w = R.operands(case)
    with pytest.raises(RuntimeError, match="DownCombineFn: HIP device only"):
        training.DownCombineFn.apply(op["x"].requires_grad_(), op["pyr"], op["ker"], op["wc"], 4, w)
    case = R.CASES["up S=4 F=3 C=5 pyr=0"]
    op, w = R.operands(case)
    with pytest.raises(RuntimeError, match="UpCombineFn: HIP device only"):
        training.UpCombineFn.apply(op["x"].requires_grad_(), op["pyr"], op["ker"], op["wc"], 4, w)
    with pytest.raises(RuntimeError, match="up_combine: HIP device only"):
        diffusion.up_combine(op["x"], op["pyr"], op["ker"], op["wc"], 4, w)


def test_the_table_holds_what_it_says():
    names = list(R.CASES)
    for kind, Ss in (("down", (2, 3, 4)), ("up", (1, 2, 3, 4))):
        for S in Ss:
            fs = {c["F"] for c in R.CASES.values() if c["kind"] == kind and c["S"] == S}
            taps = R.taps_of(kind, S)
            assert {1, 2, S + 1, 4 * S - 1, 4 * S + 1, taps + 1, 1000, R.R_TILE - 1, R.R_TILE, R.R_TILE + 1, R.R_SEG - 1,
                    R.R_SEG + 1} <= fs, (kind, S)
            assert taps <= R.MAX_TAPS
            cs = {c["C"] for c in R.CASES.values() if c["kind"] == kind and c["S"] == S}
            assert cs == {1, 5, 16}
            if kind == "up":
                assert {c["extra"] for c in R.CASES.values() if c["kind"] == kind and c["S"] == S} == {None, 0, 3}
    assert len(names) == len(set(names)) and all(c["C"] <= R.MAX_C for c in R.CASES.values())


def rel(a, b):
    m = float(np.max(np.abs(b))) if b.size else 0.0
    if m == 0:
        return 0.0 if not np.any(a) else float("inf")
    return float(np.max(np.abs(a - b))) / m


@pytest.mark.parametrize("kind", ["down", "up"])
def test_numpy_adjoints_equal_float64_autograd_and_float32_autograd_holds_the_bound(kind):
    worst_rel, worst = 0.0, {}
    for name, case in R.CASES.items():
        if case["kind"] != kind:
            continue
        op, w = R.operands(case)
        N = R.n_roundings(kind, case["S"], case["C"])
        for grads in R.variants(case):
            ref, A = R.reference(name, grads)
            mine = R.numpy_step(case, op, w, grads)
            t32 = R.torch_step(case, op, w, torch.float32, grads)
            for k in ("g_x", "g_pyr", "g_wc"):
                if ref[k] is None:
                    assert mine[k] is None, (name, k)
                    continue
                assert mine[k].shape == ref[k].shape, (name, grads, k)
                e = rel(mine[k], ref[k])
                worst_rel = max(worst_rel, e)
                assert e <= 1e-12, (name, grads, k, e)
                fr = R.fraction(t32[k], ref[k], A[k], N)
                worst[k] = max(worst.get(k, 0.0), fr)
                assert fr <= 1.0, (name, grads, k, fr)
    print(f"{kind}: numpy adjoints vs float64 autograd, worst relative distance {worst_rel:.2e}; torch float32 autograd, worst "
          f"fraction of the bound per output: {({k: round(v, 4) for k, v in worst.items()})}")


def test_exact_integer_cases_stay_exact():
    """Every absolute sum of the exact cases stays below 2^24 (float32 holds it) -- the fp64 partials below 2^53."""
    for name, case in R.EXACT.items():
        op, w = R.integer_operands(case)
        ab = {k: None if v is None else v.abs() for k, v in op.items()}
        grads = "po" if case["kind"] == "down" else "both"
        got = R.numpy_step(case, ab, w, grads, dtype=np.int64)
        keys = ("g_pyr",) if case["kind"] == "down" else ("g_x", "g_wc")
        for k in keys:
            assert got[k].dtype == np.int64 and 0 < got[k].max() < 2 ** 24 < 2 ** 53, (name, k, got[k].max())
        # and the int64 gather is the float64 reference of the same operands
        ref = R.torch_step(case, op, w, torch.float64, grads)
        mine = R.numpy_step(case, op, w, grads, dtype=np.int64)
        for k in keys:
            assert np.array_equal(mine[k].astype(np.float64), ref[k].numpy()), (name, k)
