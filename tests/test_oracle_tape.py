"""CPU side of the tape-kernel tests (tests/test_gpu_tape.py): the high-precision fixture golden g25
(tools/make_goldens_tape_mp.py, mpmath at 50 digits) is what its generator produces, its conditions hold (selector
exclusions of the ja_f points, clamped shares of the trajectory families), the case tables of the GPU tests contain
the edges they claim, and the oracle's resampler and FIR -- parity unpinned, torchaudio being absent -- are pinned to a
numpy.longdouble evaluation of the formulas in include/ntm.h at the shapes the GPU tests use."""
import importlib.util
import math
import os

import numpy as np
import pytest

import oracle
from helpers import (FIR_TAPS, RECORD_BIG, RECORD_GRID_LIMIT, RECORD_SHAPES, RESAMPLE_RATIOS, ROOT, TAPE_CUT_N, TAPE_HMAG_B,
                     TAPE_HMAG_N, TAPE_SINGLE_STREAMS, TAPE_TILE, U53, fir_case, fir_lengths, fir_ref_ld, load, resample_input,
                     resample_lengths, resample_out_lengths, resample_ref_ld, tape_cut_lists, tape_walk)

_spec = importlib.util.spec_from_file_location("make_goldens_tape_mp", os.path.join(ROOT, "tools", "make_goldens_tape_mp.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def g():
    return load("g25_tape_mp.npz")


def test_fixture_settings_and_inputs_are_the_generators(g):
    assert int(g["dps"]) == gen.DPS >= 40 and int(g["seed"]) == gen.SEED and float(g["Ts"]) == gen.TS == 1.0 / (48000 * 16)
    assert tuple(g["params"]) == gen.PARAMS == oracle.TAPE_PARAMS
    assert tuple(g["families"]) == gen.FAMILIES and tuple(g["ja_classes"]) == gen.JA_CLASSES and tuple(g["helpers"]) == gen.HELPERS
    # inputs that go through libm's sin / exp / log may differ in the last place between machines; the rest is exact
    for name, x in gen.helper_points().items():
        assert x.shape == g[f"h_{name}_x"].shape and np.allclose(x, g[f"h_{name}_x"], rtol=4 * 2.0 ** -52, atol=0), name
    for name, H in gen.family_inputs().items():
        assert H.shape == (gen.TRAJ_B, gen.TRAJ_N) == g[f"t_{name}_H"].shape
        assert np.allclose(H, g[f"t_{name}_H"], rtol=0, atol=8 * 2.0 ** -52 * np.abs(H).max()), name
    for name in ("walk_small", "step", "const", "zeros"):
        assert np.array_equal(gen.family_inputs()[name], g[f"t_{name}_H"]), name


def test_fixture_equals_a_regenerated_subset(g):
    """mpmath again, from the STORED inputs: every 16th helper point, two ja_f classes point by point, one stream of
    three families -- equality, not a tolerance."""
    pytest.importorskip("mpmath")
    for name in gen.HELPERS:
        x, y = g[f"h_{name}_x"][::16], g[f"h_{name}_y"][::16]
        assert np.array_equal(gen.mp_helper(name, x), y), name
    pts, f, sel = g["ja_pts"][::9], g["ja_f"][::9], g["ja_sel"][::9]
    for p, fv, s in zip(pts.tolist(), f, sel):
        got, gs, ok = gen.mp_ja_f(*p, detail=True)
        assert float(got) == fv and tuple(gs) == tuple(s) and ok, p
    for name, b in (("sin100", 2), ("walk_small", 1), ("chain", 3), ("sat", 0)):
        M, st = gen.mp_hmag(g[f"t_{name}_H"][b:b + 1])
        assert np.array_equal(M[0], g[f"t_{name}_M"][b]), name
        assert np.array_equal(st[gen.TRAJ_MID][0], g[f"t_{name}_state{gen.TRAJ_MID}"][b]), name
        assert np.array_equal(st[gen.TRAJ_N][0], g[f"t_{name}_state{gen.TRAJ_N}"][b]), name


def test_helper_points_cover_the_ranges_and_edges(g):
    up, dn = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    x = g["h_expm1_neg_x"]
    assert len(x) >= 2000 and x.max() == -2e-4 and (x < 0).all() and -800.0 in x and -1e4 in x and -1e7 in x
    assert g["h_expm1_neg_y"][x == -1e4] == -1.0 and g["h_expm1_neg_y"][x == -1e7] == -1.0
    for k in (1, 2, 3, 40):
        h = k * math.log(2.0) / 2
        assert {-h, -up(h), -dn(h)} <= set(x.tolist()), k
    x = g["h_coth_gt_x"]
    assert len(x) >= 2000 and np.abs(x).min() == up(1e-4) and np.abs(x).max() == 50.0 and (x > 0).any() and (x < 0).any()
    x = g["h_langevin_prime_lt1_x"]
    assert len(x) >= 2000 and np.abs(x).min() == up(1e-4) and 0.999999 in x and -0.999999 in x and np.abs(x).max() < 1
    assert set(gen.lp_bin(x).tolist()) == set(range(len(gen.LP_BINS) - 1)) and g["h_langevin_prime_lt1_eref"].shape == (5,)
    x = g["h_rcp_nr_x"]
    assert len(x) >= 2000 and np.abs(x).min() == 1e-100 and np.abs(x).max() == 1e100 and (x < 0).any()
    for p in (2.0 ** -330, 1.0, 2.0 ** 330):
        assert {p, up(p), dn(p), -p, -up(p), -dn(p)} <= set(x.tolist()), p
    # E_ref of the library functions, recomputed here (another libm may differ in the last place: factor 2)
    for name in gen.HELPERS:
        e = gen.rel_err(gen.lib_helper(name, g[f"h_{name}_x"]), g[f"h_{name}_y"])
        if name == "langevin_prime_lt1":
            b = gen.lp_bin(g[f"h_{name}_x"])
            e = np.array([e[b == k].max() for k in range(5)])
        else:
            e = np.array([e.max()])
        assert (e <= 2 * np.maximum(g[f"h_{name}_eref"], 2.0 ** -52)).all(), (name, e, g[f"h_{name}_eref"])


def test_ja_f_points_cover_the_switches_and_the_oracle_keeps_the_exclusion_cap(g):
    pts, cls, sel, keep = g["ja_pts"], g["ja_class"], g["ja_sel"], g["ja_keep"].astype(bool)
    Ms, A, alpha, _, _ = gen.PARAMS
    ours = gen.fp64_selectors(pts)
    assert np.array_equal((ours == sel).all(axis=1), keep)
    assert (~keep).mean() <= 0.01, (~keep).mean()                       # the cap, for the oracle's arithmetic alone
    Q = np.abs((pts[:, 1] + alpha * pts[:, 0]) / A)
    for v in (0, 1):                                                   # both sides of both switches, both signs
        assert (sel[keep, 0] == v).sum() >= 100 and (sel[keep, 1] == v).sum() >= 100
        assert ((sel[keep, 0] == 1) & (sel[keep, 1] == v)).sum() >= 100
    assert {-1, 1} <= set(sel[keep, 2].tolist()) and {-1, 1} <= set(sel[keep, 3].tolist())
    assert Q.max() > 5e3 and Q[Q > 0].min() < 1e-7
    names = list(gen.JA_CLASSES)
    hz, org = cls == names.index("hp_zero"), cls == names.index("origin")
    assert hz.sum() >= 100 and (pts[hz, 2] == 0).all() and (g["ja_f"][hz] == 0).all()
    assert org.sum() >= 100 and (pts[org, :2] == 0).all() and (sel[org, 2] == 0).all() and (g["ja_f"][org] != 0).all()
    assert np.isfinite(g["ja_f"]).all()
    # the oracle is the generator's plain-fp64 restatement bit for bit (the generator may not import the oracle), so its
    # error per class is what the fixture records (factor 2 for another libm)
    fo = oracle.tape_ja_f(pts)
    assert np.array_equal(fo, np.array([gen.fp64_ja_f(*p) for p in pts.tolist()]))
    e = gen.rel_err(fo, g["ja_f"])
    for k, name in enumerate(names):
        got = e[(cls == k) & keep].max()
        assert got <= 2 * max(g["ja_eref"][k], 2.0 ** -52), (name, got, g["ja_eref"][k])


def test_trajectory_families_clamped_shares_and_oracle_error(g):
    Ms = gen.PARAMS[0]
    for name in gen.FAMILIES:
        M, share = g[f"t_{name}_M"], g[f"t_{name}_clamped"]
        assert M.shape == (4, 300) and np.abs(M).max() <= Ms
        assert tuple(share) == gen.clamped_share(M), name
        if name in gen.UNSATURATED:
            assert tuple(share) == (0.0, 0.0) and np.abs(M).max() < Ms, name
        Mo, so = oracle.tape_hmag(g[f"t_{name}_H"], None, gen.TS, gen.PARAMS)
        if name in ("walk_small", "chain"):
            assert np.array_equal(Mo[:2], gen.fp64_hmag(g[f"t_{name}_H"][:2])), name
        e = np.abs(Mo - M).max()
        assert e <= 2 * float(g[f"t_{name}_eref"]) + 2.0 ** -52 * np.abs(M).max(), (name, e)
    assert len(gen.UNSATURATED) == 4
    assert g["t_sat_clamped"][0] > 0.1 and g["t_sat_clamped"][1] > 0.1          # both rails
    assert not g["t_zeros_M"].any() and not g["t_zeros_state300"].any()
    assert g["g9_walk_clamped"].sum() > 0.9                                      # why g9's walk says little
    # the state rows are those of the trajectory: M_prev = M[:, n-1], H_prev = H[:, n-1]
    for name in gen.FAMILIES:
        for n in (gen.TRAJ_MID, gen.TRAJ_N):
            st = g[f"t_{name}_state{n}"]
            assert np.array_equal(st[:, 0], g[f"t_{name}_M"][:, n - 1]) and np.array_equal(st[:, 1], g[f"t_{name}_H"][:, n - 1])


def test_gpu_case_tables_contain_their_edges():
    T = TAPE_TILE
    assert {1, T - 1, T, T + 1, 2 * T + 1} <= set(TAPE_HMAG_B) and {1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 1} <= set(TAPE_HMAG_N)
    assert set(TAPE_SINGLE_STREAMS) == {0, T - 1, T, 2 * T} and max(TAPE_SINGLE_STREAMS) < max(TAPE_HMAG_B)
    assert 67 in TAPE_CUT_N and any(n > 2 * T + 1 for n in TAPE_CUT_N)
    assert (1,) * 67 in tape_cut_lists(67)
    big = [c for n in TAPE_CUT_N for c in tape_cut_lists(n)]
    for first in (1, T - 1, T, T + 1):
        assert any(c[0] == first for c in big), first
    assert any(len(c) == 3 and c[:2] == (T, T) for c in big)
    # the inputs of the shape grid never reach the clamp (the GPU test compares unsaturated samples)
    H = tape_walk(0, max(TAPE_HMAG_B), max(TAPE_HMAG_N))
    Mo, _ = oracle.tape_hmag(H)
    assert np.abs(Mo).max() < gen.PARAMS[0]
    assert set(RESAMPLE_RATIOS) == {(1, 16), (16, 1), (147, 160), (160, 147), (2, 3), (3, 2)}
    from ntm_amd.tape import sinc_resample_kernel
    for orig, new in RESAMPLE_RATIOS:
        _, width, down, up = sinc_resample_kernel(orig, new)
        assert (down, up) == (orig, new)
        Ns = resample_lengths(width)
        assert {1, 2, width - 1, width, width + 1, 255, 256, 257, 1000} == set(Ns) and min(Ns) >= 1
        for N in Ns:
            full = math.ceil(up * N / down)
            Ms_ = resample_out_lengths(N, up, down)
            assert full in Ms_ and 1 in Ms_ and max(Ms_) > full and (full <= 2 or any(1 <= m < full for m in Ms_))
            assert 3 * max(Ms_) < 300000
    assert set(FIR_TAPS) == {1, 2, 127, 128, 129}
    for taps in FIR_TAPS:
        Ns = fir_lengths(taps)
        assert {1, taps, taps + 1, 255, 256, 257, 700} <= set(Ns) and (taps == 1 or taps - 1 in Ns) and min(Ns) >= 1
        x, h = fir_case(taps, 700)
        y, _ = fir_ref_ld(x, h)
        y = y.astype(np.float64)
        assert (y == 1.0).any() and (y == -1.0).any() and (np.abs(y) == 1.0 - U53).any() and (np.abs(y) > 2).any()
    assert set(RECORD_SHAPES) == {(1, 1), (3, 255), (2, 257)}
    B, N = RECORD_BIG
    assert B == 3 and B * N > RECORD_GRID_LIMIT >= B * (N - 1)


# ------------------------------------------------------------------------- the oracle's resampler and FIR, pinned
@pytest.mark.parametrize("orig,new", RESAMPLE_RATIOS)
def test_sinc_resample_oracle_equals_the_header_formula_in_longdouble(orig, new):
    """oracle.sinc_resample (its own kernel values from math.sin / cos, products and sums rounded one by one, phase by
    phase) against include/ntm.h's formula in longdouble on the product's kernel table.  Bound per sample: two
    roundings per tap plus a table entry that may differ by a few units in the last place (sin, cos^2, two products),
    (2 taps + 8) 2^-53 sum |ker| |x|."""
    from ntm_amd.tape import sinc_resample_kernel
    ker, width, down, up = sinc_resample_kernel(orig, new)
    taps = 2 * width + down
    for N in resample_lengths(width):
        x = resample_input(N, 3, N)
        M = math.ceil(up * N / down)
        got = oracle.sinc_resample(x, orig, new)
        want, s = resample_ref_ld(x, ker, width, up, down, M)
        assert got.shape == (3, M)
        assert (np.abs(got - want).astype(np.float64) <= (2 * taps + 8) * U53 * s).all(), (N, np.abs(got - want).max())


@pytest.mark.parametrize("taps", FIR_TAPS)
def test_fir_clamp_oracle_equals_the_header_formula_in_longdouble(taps):
    """oracle.fir_clamp (numpy.convolve, then clip) against the causal sum of include/ntm.h in longdouble: two roundings
    per tap, 2 taps 2^-53 sum |h| |x|; clamped, it is the clip of the same."""
    for N in fir_lengths(taps):
        x, h = fir_case(taps, N)
        want, s = fir_ref_ld(x, h)
        got = oracle.fir_clamp(x, h, clamp=False)
        assert (np.abs(got - want).astype(np.float64) <= 2 * taps * U53 * s).all(), N
        assert np.array_equal(oracle.fir_clamp(x, h, clamp=True), np.clip(got, -1.0, 1.0))
