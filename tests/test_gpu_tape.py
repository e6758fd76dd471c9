"""The device side of ntm_amd.Tape (tape_kernels.hip: ntm_tape_hmag, ntm_tape_record_field, ntm_resample_fir,
ntm_fir_f64) at the shapes, cuts and edges where such kernels go wrong, against references of higher precision.

tape_hmag_kernel replaces the library's tanh and division by hand-written fp64 helpers (csrc/tape_math.h); golden g9's
inputs are clamped to +-Ms almost everywhere, where any error of the helpers disappears, and the fp64 oracle is itself
up to 5e-10 of max|M| off on unsaturated input (it follows the reference's ill-conditioned closed form of L').  So the
helpers (reached through libntm_lab.so's elementwise probe), ja_f and whole trajectories are measured against mpmath
at 50 digits (golden g25, tools/make_goldens_tape_mp.py; pinned on the CPU by tests/test_oracle_tape.py):

    E_gpu <= max(4 E_ref, floor)

E_ref: the error of the library function / of the oracle on the same points; 4: the margin of the spectral tests;
floor: 2^-50 relative for a helper and for ja_f (four units in the last place for a result assembled from at most three
rounded operations on well-conditioned operands), N 2^-53 max|M_ref| for a trajectory of N samples (one rounding of a
value of that size per sample).  Measured figures: DESIGN.md, "Tape kernels: accuracy against mpmath".
Shapes, chunking and state are bit for bit; the resampler and the FIR are held to the bound of a chain of fused
multiply-adds against include/ntm.h's formulas in longdouble."""
import ctypes
import math

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import oracle
from helpers import (FIR_TAPS, RECORD_BIG, RECORD_SHAPES, RESAMPLE_RATIOS, TAPE_CUT_N, TAPE_HMAG_B, TAPE_HMAG_N, TAPE_SINGLE_STREAMS,
                     U53, fir_case, fir_lengths, fir_ref_ld, load, resample_input, resample_lengths, resample_out_lengths,
                     resample_ref_ld, tape_cut_lists, tape_walk)

pytestmark = pytest.mark.gpu
SET = dict(deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
FLOOR_REL = 2.0 ** -50
MARGIN = 4.0
PAR = oracle.TAPE_PARAMS
TS = 1.0 / (48000 * 16)
EINVAL = -1


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available()
    return ntm_amd


@pytest.fixture(scope="module")
def g():
    return load("g25_tape_mp.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def rel_err(got, want):
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(got - want) / np.abs(want)
    return np.where(got == want, 0.0, np.where(want == 0, np.inf, e))


def _par():
    return (ctypes.c_double * 5)(*PAR)


def probe(ntm, name, x):
    """libntm_lab.so's elementwise probe of csrc/tape_math.h -> numpy."""
    L = ntm._lib
    xd = dev(x)
    n = xd.numel() // (3 if name == "ja_f" else 1)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    rc = L.lab().ntm_lab_tape_math(L.LAB_TAPE_OPS[name], L.ptr(xd), L.ptr(out), n, _par(), L.current_stream())
    L.check(rc, "ntm_lab_tape_math", L.lab().ntm_lab_last_error)
    return out.cpu().numpy()


def hmag(ntm, H, state=None):
    """ntm_tape_hmag through the raw ABI: H torch (B, N) on the device -> (M, state) torch; `state` is not modified."""
    L = ntm._lib
    B, N = H.shape
    state = torch.zeros(B, 3, dtype=torch.float64, device="cuda") if state is None else state.clone()
    M = torch.full((B, N), float("nan"), dtype=torch.float64, device="cuda")
    H = H.contiguous()
    L.check(L.lib().ntm_tape_hmag(L.ptr(H), L.ptr(M), B, N, L.ptr(state), TS, _par(), L.current_stream()), "ntm_tape_hmag")
    return M, state


def hmag_cuts(ntm, H, cuts, state=None):
    outs, n0 = [], 0
    for c in cuts:
        M, state = hmag(ntm, H[:, n0:n0 + c], state)
        outs.append(M)
        n0 += c
    assert n0 == H.shape[1]
    return torch.cat(outs, 1), state


# ------------------------------------------------------------------------------------------ accuracy against mpmath
@pytest.mark.parametrize("name", ["rcp_nr", "expm1_neg", "coth_gt", "langevin_prime_lt1"])
def test_helper_against_mpmath(ntm, g, name):
    """One helper over its argument range and edges.  langevin_prime_lt1 is judged per bin of |x| (the closed form it
    replaces loses 1e-8 at 1e-4 and nothing at 1: one bar over the whole range would say nothing near 1)."""
    x, want, eref = g[f"h_{name}_x"], g[f"h_{name}_y"], g[f"h_{name}_eref"]
    got = probe(ntm, name, x)
    e = rel_err(got, want)
    bins = np.zeros(len(x), int)
    if name == "langevin_prime_lt1":
        bins = np.searchsorted(g["lp_bins"], np.abs(x), side="left") - 1
    bad = []
    for k in range(len(eref)):
        eg = float(e[bins == k].max())
        bar = max(MARGIN * float(eref[k]), FLOOR_REL)
        print(f"{name}[{k}]: E_ref {float(eref[k]):.3e}  E_gpu {eg:.3e}  bar {bar:.3e}  at x = {x[bins == k][e[bins == k].argmax()]!r}")
        if not eg <= bar:
            bad.append((k, eg, bar))
    assert np.isfinite(got).all() and not bad, bad
    if name == "expm1_neg":
        assert (got[x <= -1e4] == -1.0).all() and (got < 0).all() and (got >= -1.0).all()


def test_ja_f_against_mpmath(ntm, g):
    """The right-hand side of the hysteresis ODE, class by class of |Q| (both sides of the two 1e-4 switches, up to
    1e4), with the exact cases: Hp = 0 gives 0, and Mn = Hn = 0 takes the sgn(M_diff) = 0 path."""
    pts, cls, want, keep = g["ja_pts"], g["ja_class"], g["ja_f"], g["ja_keep"].astype(bool)
    got = probe(ntm, "ja_f", pts)
    e = rel_err(got, want)
    bad = []
    for k, name in enumerate(g["ja_classes"]):
        m = (cls == k) & keep
        eg, eref = float(e[m].max()), float(g["ja_eref"][k])
        bar = max(MARGIN * eref, FLOOR_REL)
        print(f"ja_f {name}: E_ref {eref:.3e}  E_gpu {eg:.3e}  bar {bar:.3e}")
        if not eg <= bar:
            bad.append((str(name), eg, bar))
    assert np.isfinite(got).all() and not bad, bad
    assert (got[pts[:, 2] == 0] == 0).all()


def test_trajectory_families_against_mpmath(ntm, g):
    """4 streams x 300 samples per family from zero state: M and the final state's M_prev within the family's bar;
    H_prev is the last input exactly; all zeros give exactly 0; the saturating family sits on the rails where mpmath
    does."""
    bad = []
    for name in g["families"]:
        H, want, eref = g[f"t_{name}_H"], g[f"t_{name}_M"], float(g[f"t_{name}_eref"])
        M, state = hmag(ntm, dev(H))
        M, state = M.cpu().numpy(), state.cpu().numpy()
        mx = float(np.abs(want).max())
        eg, bar = float(np.abs(M - want).max()), max(MARGIN * eref, H.shape[1] * U53 * mx)
        print(f"{name}: max|M| {mx:.4g}  E_ref {eref:.3e}  E_gpu {eg:.3e}  bar {bar:.3e}  (of max|M|: "
              f"{eref / mx if mx else 0:.2e} / {eg / mx if mx else 0:.2e})  clamped {tuple(g[f't_{name}_clamped'])}")
        if not (np.isfinite(M).all() and eg <= bar):
            bad.append((str(name), eg, bar))
        assert np.array_equal(state[:, 0], M[:, -1]) and np.array_equal(state[:, 1], H[:, -1]), name
        ref_state = g[f"t_{name}_state300"]
        # Hprime_prev = 2 (H - H_prev) / Ts - Hprime_prev: three roundings per sample, each of a value below the largest
        assert np.abs(state[:, 2] - ref_state[:, 2]).max() <= 300 * 4 * U53 * np.abs(H).max() * 2 / TS, name
        if name == "zeros":
            assert not M.any() and not state.any()
        if name == "sat":
            assert ((M == PAR[0]) == (want == PAR[0])).mean() > 0.99 and ((M == -PAR[0]) == (want == -PAR[0])).mean() > 0.99
            assert (M == PAR[0]).any() and (M == -PAR[0]).any()
    assert not bad, bad


def test_nonzero_initial_state_is_continued(ntm, g):
    """From the fixture's state after 150 samples (rounded to fp64: within the floor), samples [150, 300) follow the
    mpmath trajectory within the family's bar, and equal the second half of a two-call run bit for bit."""
    for name in ("walk_small", "sin1000", "chain"):
        H, want, eref = g[f"t_{name}_H"], g[f"t_{name}_M"], float(g[f"t_{name}_eref"])
        M2, s2 = hmag(ntm, dev(H[:, 150:]), dev(g[f"t_{name}_state150"]))
        bar = max(MARGIN * eref, 300 * U53 * np.abs(want).max())
        assert np.abs(M2.cpu().numpy() - want[:, 150:]).max() <= bar, name
        Mo, _ = oracle.tape_hmag(H[:, 150:], g[f"t_{name}_state150"], TS, PAR)
        assert np.abs(M2.cpu().numpy() - Mo).max() <= bar, name
        Ma, sa = hmag(ntm, dev(H[:, :150]))
        Mb, sb = hmag(ntm, dev(H[:, 150:]), sa)
        Mf, sf = hmag(ntm, dev(H))
        assert torch.equal(torch.cat([Ma, Mb], 1), Mf) and torch.equal(sb, sf), name


# ------------------------------------------------------------------------------------------ shapes and state, bit for bit
def fixture_rows(g, seed, B, N):
    """B streams of N <= 300 samples drawn (with repetition, every one present from B = 16 on) from the 16 streams of
    the four unsaturated families of golden g25 -> (H, M by mpmath, M by the oracle, the oracle's final state).
    Why not fresh random input against the oracle: on 130 random walks of the walk_small construction the ORACLE is
    up to 16 x 4 E_ref(walk_small) away from a CPU emulation of the kernel's arithmetic (its closed form of L' loses
    1e-8 where |L(Q)| is small, and how often a stream passes there varies): the oracle is only a reference where its
    own error is known, which is on the fixture's streams."""
    fams = [str(f) for f in g["families"][:4]]
    H16 = np.concatenate([g[f"t_{f}_H"] for f in fams])
    M16 = np.concatenate([g[f"t_{f}_M"] for f in fams])
    idx = np.random.default_rng(seed).permutation(np.arange(max(B, 16)) % 16)[:B] if B >= 16 else np.random.default_rng(seed).integers(0, 16, B)
    H = np.ascontiguousarray(H16[idx, :N])
    Mo, so = oracle.tape_hmag(H, None, TS, PAR)
    return H, M16[idx, :N], Mo, so


def prefix_bar(Mref, Mo, N):
    """(bar, E_ref): the trajectory bar max(4 E_ref, N 2^-53 max|M_ref|) with the oracle's error on these very rows and
    samples; below eight samples the floor is that of eight (one RK4 sample, m = Mp + k1/6 + k2/3 + k3/3 + k4/6, is itself
    four rounded products and four rounded sums)."""
    eref = float(np.abs(Mo - Mref).max())
    return max(MARGIN * eref, max(N, 8) * U53 * float(np.abs(Mref).max())), eref


def check_rows(g, ntm, seed, B, N):
    H, Mref, Mo, so = fixture_rows(g, seed, B, N)
    M, state = hmag(ntm, dev(H))
    Mh, sh = M.cpu().numpy(), state.cpu().numpy()
    bar, eref = prefix_bar(Mref, Mo, N)
    assert np.isfinite(Mh).all() and np.abs(Mh - Mref).max() <= bar, (B, N, np.abs(Mh - Mref).max(), bar)
    # against the oracle: |gpu - oracle| <= E_gpu + E_ref
    assert np.abs(Mh - Mo).max() <= bar + eref and np.abs(sh[:, 0] - so[:, 0]).max() <= bar + eref, (B, N)
    assert np.array_equal(sh[:, 0], Mh[:, -1]) and np.array_equal(sh[:, 1], so[:, 1]), (B, N)
    assert np.abs(sh[:, 2] - so[:, 2]).max() <= 4 * 2.0 ** -52 * np.abs(so[:, 2]).max(), (B, N)
    return M, state


@pytest.mark.parametrize("B", TAPE_HMAG_B)
def test_hmag_shape_grid_against_mpmath_and_the_oracle(ntm, g, B):
    """Every (B, N) around the 64 x 64 LDS tile on unsaturated input (rows of the fixture's unsaturated families in a
    random order): M within the trajectory bar of mpmath, M and the state rows within it of the oracle (the output
    starts as NaN: every sample must have been written)."""
    for N in TAPE_HMAG_N:
        check_rows(g, ntm, 1000 * B + N, B, N)


@pytest.mark.parametrize("N", TAPE_CUT_N)
def test_hmag_cut_lists_bit_for_bit(ntm, N):
    """One call over [0, N) equals the concatenation of calls over every cut list with the state carried; so do the
    final states."""
    H = dev(tape_walk(N, 65, N))
    Mf, sf = hmag(ntm, H)
    for cuts in tape_cut_lists(N):
        Mc, sc = hmag_cuts(ntm, H, cuts)
        assert torch.equal(Mc, Mf) and torch.equal(sc, sf), cuts[:4]


def test_hmag_stream_alone_equals_stream_in_a_batch(ntm):
    H = dev(tape_walk(5, 129, 193))
    s0 = dev(np.random.default_rng(6).standard_normal((129, 3)) * [1e4, 1e2, 1e7])
    Mf, sf = hmag(ntm, H, s0)
    for b in TAPE_SINGLE_STREAMS:
        M1, s1 = hmag(ntm, H[b:b + 1], s0[b:b + 1])
        assert torch.equal(M1[0], Mf[b]) and torch.equal(s1[0], sf[b]), b


@settings(max_examples=30, **SET)
@given(B=st.integers(1, 130), N=st.integers(1, 260), seed=st.integers(0, 2 ** 16), cuts=st.lists(st.integers(1, 259), max_size=3))
def test_hmag_sweep_chunk_invariance_and_oracle(ntm, g, B, N, seed, cuts):
    """B 1..130, N 1..260, up to three cuts: chunk invariance bit for bit on a random walk (distinct streams) and on
    fixture rows, and the fixture rows against mpmath and the oracle within their bar (see fixture_rows)."""
    edges = sorted({c for c in cuts if c < N})
    lens = [b - a for a, b in zip([0] + edges, edges + [N])]
    Hw = dev(tape_walk(seed, B, N))
    Mf, sf = hmag(ntm, Hw)
    Mc, sc = hmag_cuts(ntm, Hw, lens)
    assert torch.equal(Mc, Mf) and torch.equal(sc, sf), (B, N, lens)
    Mf, sf = check_rows(g, ntm, seed, B, N)
    Mc, sc = hmag_cuts(ntm, dev(fixture_rows(g, seed, B, N)[0]), lens)
    assert torch.equal(Mc, Mf) and torch.equal(sc, sf), (B, N, lens)


# ------------------------------------------------------------------------------------------ ntm_resample_fir, raw ABI
def resample(ntm, x, ker, width, up, down, M):
    L = ntm._lib
    B, N = x.shape
    y = torch.full((B, M), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib().ntm_resample_fir(L.ptr(x), L.ptr(y), B, N, M, up, down, width, L.ptr(ker), L.current_stream()), "ntm_resample_fir")
    return y


@pytest.mark.parametrize("orig,new", RESAMPLE_RATIOS)
def test_resample_fir_against_longdouble(ntm, orig, new):
    """Any up / down / width / N / M: every output sample within taps 2^-53 sum_k |ker[p][k]| |xpad[i down + k]| (the
    standard bound of a chain of `taps` fused multiply-adds) of include/ntm.h's formula in longdouble, and, the inputs
    being the same, bit for bit independent of M and of B."""
    from ntm_amd.tape import sinc_resample_kernel
    ker, width, down, up = sinc_resample_kernel(orig, new)
    taps, kd = 2 * width + down, dev(ker)
    for N in resample_lengths(width):
        x = resample_input(N, 3, N)
        xd = dev(x)
        full = math.ceil(up * N / down)
        base = None
        for M in resample_out_lengths(N, up, down):
            want, s = resample_ref_ld(x, ker, width, up, down, M)
            y = resample(ntm, xd, kd, width, up, down, M)
            yh = y.cpu().numpy()
            assert np.isfinite(yh).all() and (np.abs(yh - want).astype(np.float64) <= taps * U53 * s).all(), (N, M)
            if M == full:
                base = y
                y1 = resample(ntm, xd[1:2].contiguous(), kd, width, up, down, M)
                assert torch.equal(y1[0], y[1]), (N, M)
            else:
                k = min(M, full)
                assert torch.equal(y[:, :k], base[:, :k]), (N, M)


# ------------------------------------------------------------------------------------------ ntm_fir_f64
def fir(ntm, x, h, clamp):
    L = ntm._lib
    B, N = x.shape
    y = torch.full((B, N), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib().ntm_fir_f64(L.ptr(x), L.ptr(y), B, N, L.ptr(h), h.numel(), int(clamp), L.current_stream()), "ntm_fir_f64")
    return y


@pytest.mark.parametrize("taps", FIR_TAPS)
def test_fir_f64_against_longdouble_and_the_clamp(ntm, taps):
    """y[n] = sum_{k < taps, k <= n} h[k] x[n-k] within taps 2^-53 sum |h[k]| |x[n-k]| of the longdouble sum; clamped,
    every output lies in [-1, 1] and equals the unclamped one wherever that lies inside (outputs exactly on +-1, one
    unit in the last place inside, and far outside are all present)."""
    for N in fir_lengths(taps):
        x, h = fir_case(taps, N)
        want, s = fir_ref_ld(x, h)
        y0 = fir(ntm, dev(x), dev(h), False).cpu().numpy()
        y1 = fir(ntm, dev(x), dev(h), True).cpu().numpy()
        assert np.isfinite(y0).all() and (np.abs(y0 - want).astype(np.float64) <= taps * U53 * s).all(), N
        assert y0[0, 0] == 1.0 and y0[1, 0] == -1.0
        assert np.array_equal(y1, np.clip(y0, -1.0, 1.0)) and np.abs(y1).max() <= 1.0, N
        inside = np.abs(y0) <= 1.0
        assert np.array_equal(y1[inside], y0[inside])
        if N > taps:
            assert y0[0, -1] == -(1.0 - U53) and y0[1, -1] == 1.0 - U53 and y1[0, -1] == y0[0, -1]


# ------------------------------------------------------------------------------------------ ntm_tape_record_field
def record_field(ntm, I, bias, gain, gap):
    L = ntm._lib
    B, N = I.shape
    H = torch.full((B, N), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib().ntm_tape_record_field(L.ptr(I), L.ptr(bias), L.ptr(H), B, N, gain, gap, L.current_stream()), "ntm_tape_record_field")
    return H


@pytest.mark.parametrize("B,N", RECORD_SHAPES + (RECORD_BIG,))
def test_record_field_bit_for_bit(ntm, B, N):
    """H = (gain (I + bias[n])) / gap as numpy's fp64 evaluates it, with a bias and with none; the last shape is the
    smallest with B = 3 at which the grid-stride loop goes round a second time (B N just above 65536 x 256)."""
    rng = np.random.default_rng(B * N % 9973)
    gain, gap = 100 * 0.1, 6e-6
    I = rng.standard_normal((B, N)) * 1e-3
    bias = rng.standard_normal(N) * 5e-3
    Id, bd = dev(I), dev(bias)
    got = record_field(ntm, Id, bd, gain, gap)
    assert torch.equal(got, dev((gain * (I + bias[None, :])) / gap))
    del got
    got = record_field(ntm, Id, None, gain, gap)
    assert torch.equal(got, dev((gain * I) / gap))


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_and_empty_calls_through_the_raw_abi(ntm):
    L = ntm._lib
    lib, lab, P, S = L.lib(), L.lab(), L.ptr, L.current_stream()
    a = torch.zeros(4, 16, dtype=torch.float64, device="cuda")
    out = torch.full((4, 16), -7.0, dtype=torch.float64, device="cuda")
    state = torch.full((4, 3), -7.0, dtype=torch.float64, device="cuda")
    ker = torch.ones(2, 5, dtype=torch.float64, device="cuda")
    par = _par()

    def refused(rc, text, err=lib.ntm_last_error):
        assert rc == EINVAL and text in err().decode(), (rc, text, err().decode())

    for B, N, Ts in ((-1, 16, TS), (4, -1, TS), (4, 16, 0.0), (4, 16, -TS), (4, 16, float("nan"))):
        refused(lib.ntm_tape_hmag(P(a), P(out), B, N, P(state), Ts, par, S), "ntm_tape_hmag: bad size or Ts")
    for H, M, s, p in ((None, out, state, par), (a, None, state, par), (a, out, None, par), (a, out, state, None)):
        refused(lib.ntm_tape_hmag(P(H), P(M), 4, 16, P(s), TS, p, S), "ntm_tape_hmag: null pointer")
    for B, N, gap in ((-1, 16, 1.0), (4, -1, 1.0), (4, 16, 0.0), (4, 16, float("nan"))):
        refused(lib.ntm_tape_record_field(P(a), None, P(out), B, N, 1.0, gap, S), "ntm_tape_record_field: bad size or gap")
    for I, H in ((None, out), (a, None)):
        refused(lib.ntm_tape_record_field(P(I), None, P(H), 4, 16, 1.0, 1.0, S), "ntm_tape_record_field: null pointer")
    for B, N, M, up, down, width in ((-1, 16, 8, 2, 1, 2), (4, -1, 8, 2, 1, 2), (4, 16, -1, 2, 1, 2), (4, 16, 8, 0, 1, 2),
                                     (4, 16, 8, 2, 0, 2), (4, 16, 8, 2, 1, -1)):
        refused(lib.ntm_resample_fir(P(a), P(out), B, N, M, up, down, width, P(ker), S), "ntm_resample_fir: bad size")
    refused(lib.ntm_resample_fir(P(a), P(out), 65536, 16, 8, 2, 1, 2, P(ker), S), "ntm_resample_fir: at most 65535 streams")
    for x, y, k in ((None, out, ker), (a, None, ker), (a, out, None), (a, a, ker)):
        refused(lib.ntm_resample_fir(P(x), P(y), 4, 16, 8, 2, 1, 2, P(k), S), "ntm_resample_fir: null or aliased pointer")
    for B, N, taps in ((-1, 16, 5), (4, -1, 5), (4, 16, 0), (4, 16, -3)):
        refused(lib.ntm_fir_f64(P(a), P(out), B, N, P(ker), taps, 1, S), "ntm_fir_f64: bad size")
    refused(lib.ntm_fir_f64(P(a), P(out), 65536, 16, P(ker), 5, 1, S), "ntm_fir_f64: at most 65535 streams")
    for x, y, h in ((None, out, ker), (a, None, ker), (a, out, None), (a, a, ker)):
        refused(lib.ntm_fir_f64(P(x), P(y), 4, 16, P(h), 5, 1, S), "ntm_fir_f64: null or aliased pointer")
    for op in (-1, 5):
        refused(lab.ntm_lab_tape_math(op, P(a), P(out), 16, par, S), "ntm_lab_tape_math: op", lab.ntm_lab_last_error)
    refused(lab.ntm_lab_tape_math(0, P(a), P(out), -1, par, S), "ntm_lab_tape_math: negative n", lab.ntm_lab_last_error)
    for x, y, op, p in ((None, out, 0, par), (a, None, 0, par), (a, a, 0, par)):
        refused(lab.ntm_lab_tape_math(op, P(x), P(y), 16, p, S), "ntm_lab_tape_math: null or aliased pointer", lab.ntm_lab_last_error)
    refused(lab.ntm_lab_tape_math(4, P(a), P(out), 4, None, S), "ntm_lab_tape_math: NTM_LAB_TAPE_JA_F needs params5", lab.ntm_lab_last_error)
    # empty calls: NTM_OK, nothing written
    for B, N in ((0, 16), (4, 0)):
        assert lib.ntm_tape_hmag(P(a), P(out), B, N, P(state), TS, par, S) == 0
        assert lib.ntm_tape_record_field(P(a), None, P(out), B, N, 1.0, 1.0, S) == 0
        assert lib.ntm_fir_f64(P(a), P(out), B, N, P(ker), 5, 1, S) == 0
    assert lib.ntm_resample_fir(P(a), P(out), 0, 16, 8, 2, 1, 2, P(ker), S) == 0
    assert lib.ntm_resample_fir(P(a), P(out), 4, 16, 0, 2, 1, 2, P(ker), S) == 0
    assert lab.ntm_lab_tape_math(0, P(a), P(out), 0, par, S) == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (state == -7.0).all()


# ------------------------------------------------------------------------------------------ Tape end to end
def test_tape_startup_then_one_call_equals_the_oracle_chain(ntm):
    """Tape(batch_size=2, startup_enable=True): the 480 start-up zeros and then a call of 300 samples, against the
    oracle's composition of the same stages (as in test_gpu_round2.py::test_tape_resamplers_playback_filter_and_whole_chain,
    at that test's bar)."""
    B = 2
    V = 0.5 * np.random.default_rng(23).standard_normal((B, 300))
    tp = ntm.Tape(batch_size=B, startup_enable=True, playback_loss_enable=False)
    assert tp.FLAG_STARTUP is False and tp.M.shape == (B, 480) and tp.M_OS.shape == (B, 480 * 16)
    out = tp(dev(V))
    ref = ntm.TapeMagnetization(batch_size=B)            # host-side bias waveform generator (pinned by golden g14)
    g_play = tp.PLAY_N * tp.PLAY_W * tp.PLAY_E * tp.TAPE_V * tp.PLAY_MU0 * tp.PLAY_G
    state, m_os_prev, m_prev = None, np.zeros((B, 0)), np.zeros((B, 0))
    for Vc in (np.zeros((B, 480)), V):
        I_os = oracle.sinc_resample(tp.signal_amplitude * Vc, 48000, 768000)
        H = (10.0 * (I_os + ref.bias_signal(I_os.shape[1])[None, :])) / 6e-6
        M_os, state = oracle.tape_hmag(H, state, tp.Ts_OS)
        M = oracle.sinc_resample(np.concatenate([m_os_prev, M_os], 1), 768000, 48000)[:, m_prev.shape[1]:]
        m_os_prev, m_prev = M_os, M
        want = tp.POST_GAIN * (g_play * M)
    assert out.shape == (B, 300) and torch.isfinite(out).all()
    assert np.abs(out.cpu().numpy() - want).max() < 1e-6 * tp.POST_GAIN * g_play * tp.TAPE_Ms
    assert np.abs(want).max() > 1e-3 * tp.POST_GAIN * g_play * tp.TAPE_Ms          # the comparison is not of zeros
    assert abs(tp.bias_phase - ref.bias_phase) < 1e-15


def test_tape_short_batch_equals_hand_padded_batch(ntm):
    """A call with 2 streams on batch_size = 4 is the first two rows of the same call padded by hand with zero streams,
    bit for bit, over two stateful calls."""
    V = 0.5 * np.random.default_rng(29).standard_normal((2, 500))
    a, b = ntm.Tape(batch_size=4), ntm.Tape(batch_size=4)
    for sl in (slice(0, 300), slice(300, 500)):
        ya = a(dev(V[:, sl]))
        yb = b(dev(np.concatenate([V[:, sl], np.zeros((2, sl.stop - sl.start))], 0)))
        assert ya.shape == (2, sl.stop - sl.start) and torch.equal(ya, yb[:2])
    assert torch.equal(a._state, b._state)
