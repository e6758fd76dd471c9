"""The time-domain loss kernels against an exact reference at their structural edges and on badly conditioned inputs:
esr_dcpre_kernel and esr_sums_kernel (csrc/aux_kernels.hip) through the raw C ABI, the fused flush (dcp_filter /
dcp_accumulate in csrc/gru_mfma2.hip) through RNN.predict_losses / DiffDelRNN.predict_losses.  The reference is
tests/helpers.py's numpy.longdouble recursion on the same float32 inputs (dcpre_sums_exact / esr_sums_exact, pinned to mpmath
by tests/test_oracle_losses.py, which also checks that every case asserted here at the 2e-5 bar is well conditioned: the
float32 sequential recursion is within 2e-6 of exact on it).  Every output buffer is pre-filled with NaN, so a row that a
kernel does not write fails the comparison.  Each test prints the worst error it saw (`LOSSERR ...`): DESIGN.md's table of
measured errors is made of those lines."""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle
from helpers import (DCPRE_COND_B, DCPRE_COND_N, DCPRE_COND_POLES, DCPRE_COND_SEED, DCPRE_COND_SKIP, DCPRE_GROWTH_B, DCPRE_GROWTH_FAMILIES,
                     DCPRE_GROWTH_N, DCPRE_GROWTH_SEED, DCPRE_STRUCT_B, DCPRE_STRUCT_N, DCPRE_STRUCT_SEED, DCPRE_STRUCT_SKIP, FLUSH_FAMILIES,
                     FLUSH_POLES, FLUSH_SEED, FLUSH_T, LOSS_BAR, LOSS_FAMILIES, R_BELOW_ONE, dcpre_sums_exact, esr_sums_exact, flush_skips,
                     loss_family, rel_err)

pytestmark = pytest.mark.gpu

W_G = "GRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE]_BEST"
W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"
NAN = float("nan")
# esr_dcpre_kernel at pole 0.9999 and n = 65 536: the error measured on an MI355X against exact is 3.04e-5 on dc_small_ac
# (4.1e-6 on slow_sine), above the 2e-5 bar -- the float32 filter's rounding has 1 / (1 - R) = 10 000 samples of memory there and
# the sums grow with n (DESIGN.md section 2 has the table).  The long case is held at twice the measured value.
GROWTH_9999_MEASURED = 3.04e-5
GROWTH_9999_BAR = 2 * GROWTH_9999_MEASURED
GROWTH_9999_SWEEP = (8192, 16384, 32768)        # recorded, not asserted: where between 4097 and 65 536 the 2e-5 is crossed


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _place(a, off):
    """A (B, T) float32 array on the device, `off` floats into a NaN-filled allocation (with NaN behind it too): the base
    pointer is 4 * off bytes off torch's 256-byte alignment, and a read outside the B * T floats poisons the result."""
    buf = torch.full((a.size + off + 4,), NAN, dtype=torch.float32, device="cuda")
    buf[off:off + a.size] = torch.from_numpy(np.ascontiguousarray(a).ravel()).cuda()
    return buf, ctypes.c_void_p(buf.data_ptr() + 4 * off)


def raw_dcpre(ntm, y, t, skip, R, off=0):
    """ntm_esr_dcpre_sums through the raw ABI into a NaN-filled (B, 2) float64 buffer -> numpy."""
    B, T = y.shape
    ybuf, yp = _place(y, off)
    tbuf, tp = _place(t, off)
    out = torch.full((B, 2), NAN, dtype=torch.float64, device="cuda")
    rc = ntm._lib.lib().ntm_esr_dcpre_sums(yp, tp, B, T, int(skip), float(R), ntm._lib.ptr(out), ntm._lib.current_stream())
    ntm._lib.check(rc, "ntm_esr_dcpre_sums")
    return out.cpu().numpy()


def raw_esr(ntm, y, t, skip, splits, off=0):
    """ntm_esr_sums through the raw ABI into a NaN-filled (B, splits, 2) float64 buffer -> numpy."""
    B, T = y.shape
    ybuf, yp = _place(y, off)
    tbuf, tp = _place(t, off)
    out = torch.full((B, splits, 2), NAN, dtype=torch.float64, device="cuda")
    rc = ntm._lib.lib().ntm_esr_sums(yp, tp, B, T, int(skip), int(splits), ntm._lib.ptr(out), ntm._lib.current_stream())
    ntm._lib.check(rc, "ntm_esr_sums")
    return out.cpu().numpy()


def check_sums(got, want, bar, what):
    """Every entry written and finite, exact zero where the exact sum is zero, within `bar` relative elsewhere (atol = 0)
    -> the worst relative error."""
    assert got.shape == want.shape and np.isfinite(got).all(), (what, got)
    err = rel_err(got, want)
    assert (got[want == 0] == 0).all(), (what, got[want == 0])
    worst = float(err.max(initial=0.0))
    assert worst <= bar, (what, worst, bar)
    return worst


def record(kernel, pole, group, n, err):
    print(f"LOSSERR kernel={kernel} pole={pole} group={group} n={n} err={err:.3e}")


# ----------------------------------------------------------------------------- a. streaming kernel: structure
@pytest.mark.parametrize("n", DCPRE_STRUCT_N)
def test_streaming_dcpre_structure(ntm, n):
    """Chunk and quarter edges of esr_dcpre_kernel (n = 1025: quarter 1 holds one sample; 4097: five chunks, two per quarter,
    quarter 3 starts beyond T; 0 .. 17: one lane, one lane's run and one sample more), slow_sine at pole 0.995 -- the state
    entering a quarter is large, so the chaining terms 2 c S1 + c^2 C2 carry weight.  skip 0 / 7 / 1024 with T = skip + n, and
    skip = T - 1 and skip = T of the same signals."""
    worst = 0.0
    for skip in DCPRE_STRUCT_SKIP:
        y, t = loss_family("slow_sine", DCPRE_STRUCT_SEED, DCPRE_STRUCT_B, skip + n)
        got = raw_dcpre(ntm, y, t, skip, 0.995)
        if n == 0:
            assert (got == 0).all() and not np.signbit(got).any(), got
        worst = max(worst, check_sums(got, dcpre_sums_exact(y, t, skip, 0.995), LOSS_BAR, (n, skip)))
        T = skip + n
        if T >= 1:
            worst = max(worst, check_sums(raw_dcpre(ntm, y, t, T - 1, 0.995), dcpre_sums_exact(y, t, T - 1, 0.995), LOSS_BAR, (n, "T-1")))
        zero = raw_dcpre(ntm, y, t, T, 0.995)
        assert zero.shape == (DCPRE_STRUCT_B, 2) and (zero == 0).all(), (n, skip, zero)
    record("streaming", 0.995, "structure/slow_sine", n, worst)


@pytest.mark.parametrize("n,off,skip", [(1025, 1, 8), (4097, 2, 1024), (8193, 3, 0), (17, 3, 8)])
def test_streaming_dcpre_unaligned_base_pointers(ntm, n, off, skip):
    """ntm_esr_dcpre_sums documents no alignment demand: base pointers 4, 8 and 12 bytes off, odd T (odd row stride)."""
    T = skip + n
    assert T % 2 == 1
    y, t = loss_family("slow_sine", DCPRE_STRUCT_SEED + off, DCPRE_STRUCT_B, T)
    got = raw_dcpre(ntm, y, t, skip, 0.995, off=off)
    check_sums(got, dcpre_sums_exact(y, t, skip, 0.995), LOSS_BAR, (n, off))
    assert np.array_equal(got, raw_dcpre(ntm, y, t, skip, 0.995, off=0))


# ----------------------------------------------------------------------------- b. streaming kernel: conditioning and poles
@pytest.mark.parametrize("name", list(LOSS_FAMILIES))
def test_streaming_dcpre_families_and_poles(ntm, name):
    """Every family x pole {0, 0.5, 0.9, 0.995} x n {17, 1025, 4097} at 2e-5 against exact; pole 0.9999 at max(2e-5, 4 E_ref),
    E_ref the float32 sequential recursion's own error on the case; the largest float32 below 1 finite and its error recorded."""
    worst = {}
    for n in DCPRE_COND_N:
        y, t = loss_family(name, DCPRE_COND_SEED, DCPRE_COND_B, DCPRE_COND_SKIP + n)
        poles = DCPRE_COND_POLES + (0.9999, R_BELOW_ONE)
        exact = dcpre_sums_exact(y, t, DCPRE_COND_SKIP, poles)
        for i, R in enumerate(poles):
            got = raw_dcpre(ntm, y, t, DCPRE_COND_SKIP, R)
            if R in DCPRE_COND_POLES:
                e = check_sums(got, exact[i], LOSS_BAR, (name, R, n))
            elif R == 0.9999:
                e_ref = float(rel_err(oracle.esr_dcpre_sums(y, t, DCPRE_COND_SKIP, R), exact[i]).max())
                e = check_sums(got, exact[i], max(LOSS_BAR, 4 * e_ref), (name, R, n, e_ref))
            else:
                assert np.isfinite(got).all() and (got >= 0).all(), (name, R, n, got)
                e = float(rel_err(got, exact[i]).max())
            worst[R] = max(worst.get(R, 0.0), e)
    for R, e in worst.items():
        record("streaming", R, name, "17..4097", e)


@pytest.mark.parametrize("name", DCPRE_GROWTH_FAMILIES)
def test_streaming_dcpre_growth(ntm, name):
    """n = 65 536 (16 chunks per quarter): the float32 weights R^(k+1) of the chaining sums have decayed to 2e-36 at pole
    0.995 by the end of a quarter and the error of the state entering a quarter has had 16 384 samples to grow.  2e-5 at
    the shipped pole; pole 0.9999 at GROWTH_9999_BAR (module top: measured 3.04e-5 on dc_small_ac, a finding -- the 2e-5 does
    not hold there), the lengths in between recorded."""
    y, t = loss_family(name, DCPRE_GROWTH_SEED, DCPRE_GROWTH_B, DCPRE_GROWTH_N)
    exact = dcpre_sums_exact(y, t, 0, (0.995, 0.9999))
    e995 = float(rel_err(raw_dcpre(ntm, y, t, 0, 0.995), exact[0]).max())
    got = raw_dcpre(ntm, y, t, 0, 0.9999)
    e9999 = float(rel_err(got, exact[1]).max())
    record("streaming", 0.995, "growth/" + name, DCPRE_GROWTH_N, e995)
    record("streaming", 0.9999, "growth/" + name, DCPRE_GROWTH_N, e9999)
    for m in GROWTH_9999_SWEEP:
        ym, tm = np.ascontiguousarray(y[:, :m]), np.ascontiguousarray(t[:, :m])
        record("streaming", 0.9999, "growth/" + name, m, float(rel_err(raw_dcpre(ntm, ym, tm, 0, 0.9999), dcpre_sums_exact(ym, tm, 0, 0.9999)).max()))
    assert e995 <= LOSS_BAR, (name, e995)
    assert np.isfinite(got).all() and e9999 <= GROWTH_9999_BAR, (name, e9999)


# ----------------------------------------------------------------------------- c. isolation
def _isolation(run, n, skip):
    """`run(y, t) -> (B, ..) rows`: the row of one stream must not depend on the sample at skip - 1, on its neighbours or on
    where it sits in the batch, and a NaN inside [skip, T) of one stream stays in that row."""
    T = skip + n
    y, t = loss_family("slow_sine", 61, 3, T)
    base = run(y, t)
    assert np.isfinite(base).all()
    for bad in (NAN, 1e30):
        y2, t2 = y.copy(), t.copy()
        y2[:, skip - 1], t2[:, skip - 1] = bad, bad
        assert np.array_equal(run(y2, t2), base), ("skip - 1", bad, n)
    y2, t2 = y.copy(), t.copy()
    y2[[0, 2]], t2[[0, 2]] = NAN, NAN
    got = run(y2, t2)
    assert np.array_equal(got[1], base[1]) and np.isnan(got[[0, 2]]).all(), ("neighbours", n)
    alone = run(y[1:2], t[1:2])
    assert np.array_equal(alone[0], base[1]), ("alone", n)
    y70, t70 = loss_family("noise_offset", 62, 70, T)
    y70[37], t70[37] = y[1], t[1]
    assert np.array_equal(run(y70, t70)[37], base[1]), ("row 37 of 70", n)
    for pos in (skip, skip + n // 2, T - 1):
        y2, t2 = y.copy(), t.copy()
        y2[1, pos], t2[1, pos] = NAN, NAN
        got = run(y2, t2)
        assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2]], base[[0, 2]]), ("NaN inside", pos, n)


@pytest.mark.parametrize("n,skip", [(1025, 7), (4097, 1024), (17, 1)])
def test_streaming_dcpre_rows_are_isolated(ntm, n, skip):
    _isolation(lambda y, t: raw_dcpre(ntm, y, t, skip, 0.995), n, skip)


@pytest.mark.parametrize("n,skip,splits", [(1025, 7, 3), (4097, 1024, 1), (17, 1, 2)])
def test_esr_sums_rows_are_isolated(ntm, n, skip, splits):
    _isolation(lambda y, t: raw_esr(ntm, y, t, skip, splits).sum(1), n, skip)


# ----------------------------------------------------------------------------- d. esr_sums_kernel
ESR_SLAB = 256


def _esr_rows_f64(y, t, skip, splits):
    """(B, splits, 2): row p = the sum over exactly the 256-sample slabs p, p + splits, ... of [skip, T)."""
    e, tt = (t - y).astype(np.longdouble), t.astype(np.longdouble)
    B, T = y.shape
    out = np.zeros((B, splits, 2), np.longdouble)
    slab = (np.arange(skip, T) - skip) // ESR_SLAB
    for p in range(splits):
        idx = skip + np.nonzero(slab % splits == p)[0]
        out[:, p, 0] = (e[:, idx] ** 2).sum(1)
        out[:, p, 1] = (tt[:, idx] ** 2).sum(1)
    return out


def _esr_check(ntm, y, t, skip, splits, what, off=0):
    got = raw_esr(ntm, y, t, skip, splits, off=off)
    want = _esr_rows_f64(y, t, skip, splits)
    assert got.shape == want.shape and np.isfinite(got).all(), (what, got)               # every partial row is written
    n_slabs = -(-(y.shape[1] - skip) // ESR_SLAB)
    assert (got[:, n_slabs:] == 0).all() and (got[want == 0] == 0).all(), what            # a row without a slab: exact zero
    err = float(rel_err(got, want).max(initial=0.0))
    assert err <= 1e-13, (what, err)
    total = np.zeros((y.shape[0], 2))
    for p in range(splits):                                                               # the caller's order
        total = total + got[:, p]
    err_t = float(rel_err(total, esr_sums_exact(y, t, skip)).max(initial=0.0))
    assert err_t <= 1e-13, (what, err_t)
    return max(err, err_t)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4097])
def test_esr_sums_partition(ntm, n):
    slabs = -(-n // ESR_SLAB)
    worst = 0.0
    for splits in sorted({1, 2, 3, slabs, slabs + 1, 64} - {0}):
        for skip, off in ((0, 0), (5, 1)):
            y, t = loss_family("noise_offset", 71 + n, 3, skip + n)
            worst = max(worst, _esr_check(ntm, y, t, skip, splits, (n, splits, skip), off=off))
    record("esr_sums", "-", "partition/noise_offset", n, worst)


def test_esr_sums_magnitudes(ntm):
    """Squares that overflow float32 (inputs of 1e25) are finite and exact: the products are formed in float64.  float32
    subnormal inputs give the exact non-zero sums: nothing is flushed on the way to the float64 product.  tight_fit: t - y is
    the float32 subtraction by definition, so column 0 holds to 1e-13 like any other."""
    rng = np.random.default_rng(73)
    B, n, skip, splits = 2, 4097, 5, 3
    t = (1e25 * (1.0 + 0.1 * rng.standard_normal((B, skip + n)))).astype(np.float32)
    y = (0.5 * t).astype(np.float32)
    with np.errstate(over="ignore"):
        assert np.isinf(t * t).all() and np.isinf((t - y) * (t - y)).all()
    record("esr_sums", "-", "1e25", n, _esr_check(ntm, y, t, skip, splits, "1e25"))
    tiny = np.float32(2.0 ** -149)
    t = rng.integers(-2 ** 20, 2 ** 20, (B, skip + n)).astype(np.float32) * tiny
    y = rng.integers(-2 ** 20, 2 ** 20, (B, skip + n)).astype(np.float32) * tiny
    assert np.abs(t).max() < np.finfo(np.float32).tiny and np.count_nonzero(t) > n and np.count_nonzero(t - y) > n
    assert (esr_sums_exact(y, t, skip) > 0).all()
    record("esr_sums", "-", "subnormal", n, _esr_check(ntm, y, t, skip, splits, "subnormal"))
    y, t = loss_family("tight_fit", 74, B, skip + n)
    record("esr_sums", "-", "tight_fit", n, _esr_check(ntm, y, t, skip, splits, "tight_fit"))


def test_esr_default_splits_rule(ntm):
    """include/ntm.h: the split count that fills the device, 1 for B >= 2048 -- at least 4096 samples (16 per thread) per
    workgroup, no more workgroups than ceil(2048 / B) per stream, never below 1."""
    L = ntm._lib.lib()
    for B in (1, 8, 2048, 4096):
        for n in (0, 1, 4095, 4096, 4097, 65536, 441000, 10 ** 7):
            for skip in (0, 1024):
                want = 1 if n <= 0 else max(1, min(math.ceil(n / 4096), math.ceil(2048 / B)))
                assert L.ntm_esr_splits(B, skip + n, skip) == want, (B, n, skip)
                assert B < 2048 or want == 1


# ----------------------------------------------------------------------------- e. fused flush
@pytest.fixture(scope="module")
def gru(ntm):
    return ntm.harness.build_model(W_G)


def _flush_case(ntm, m, name, B, T, skips, poles, seed):
    """RNN.predict_losses on B streams (the matrix-pipe launch from 1025 streams up): y bit-identical to predict(), both
    DCPreESR columns of ALL rows against exact on the returned y.  The float32 sequential recursion is within 2e-6 of exact on
    the same rows (the input condition of the 2e-5 bar; column 1 is checked on the CPU as well) -> worst error per pole."""
    rng = np.random.default_rng(seed + T)
    x = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)
    _, t = loss_family(name, seed, B, T)
    xd, td = dev(x).unsqueeze(1), dev(t).unsqueeze(1)
    y0 = m.predict(xd)
    y_np = y0[:, 0].cpu().numpy()
    worst = dict.fromkeys(poles, 0.0)
    for skip in skips:
        exact = dcpre_sums_exact(y_np, t, skip, poles)
        for i, R in enumerate(poles):
            y, s, d = m.predict_losses(xd, td, skip=skip, R=R)
            assert torch.equal(y, y0), (name, T, skip, R)
            e_ref = float(rel_err(oracle.esr_dcpre_sums(y_np, t, skip, R), exact[i]).max(initial=0.0))
            assert e_ref <= LOSS_BAR / 10, (name, T, skip, R, e_ref)
            worst[R] = max(worst[R], check_sums(d.cpu().numpy(), exact[i], LOSS_BAR, (name, B, T, skip, R)))
            assert rel_err(s.cpu().numpy(), esr_sums_exact(y_np, t, skip)).max(initial=0.0) <= 1e-13, (name, T, skip)
    return worst


@pytest.mark.parametrize("T", FLUSH_T)
@pytest.mark.parametrize("name", FLUSH_FAMILIES)
def test_fused_flush_dcpre_vs_exact(ntm, gru, name, T):
    """T: one ragged tile, exactly one / two tiles and one sample either side, several tiles; skip 0, 4 (inside the first
    tile), 64 and 68 (the second), T rounded down to 4 (an empty or 1 .. 3-sample window); poles 0.995, 0.9 and 0."""
    worst = _flush_case(ntm, gru, name, 1040, T, flush_skips(T), FLUSH_POLES, FLUSH_SEED)
    for R, e in worst.items():
        record("fused_flush", R, name, T, e)


@pytest.mark.parametrize("B", [4200, 4112])
def test_fused_flush_dcpre_other_launch_shapes(ntm, gru, B):
    """4200 > 4096 streams: the YPN = 4 instantiation (three workgroups per CU); 4112 = whole device rounds and 16 remainder
    rows, which take the low-latency kernel and the streaming passes."""
    worst = _flush_case(ntm, gru, "slow_sine", B, 129, (64,), (0.995,), FLUSH_SEED + 1)
    record("fused_flush", 0.995, f"slow_sine/B={B}", 129, worst[0.995])


@pytest.fixture(scope="module")
def diffdel(ntm):
    m = ntm.DiffDelRNN(1, 64, 1, skip=False, max_delay=36)        # a delay buffer of D = 37 samples
    m.load_state_dict(ntm.weights.load_state_dict(W_D))
    return m.to("cuda").eval()


def _diffdel_inputs(B, T):
    rng = np.random.default_rng(FLUSH_SEED + 2)
    x = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)
    _, t = loss_family("slow_sine", FLUSH_SEED + 2, B, T)
    d = np.full((B, T), 20.25, np.float32)
    return x, t, d


def test_fused_delay_stage_dcpre_vs_exact(ntm, diffdel):
    """DiffDelRNN.predict_losses with the delay line fused into the launch (D = 37, T = 129, a constant delay of 20.25
    samples): the sums are taken on the DELAYED output in the delay stage."""
    B, T, skip = 1040, 129, 64
    x, t, d = _diffdel_inputs(B, T)
    xd, td, dd = dev(x).unsqueeze(1), dev(t).unsqueeze(1), dev(d).unsqueeze(1)
    assert diffdel.delay_mode == "auto" and int(diffdel.diffdel.max_delay) == 37
    y0, p0 = diffdel.predict(xd, dd)
    y, pre, s, dc = diffdel.predict_losses(xd, dd, td, skip=skip)
    assert torch.equal(y, y0) and torch.equal(pre, p0)
    y_np = y0[:, 0].cpu().numpy()
    exact = dcpre_sums_exact(y_np, t, skip, 0.995)
    e_ref = float(rel_err(oracle.esr_dcpre_sums(y_np, t, skip, 0.995), exact).max())
    assert e_ref <= LOSS_BAR / 10, e_ref
    record("fused_delay_stage", 0.995, "slow_sine", T, check_sums(dc.cpu().numpy(), exact, LOSS_BAR, "diffdel"))
    assert rel_err(s.cpu().numpy(), esr_sums_exact(y_np, t, skip)).max() <= 1e-13


@pytest.mark.parametrize("model", ["gru", "diffdel"])
def test_fused_losses_ignore_the_target_outside_the_window(ntm, gru, diffdel, model):
    """T = 129, skip = 64: the target samples [0, 64) of every stream are NaN -- that is the sample at skip - 1, and, the rows
    being contiguous, the 63 columns of the previous stream's last tile beyond T.  Not a bit of either pair of sums moves."""
    B, T, skip = 1040, 129, 64
    x, t, d = _diffdel_inputs(B, T)
    bad = t.copy()
    bad[:, :skip] = NAN
    xd, dd = dev(x).unsqueeze(1), dev(d).unsqueeze(1)
    run = (lambda tg: gru.predict_losses(xd, dev(tg).unsqueeze(1), skip=skip)) if model == "gru" else \
          (lambda tg: diffdel.predict_losses(xd, dd, dev(tg).unsqueeze(1), skip=skip))
    a, b = run(t), run(bad)
    assert len(a) == (3 if model == "gru" else 4)
    assert torch.isfinite(a[-1]).all() and torch.isfinite(a[-2]).all() and (a[-1] > 0).all()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
