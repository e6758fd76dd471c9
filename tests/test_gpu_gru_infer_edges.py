"""The GRU inference kernels off the headline at their structural edges: gru_small_kernel<8|16|32|64, PAD>, gru_wide_kernel<REGW>
and gru_io_kernel (csrc/gru_small.hip), gru_lat_kernel<HEADW, REP> (csrc/gru_lat.hip, csrc/gru_lat_step.h) -- through the raw ABI
(ntm_gru_forward_ex, ntm_gru_forward_io, ntm_gru_forward_replicas), every output buffer pre-filled with NaN / a sentinel and
checked behind T and behind the last row on EVERY launch.  Tables, inputs and references: tests/gru_infer_cases.py (checked on
the CPU by tests/test_gru_infer_cases_cpu.py).

 (a) accuracy: max|hip - f64| <= 4 max(E_ref, 2^-23 max|f64|) for y and the final h, E_ref = max|oracle32 - f64| pooled over the
     hidden size's table; beside it the project's gate |hip - oracle32| < 1e-5.  `pytest -s` prints every figure as a line
     `GRUERR <kernel>/<y|h> H B T err E_ref ratio` (ratio = err / max(E_ref, ulp): the bar is 4).
 (b) prefix and carry, bit for bit: y(T) = y(T_max)[:, :T]; continuing from the carried state gives y(T_max)[:, T:] and the final
     state.  For `lat` with the head wave (B = 3) and with the rotating head (B = CUs + 1), whose first three rows must agree.
 (c) a stream does not see its neighbours: alone = in the batch = in a batch whose other rows are NaN; one input tiled over all
     rows gives identical rows.
 (d) the padded forms equal the unpadded kernels on explicitly zero-padded weights, as floats, and the padded units end at 0.
 (e) interfaces: row strides above T, NULL h_state, NULL b_o, two equal calls."""
import functools

import numpy as np
import pytest
import torch

import gru_infer_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
Y_PAD, X_PAD = 5, 3


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()       # raises if libntm.so is missing: no silent fallback
    return ntm_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


class Kern:
    """A model on the device and the entry point that runs it: `io` = ntm_gru_forward_io, otherwise ntm_gru_forward_ex with the
    low-latency variant (H = 64 runs gru_lat_kernel, every other H the kernel launch_gru_small picks)."""

    def __init__(self, name, sd, io=False):
        self.name, self.io = name, io
        self.H, self.I, self.O = sd[C.KEYS[1]].shape[1], sd[C.KEYS[0]].shape[1], sd[C.KEYS[4]].shape[0]
        assert io or (self.I == 1 and self.O == 1)
        self.w = [dev(sd[k]) for k in C.KEYS]


def fwd(ntm, k, x, T, h=None, bias=True):
    """One launch on the rows of the device tensor x (B, >= T * I; any row stride) from the state h (B, H), which is overwritten
    with the final state (None: the NULL pointer) -> y (B, T * O).  y is allocated with Y_PAD floats behind every row and a row
    behind the last one, all NaN, and a sentinel row stands behind h: whatever the kernel does not own must be untouched."""
    L = ntm._lib
    B = x.shape[0]
    assert x.stride(1) == 1 and x.shape[1] >= T * k.I and x.is_cuda and x.dtype == torch.float32
    y = torch.full((B + 1, T * k.O + Y_PAD), float("nan"), device="cuda")
    hbuf = None
    if h is not None:
        assert h.shape == (B, k.H) and h.is_contiguous()
        hbuf = torch.full((B + 1, k.H), SENTINEL, device="cuda")
        hbuf[:B] = h
    w = [L.ptr(t) for t in k.w]
    if not bias:
        w[5] = None
    if k.io:
        rc = L.lib().ntm_gru_forward_io(*w, k.H, k.I, k.O, L.ptr(x), L.ptr(y), B, T, x.stride(0), y.stride(0), L.ptr(hbuf), L.current_stream())
    else:
        rc = L.lib().ntm_gru_forward_ex(*w, k.H, L.ptr(x), L.ptr(y), B, T, x.stride(0), y.stride(0), L.ptr(hbuf), L.NTM_GRU_LAT, L.current_stream())
    assert rc == 0, L.lib().ntm_last_error()
    assert bool(torch.isnan(y[:B, T * k.O:]).all()) and bool(torch.isnan(y[B]).all()), (k.name, B, T, "wrote outside its y rows")
    if h is not None:
        assert bool((hbuf[B] == SENTINEL).all()), (k.name, B, T, "wrote behind h_state")
        h.copy_(hbuf[:B])
    return y[:B, :T * k.O]


def run(ntm, k, x, h0, T):
    """-> (y, final state) as device tensors; x (B, >= T * I) and h0 (B, H) on the device, h0 left alone."""
    h = h0.clone()
    y = fwd(ntm, k, x, T, h)
    return y, h


def _report(name, what, H, B, T, got, f64, e_ref):
    err = float(np.abs(got.astype(np.float64) - f64).max())
    unit = max(e_ref, C.ULP * float(np.abs(f64).max()))
    print(f"GRUERR {name}/{what} {H} {B} {T} {err:.3e} {e_ref:.3e} {err / unit:.2f}")
    return err, err / unit


def sweep(ntm, k, x, h0, ref, lengths, rows=None):
    """(a) and (b) for one batch: x, h0 numpy (B, ...); ref: the Ref of the rows `rows` of the batch (default: all of them, in
    order).  One run at T_max, then for every T a run of T samples and its continuation.  -> {"acc": [(T, what, err, ratio,
    gate_err)], "bits": [(T, what)] failures of (b), "y": {T: y (B, T * O) numpy}, "h": {T: final state}}."""
    B, Tm = x.shape[0], max(lengths)
    rows = list(range(B)) if rows is None else list(rows)
    xd, hd = dev(x), dev(h0)
    y_full, h_full = run(ntm, k, xd, hd, Tm)
    assert bool(torch.isfinite(y_full).all()) and bool(torch.isfinite(h_full).all())
    out = {"acc": [], "bits": [], "y": {}, "h": {}}
    for T in lengths:
        y, h = run(ntm, k, xd, hd, T)
        yn, hn = y.cpu().numpy(), h.cpu().numpy()
        out["y"][T], out["h"][T] = yn, hn
        for what, got, f64, f32, e in (("y", yn[rows], ref.y64[:, :T * k.O], ref.y32[:, :T * k.O], ref.e_y),
                                       ("h", hn[rows], ref.h64[T], ref.h32[T], ref.e_h)):
            err, ratio = _report(k.name, what, k.H, B, T, got, f64, e)
            out["acc"].append((T, what, err, ratio, float(np.abs(got - f32).max())))
        if not torch.equal(y, y_full[:, :T * k.O]):
            out["bits"].append((T, "prefix"))
        if T < Tm:
            h2 = h.clone()
            y2 = fwd(ntm, k, xd[:, T * k.I:], Tm - T, h2)
            if not torch.equal(y2, y_full[:, T * k.O:]):
                out["bits"].append((T, "continued y"))
            if not torch.equal(h2, h_full):
                out["bits"].append((T, "continued state"))
        elif not torch.equal(h, h_full):
            out["bits"].append((T, "state of two equal calls"))
    return out


def _assert_sweep(res, tag):
    assert not res["bits"], (tag, res["bits"])                              # (b)
    worst = max(res["acc"], key=lambda r: r[3])
    assert all(r[4] < C.GATE for r in res["acc"]), (tag, max(r[4] for r in res["acc"]))          # the project's gate
    assert worst[3] <= C.MARGIN, (tag, "T, what, err, ratio:", worst[:4])                       # (a)


# ---- (a) + (b): gru_small_kernel
@functools.lru_cache(maxsize=None)
def _kern(family, H, I=1, O=1):
    if family == "io":
        return Kern(f"io<{I},{O}>", C.random_sd(H, I, O), io=True)
    return Kern(C.kernel_of(H), C.random_sd(H))


@pytest.mark.parametrize("H", C.SMALL_H)
def test_small_accuracy_prefix_and_carry(ntm, H):
    x, h0, ref = C.small_ref(H)
    k = _kern("small", H)
    for B in C.small_batches(H):
        _assert_sweep(sweep(ntm, k, x[:B], h0[:B], ref.rows(slice(0, B)), C.TILE64_T), (k.name, H, B))


@pytest.mark.parametrize("H", C.WIDE_H)
def test_wide_accuracy_prefix_and_carry(ntm, H):
    x, h0, ref = C.wide_ref(H)
    k = _kern("wide", H)
    for B in C.wide_batches(H):
        _assert_sweep(sweep(ntm, k, x[:B], h0[:B], ref.rows(slice(0, B)), C.wide_lengths(H)), (k.name, H, B))


@pytest.mark.parametrize("H,I,O", C.IO_CASES)
def test_io_accuracy_prefix_and_carry(ntm, H, I, O):
    x, h0, ref = C.io_ref(H, I, O)
    k = _kern("io", H, I, O)
    for B in C.IO_B:
        _assert_sweep(sweep(ntm, k, x[:B], h0[:B], ref.rows(slice(0, B)), C.TILE64_T), (k.name, H, B))


# ---- (a) + (b): gru_lat_kernel
def _lat_rows():
    return tuple(sorted(set(range(max(C.LAT_SMALL_B))) | set(C.lat_big_rows(cus()))))


@functools.lru_cache(maxsize=None)
def _lat_kern(weights):
    return Kern(f"lat[{weights}]", C.lat_sd(weights))


@pytest.mark.parametrize("weights", C.LAT_WEIGHTS)
def test_lat_accuracy_prefix_and_carry_in_both_head_forms(ntm, weights):
    """B = 1 and 3: a fifth wave does the head (HEADW = true).  B = CUs + 1: the head rotates over the four waves (HEADW = false);
    rows 0, CUs / 2 and CUs against the oracle, every row for prefix and carry, and the first three rows -- the inputs of the
    B = 3 batch -- bit for bit against that batch: the head's arithmetic does not depend on the wave that evaluates it."""
    rows = _lat_rows()
    _, _, ref = C.lat_ref(weights, rows)
    assert max(ref.e_y, ref.e_h) <= C.E_REF_MAX                             # the rows of THIS device (the CPU test assumes 256 CUs)
    k = _lat_kern(weights)
    big = cus() + 1
    x, h0 = C.inputs("lat", C.H_LAT, big, max(C.LAT_T))
    res = {}
    for B in C.lat_batches(cus()):
        sel = list(range(B)) if B < big else list(C.lat_big_rows(cus()))
        res[B] = sweep(ntm, k, x[:B], h0[:B], ref.rows([rows.index(r) for r in sel]), C.LAT_T, rows=sel)
    for B in res:
        _assert_sweep(res[B], (k.name, B))
    for T in C.LAT_T:
        assert np.array_equal(res[big]["y"][T][:3], res[3]["y"][T]) and np.array_equal(res[big]["h"][T][:3], res[3]["h"][T]), T
        assert np.array_equal(res[3]["y"][T][:1], res[1]["y"][T]), T


def test_lat_replicas_against_fp64(ntm):
    """gru_lat_kernel<true, true> (R = 2 stacked models, two streams each) at T = 258 (finish() flushes the previous tile) and
    385 (the prefetch has run in the second tile): each replica against ITS fp64 reference, not its sibling instantiation."""
    L = ntm._lib
    sds = C.rep_sds()
    stacks = [dev(np.stack([sd[k] for sd in sds])) for k in C.KEYS]
    rows = _lat_rows()
    refs = [C.lat_ref(w, rows)[2].rows([0, 1]) for w in C.LAT_WEIGHTS]
    x1, h1 = C.inputs("lat", C.H_LAT, C.REP_BPER, max(C.LAT_T))
    B = C.REP_R * C.REP_BPER
    x, h0 = dev(np.concatenate([x1] * C.REP_R)), dev(np.concatenate([h1] * C.REP_R))
    for T in C.REP_T:
        y = torch.full((B + 1, T + Y_PAD), float("nan"), device="cuda")
        h = torch.full((B + 1, C.H_LAT), SENTINEL, device="cuda")
        h[:B] = h0
        rc = L.lib().ntm_gru_forward_replicas(*[L.ptr(s) for s in stacks], L.ptr(x), L.ptr(y), C.REP_R, C.REP_BPER, T, x.stride(0), y.stride(0),
                                              L.ptr(h), L.current_stream())
        assert rc == 0, L.lib().ntm_last_error()
        assert bool(torch.isnan(y[:B, T:]).all()) and bool(torch.isnan(y[B]).all()) and bool((h[B] == SENTINEL).all())
        yn, hn = y[:B, :T].cpu().numpy(), h[:B].cpu().numpy()
        for r, ref in enumerate(refs):
            sl = slice(r * C.REP_BPER, (r + 1) * C.REP_BPER)
            for what, got, f64, f32, e in (("y", yn[sl], ref.y64[:, :T], ref.y32[:, :T], ref.e_y), ("h", hn[sl], ref.h64[T], ref.h32[T], ref.e_h)):
                err, ratio = _report(f"lat<REP>[{C.LAT_WEIGHTS[r]}]", what, C.H_LAT, B, T, got, f64, e)
                assert float(np.abs(got - f32).max()) < C.GATE
                assert ratio <= C.MARGIN, (r, T, what, err, ratio)
            # and the bits of the single-model kernel on the replica's slice
            y1, hs = run(ntm, _lat_kern(C.LAT_WEIGHTS[r]), x[sl], h0[sl], T)
            assert torch.equal(y1, y[sl, :T]) and torch.equal(hs, h[sl])


# ---- (c) a stream does not see its neighbours
def _isolation(ntm, k, x, h0, T, rows=None):
    """Row r alone = row r in the batch = row r in a batch whose other rows are NaN (x and h0); one input tiled over all rows gives
    identical rows."""
    B = x.shape[0]
    xd, hd = dev(x), dev(h0)
    y, h = run(ntm, k, xd, hd, T)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(h).all())
    for r in (range(B) if rows is None else rows):
        y1, h1 = run(ntm, k, xd[r:r + 1], hd[r:r + 1], T)
        assert torch.equal(y1[0], y[r]) and torch.equal(h1[0], h[r]), (k.name, B, r, "alone")
        xn, hn = torch.full_like(xd, float("nan")), torch.full_like(hd, float("nan"))
        xn[r], hn[r] = xd[r], hd[r]
        yn, hn = run(ntm, k, xn, hn, T)
        assert torch.equal(yn[r], y[r]) and torch.equal(hn[r], h[r]), (k.name, B, r, "NaN neighbours")
        others = [i for i in range(B) if i != r]
        assert bool(torch.isnan(yn[others]).all()), (k.name, B, r)           # the neighbours did run on their NaN
    yt, ht = run(ntm, k, xd[:1].expand(B, -1).contiguous(), hd[:1].expand(B, -1).contiguous(), T)
    assert torch.equal(yt, y[:1].expand_as(yt)) and torch.equal(ht, h[:1].expand_as(ht)), (k.name, B, "tiled")


@pytest.mark.parametrize("H", C.SMALL_H)
def test_small_streams_do_not_see_their_wave_neighbours(ntm, H):
    x, h0, _ = C.small_ref(H)
    for B in C.small_batches(H):
        if B > 1:
            _isolation(ntm, _kern("small", H), x[:B], h0[:B], 65)


def test_wide_io_and_lat_streams_do_not_see_their_neighbours(ntm):
    x, h0, _ = C.wide_ref(96)
    _isolation(ntm, _kern("wide", 96), x, h0, 65)
    x, h0, _ = C.wide_ref(200)
    _isolation(ntm, _kern("wide", 200), x, h0, 65)
    H, I, O = C.IO_CASES[1]
    x, h0, _ = C.io_ref(H, I, O)
    _isolation(ntm, _kern("io", H, I, O), x, h0, 65)
    big = cus() + 1
    x, h0 = C.inputs("lat", C.H_LAT, big, 258)
    _isolation(ntm, _lat_kern("ckpt"), x[:3], h0[:3], 258)
    _isolation(ntm, _lat_kern("ckpt"), x, h0, 258, rows=C.lat_big_rows(cus()))


# ---- (d) the padding identity
@pytest.mark.parametrize("H,HP", C.PAD_PAIRS)
def test_the_padded_form_equals_the_unpadded_kernel_on_zero_padded_weights(ntm, H, HP):
    family = "small" if H < C.H_LAT else "wide"
    assert C.kernel_of(H).replace(",true", "") == C.kernel_of(HP)          # small<HP, true> against small<HP>; the same wide form
    kp, ku = Kern(C.kernel_of(H), C.random_sd(H)), Kern(C.kernel_of(HP) + " on padded weights", C.zero_padded(C.random_sd(H), HP))
    B = max(C.small_batches(H)) if family == "small" else max(C.WIDE_B)
    x, h0 = C.inputs(family, H, B, max(C.TILE64_T))
    xd = dev(x)
    for T in (2, 65, max(C.TILE64_T)):
        y, h = run(ntm, kp, xd, dev(h0), T)
        yu, hu = run(ntm, ku, xd, dev(C.zero_padded_state(h0, HP)), T)
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 1e-3
        assert np.array_equal(y.cpu().numpy(), yu.cpu().numpy()), (H, HP, T)
        assert np.array_equal(h.cpu().numpy(), hu[:, :H].cpu().numpy()), (H, HP, T)
        assert not hu[:, H:].cpu().numpy().any(), (H, HP, T)                # the padded units are exactly 0 at the end


# ---- (e) interfaces
def _interfaces(ntm, k, sd, x, h0, T):
    B = x.shape[0]
    xd, hd = dev(x[:, :T * k.I]), dev(h0)
    y, h = run(ntm, k, xd, hd, T)
    y2, h2 = run(ntm, k, xd, hd, T)
    assert torch.equal(y, y2) and torch.equal(h, h2)                          # two equal calls
    # an x row stride above T * I with NaN behind every row (the y stride is above T * O in every call of this file)
    xs = torch.full((B, T * k.I + X_PAD), float("nan"), device="cuda")
    xs[:, :T * k.I] = xd
    y3, h3 = run(ntm, k, xs, hd, T)
    assert torch.equal(y, y3) and torch.equal(h, h3)
    # NULL h_state is an all-zero h0
    yz, _ = run(ntm, k, xd, torch.zeros_like(hd), T)
    y0 = fwd(ntm, k, xd, T, None)
    assert torch.equal(y0, yz) and not torch.equal(yz, y)
    # NULL b_o is a zero bias
    sz = dict(sd)
    sz["output.bias"] = np.zeros_like(sd["output.bias"])
    kz = Kern(k.name + " zero bias", sz, io=k.io)
    yb, hb = run(ntm, kz, xd, hd, T)
    hn = hd.clone()
    yn = fwd(ntm, k, xd, T, hn, bias=False)
    assert torch.equal(yn, yb) and torch.equal(hn, hb) and torch.equal(hn, h) and not torch.equal(yb, y)


@pytest.mark.parametrize("family,H", [("small", 16), ("small", 5), ("small", 48), ("wide", 96), ("wide", 200)])
def test_interfaces_small_and_wide(ntm, family, H):
    x, h0, _ = (C.small_ref if family == "small" else C.wide_ref)(H)
    _interfaces(ntm, _kern(family, H), C.random_sd(H), x, h0, 65)


def test_interfaces_io(ntm):
    H, I, O = C.IO_CASES[1]
    x, h0, _ = C.io_ref(H, I, O)
    _interfaces(ntm, _kern("io", H, I, O), C.random_sd(H, I, O), x, h0, 65)


def test_interfaces_lat_in_both_head_forms(ntm):
    big = cus() + 1
    x, h0 = C.inputs("lat", C.H_LAT, big, 258)
    for B in (3, big):
        for T in (65, 258):
            _interfaces(ntm, _lat_kern("ckpt"), C.ckpt_sd(), x[:B], h0[:B], T)
