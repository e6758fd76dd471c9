"""GPU: the kernels of csrc/gru_train.hip at their step, stage and tile edges, through the raw ABI (tests/gru_train_cases.py holds the
references and the tables; tests/test_gru_train_cases_cpu.py proves them on the CPU).

  1. gru_train_bwd_kernel on CONSTRUCTED integer workspaces whose exact gradients are representable in fp32: equality on all
     12929 entries and dh0, at every length of the shared edge list (group loop, tail, ring start), with null dy / dh_T / dh0, padded
     rows, and through the `_replicas` entry.
  2. gru_train_fwd_kernel's workspace: the exact chain h_t = fma(z, fl(h_{t-1} - n), n) through every save slot, the saved gates
     against a float64 step from the saved h_{t-1}, NaN guards behind ws and between the rows of y, strides, null pointers, replicas.
  4. delay_bwd_kernel at L around its 2048-sample tile and D around its 256 owners: equality with an integer scatter for
     delays with weights 0, 1/2, 1; the float64 bar of tests/test_gpu_train_diffdel.py for the others.
(3., the module-level forward identity and gradients at the same lengths, are further cases of tests/test_gpu_train.py.)"""
import numpy as np
import pytest
import torch

import gru_train_cases as C

W_G = "GRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE]_BEST"
PKEYS = ["GRU.weight_ih_l0", "GRU.weight_hh_l0", "GRU.bias_ih_l0", "GRU.bias_hh_l0", "output.weight", "output.bias"]
NAN = float("nan")


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _padded(a, pad):
    """(B, T) -> device rows of T + pad floats, the padding NaN."""
    B, T = a.shape
    out = torch.full((B, T + pad), NAN, device="cuda")
    out[:, :T] = _dev(a)
    return out


# ---- 1. BPTT
def _bptt(ntm, w_hh, w_o, x, ws, dy, dh_T, *, want_dh0=True, pad=0, replicas=None):
    """ntm_gru_train_backward (or `_replicas` with replicas = (R, Bper)) and the reduction on top
    -> (part (B, 12929), dh0 (B, 64) or None, grad (R, 12929)) as numpy float32."""
    L, ptr, s = ntm._lib.lib(), ntm._lib.ptr, ntm._lib.current_stream()
    B, T = x.shape
    xd, dyd = _padded(x, pad), (None if dy is None else _padded(dy, pad))
    whd, wod, wsd, dhd = _dev(w_hh), _dev(w_o), _dev(ws), _dev(dh_T)
    assert wsd.numel() == B * T * C.NSAVE * C.H
    part = torch.full((B, C.NGRAD), NAN, device="cuda")
    dh0 = torch.full((B, C.H), NAN, device="cuda") if want_dh0 else None
    if replicas is None:
        ntm._lib.check(L.ntm_gru_train_backward(ptr(whd), ptr(wod), ptr(xd), T + pad, ptr(wsd), ptr(dyd), T + pad, ptr(dhd), B, T, ptr(dh0),
                                                ptr(part), s), "ntm_gru_train_backward")
        grad = torch.full((1, C.NGRAD), NAN, device="cuda")
        ntm._lib.check(L.ntm_gru_train_reduce(ptr(part), B, ptr(grad), s), "ntm_gru_train_reduce")
    else:
        R, Bper = replicas
        assert R * Bper == B and whd.shape == (R, 3 * C.H, C.H) and wod.shape == (R, C.H)
        ntm._lib.check(L.ntm_gru_train_backward_replicas(ptr(whd), ptr(wod), ptr(xd), T + pad, ptr(wsd), ptr(dyd), T + pad, ptr(dhd), R, Bper,
                                                         T, ptr(dh0), ptr(part), s), "ntm_gru_train_backward_replicas")
        grad = torch.full((R, C.NGRAD), NAN, device="cuda")
        ntm._lib.check(L.ntm_gru_train_reduce_replicas(ptr(part), R, Bper, ptr(grad), s), "ntm_gru_train_reduce_replicas")
    torch.cuda.synchronize()
    return part.cpu().numpy(), (None if dh0 is None else dh0.cpu().numpy()), grad.cpu().numpy()


def _same(got, want, what):
    bad = np.flatnonzero(~(got.reshape(-1) == want.reshape(-1)))
    assert bad.size == 0, (what, int(bad.size), [(int(i), float(got.reshape(-1)[i]), float(want.reshape(-1)[i])) for i in bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("family,T", C.BPTT_CASES)
def test_bptt_equals_the_exact_reference_on_constructed_workspaces(ntm, family, T):
    c = C.bptt_case(family, T)
    part_w, dh0_w, bd = C.bptt_expected(family, T)
    assert C.bounds_hold(bd)
    part, dh0, grad = _bptt(ntm, c["w_hh"], c["w_o"], c["x"], c["ws"], c["dy"], c["dh_T"])
    _same(part, part_w, "part")
    _same(dh0, dh0_w, "dh0")
    _same(grad, C.reduce_reference(part_w), "grad")
    # rows of T + 3 floats with NaN between them: the bits of the contiguous call
    part_p, dh0_p, grad_p = _bptt(ntm, c["w_hh"], c["w_o"], c["x"], c["ws"], c["dy"], c["dh_T"], pad=3)
    _same(part_p, part, "part, padded rows")
    _same(dh0_p, dh0, "dh0, padded rows")
    _same(grad_p, grad, "grad, padded rows")
    # dh0 null: the partials do not change
    part_n, none, _ = _bptt(ntm, c["w_hh"], c["w_o"], c["x"], c["ws"], c["dy"], c["dh_T"], want_dh0=False)
    assert none is None
    _same(part_n, part_w, "part, dh0 null")


@pytest.mark.gpu
@pytest.mark.parametrize("family,T", C.BPTT_CASES)
@pytest.mark.parametrize("null", ["dy", "dh_T"])
def test_bptt_with_a_null_dy_or_dh_T_equals_the_exact_reference(ntm, null, family, T):
    c = C.bptt_case(family, T)
    with_dy, with_dh = null != "dy", null != "dh_T"
    part_w, dh0_w, bd = C.bptt_expected(family, T, 3, 0, with_dy, with_dh)
    assert C.bounds_hold(bd)
    part, dh0, grad = _bptt(ntm, c["w_hh"], c["w_o"], c["x"], c["ws"], c["dy"] if with_dy else None, c["dh_T"] if with_dh else None)
    _same(part, part_w, "part")
    _same(dh0, dh0_w, "dh0")
    _same(grad, C.reduce_reference(part_w), "grad")


@pytest.mark.gpu
@pytest.mark.parametrize("family,T", [(f, T) for f in ("routing", "allgates") for T in C.BPTT_REPLICA_T if f == "routing" or T in C.ALLGATES_T])
def test_bptt_replicas_equal_every_replica_alone_and_the_exact_reference(ntm, family, T):
    R, Bper = C.BPTT_R, C.BPTT_BPER
    cs = [C.bptt_case(family, T, Bper, r + 1) for r in range(R)]
    cat = {k: (np.stack if k in ("w_hh", "w_o") else np.concatenate)([c[k] for c in cs]) for k in cs[0]}
    part, dh0, grad = _bptt(ntm, cat["w_hh"], cat["w_o"], cat["x"], cat["ws"], cat["dy"], cat["dh_T"], replicas=(R, Bper))
    for r, c in enumerate(cs):
        sl = slice(r * Bper, (r + 1) * Bper)
        part_w, dh0_w, bd = C.bptt_expected(family, T, Bper, r + 1)
        assert C.bounds_hold(bd)
        part_1, dh0_1, grad_1 = _bptt(ntm, c["w_hh"], c["w_o"], c["x"], c["ws"], c["dy"], c["dh_T"])
        _same(part[sl], part_1, f"part of replica {r} against the single call")
        _same(dh0[sl], dh0_1, f"dh0 of replica {r} against the single call")
        _same(grad[r], grad_1[0], f"grad of replica {r} against the single call")
        _same(part[sl], part_w, f"part of replica {r}")
        _same(dh0[sl], dh0_w, f"dh0 of replica {r}")
        _same(grad[r], C.reduce_reference(part_w)[0], f"grad of replica {r}")


# ---- 2. the forward's workspace
def _sd(ntm, wk, seed=77):
    if wk == "ckpt":
        return {k: np.asarray(v, np.float32) for k, v in ntm.weights.load_state_dict(W_G).items()}
    g = torch.Generator().manual_seed(seed)            # torch's init scale: U(-1/8, 1/8)
    shapes = {"GRU.weight_ih_l0": (192, 1), "GRU.weight_hh_l0": (192, 64), "GRU.bias_ih_l0": (192,), "GRU.bias_hh_l0": (192,),
              "output.weight": (1, 64), "output.bias": (1,)}
    return {n: ((torch.rand(*s, generator=g) * 2 - 1) / 8.0).float().numpy() for n, s in shapes.items()}


def _fwd_inputs(B, T, seed=0):
    g = torch.Generator().manual_seed(B * 7919 + T + seed)
    return (torch.rand(B, T, generator=g) - 0.5).numpy(), (0.5 * (torch.rand(B, C.H, generator=g) - 0.5)).numpy()


def _forward(ntm, sds, x, h0, *, x_pad=0, null_bo=False, replicas=None):
    """ntm_gru_train_forward (or `_replicas`) with NaN guards: C.WS_GUARD floats behind ws, y rows of T + C.Y_PAD.  h0 None: null
    h_state.  -> (ws (B, T, 5, 64), y (B, T), h_state or None) numpy float32, after the guards were found untouched."""
    L, ptr, s = ntm._lib.lib(), ntm._lib.ptr, ntm._lib.current_stream()
    B, T = x.shape
    stack = [_dev(np.stack([np.asarray(sd[k], np.float32).reshape(-1) for sd in sds])) for k in PKEYS]
    if null_bo:
        stack[5] = None
    xd = _padded(x, x_pad)
    yd = torch.full((B, T + C.Y_PAD), NAN, device="cuda")
    n = B * T * C.NSAVE * C.H
    assert n == L.ntm_gru_train_workspace_floats(B, T)
    wsd = torch.full((n + C.WS_GUARD,), NAN, device="cuda")
    hd = _dev(h0)
    args = [ptr(t) for t in stack] + [ptr(xd), ptr(yd)]
    if replicas is None:
        assert len(sds) == 1
        ntm._lib.check(L.ntm_gru_train_forward(*args, B, T, T + x_pad, T + C.Y_PAD, ptr(hd), ptr(wsd), s), "ntm_gru_train_forward")
    else:
        R, Bper = replicas
        assert R == len(sds) and R * Bper == B
        ntm._lib.check(L.ntm_gru_train_forward_replicas(*args, R, Bper, T, T + x_pad, T + C.Y_PAD, ptr(hd), ptr(wsd), s),
                       "ntm_gru_train_forward_replicas")
    torch.cuda.synchronize()
    assert bool(torch.isnan(wsd[n:]).all()), "the guard behind the workspace was written"
    assert bool(torch.isnan(yd[:, T:]).all()), "the padding between the rows of y was written"
    assert bool(torch.isfinite(wsd[:n]).all()) and bool(torch.isfinite(yd[:, :T]).all())
    return wsd[:n].reshape(B, T, C.NSAVE, C.H).cpu().numpy(), yd[:, :T].cpu().numpy(), (None if hd is None else hd.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("T", C.T_EDGES)
@pytest.mark.parametrize("B", C.FWD_B)
@pytest.mark.parametrize("wk", C.FWD_WEIGHTS)
def test_saved_workspace_chain_is_exact_and_the_gates_match_float64(ntm, wk, B, T):
    """Bar per quantity: 4 x the error of the plain-float32 twin against float64 over the case, with a floor of 2^-22 (r, z, n: exp2 and
    rcp are 1-ulp approximations, the tanh form is absolute to ~1 ulp of 1) or 2^-22 (sum |W_hn| |h| + |b_hn|) (gh_n).  Observed / bar
    is printed per case; the first run on an MI355X gave at most r 0.33, z 0.59, n 0.62, gh_n 0.32 over the 80 cases."""
    sd = _sd(ntm, wk)
    x, h0 = _fwd_inputs(B, T)
    ws, y, hT = _forward(ntm, [sd], x, h0)
    # the exact chain: row 0 of step 0 is h0, row 0 of step t + 1 (and the returned state) is fma(z, fl(h - n), n) of step t's rows
    nxt = C.chain_next_h(ws)
    _same(ws[:, 0, 0], h0, "h_{-1}")
    _same(ws[:, 1:, 0], nxt[:, :-1], "h_{t-1} of the next step")
    _same(hT, nxt[:, -1], "h_state")
    # the gates of every step from its saved h_{t-1}, float64 against the kernel and against plain float32
    r64, z64, n64, g64, cond = C.saved_gates(sd, ws[:, :, 0], x, np.float64)
    r32, z32, n32, g32, _ = C.saved_gates(sd, ws[:, :, 0], x, np.float32)
    ratios = {}
    for name, j, v64, v32, floor in (("r", 1, r64, r32, C.GATE_FLOOR), ("z", 2, z64, z32, C.GATE_FLOOR), ("n", 3, n64, n32, C.GATE_FLOOR),
                                     ("gh_n", 4, g64, g32, C.GATE_FLOOR * cond)):
        err = float(np.abs(ws[:, :, j].astype(np.float64) - v64).max())
        bar = max(C.GATE_MARGIN * float(np.abs(v32.astype(np.float64) - v64).max()), floor)
        ratios[name] = (err, bar)
    print(f"saved gates {wk} B={B} T={T}: " + "  ".join(f"{k} {e:.3g}/{b:.3g} = {e / b:.3f}" for k, (e, b) in ratios.items()))
    for name, (err, bar) in ratios.items():
        assert err <= bar, (name, err, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("T", C.T_EDGES)
def test_forward_strides_and_null_pointers(ntm, T):
    B = 3
    sd = _sd(ntm, "ckpt")
    x, h0 = _fwd_inputs(B, T, seed=1)
    ws, y, hT = _forward(ntm, [sd], x, h0)
    ws_p, y_p, hT_p = _forward(ntm, [sd], x, h0, x_pad=C.X_PAD)
    _same(ws_p, ws, "ws, padded x rows")
    _same(y_p, y, "y, padded x rows")
    _same(hT_p, hT, "h_state, padded x rows")
    # h_state null: a zero initial state
    zero = np.zeros_like(h0)
    ws_z, y_z, _ = _forward(ntm, [sd], x, zero)
    ws_n, y_n, none = _forward(ntm, [sd], x, None)
    assert none is None
    _same(ws_n, ws_z, "ws, h_state null")
    _same(y_n, y_z, "y, h_state null")
    assert not np.array_equal(ws_z, ws)
    # b_o null: a zero bias
    sd0 = dict(sd, **{"output.bias": np.zeros(1, np.float32)})
    assert float(np.abs(sd["output.bias"]).max()) > 0
    ws_b0, y_b0, hT_b0 = _forward(ntm, [sd0], x, h0)
    ws_bn, y_bn, hT_bn = _forward(ntm, [sd0], x, h0, null_bo=True)
    _same(ws_bn, ws_b0, "ws, b_o null")
    _same(y_bn, y_b0, "y, b_o null")
    _same(hT_bn, hT_b0, "h_state, b_o null")
    _same(ws_b0, ws, "ws does not depend on b_o")
    assert not np.array_equal(y_b0, y)


@pytest.mark.gpu
@pytest.mark.parametrize("T", C.FWD_REPLICA_T)
def test_forward_replicas_save_what_every_replica_alone_saves(ntm, T):
    R, Bper = 3, 2
    sds = [_sd(ntm, "rand", 1), _sd(ntm, "ckpt"), _sd(ntm, "rand", 2)]
    x, h0 = _fwd_inputs(R * Bper, T, seed=2)
    ws, y, hT = _forward(ntm, sds, x, h0, replicas=(R, Bper))
    for r, sd in enumerate(sds):
        sl = slice(r * Bper, (r + 1) * Bper)
        ws_1, y_1, hT_1 = _forward(ntm, [sd], x[sl], h0[sl])
        _same(ws[sl], ws_1, f"ws of replica {r}")
        _same(y[sl], y_1, f"y of replica {r}")
        _same(hT[sl], hT_1, f"h_state of replica {r}")


# ---- 4. the delay line's adjoint
def _delay(ntm, gy, d, gnb, L, D, need_gbuf, flags):
    L_, p = ntm._lib.lib(), ntm._lib.ptr
    B = C.DELAY_B
    gpre = torch.full((B, L), NAN, device="cuda")
    gbuf = torch.full((B, D), NAN, device="cuda") if need_gbuf else None
    ntm._lib.check(L_.ntm_delay_backward(p(gy), p(d), p(gnb), p(gpre), p(gbuf), B, L, D, 0, flags, ntm._lib.current_stream()),
                   "ntm_delay_backward")
    torch.cuda.synchronize()
    return gpre.cpu(), (None if gbuf is None else gbuf.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("L", C.DELAY_L)
@pytest.mark.parametrize("D", C.DELAY_D)
def test_delay_adjoint_equals_the_exact_scatter_for_weights_0_half_1(ntm, D, L):
    for kind in C.DELAY_EXACT_KINDS:
        d, gy, gnb = C.delay_exact_inputs(kind, L, D)
        dc, gyc, gnbc = d.cuda(), gy.float().cuda(), gnb.float().cuda()
        for with_gnb in (True, False):
            gpre_w, gbuf_w, top = C.delay_adjoint_exact(gy.numpy(), d.numpy(), gnb.numpy() if with_gnb else None, L, D)
            assert top < C.F24
            for need_gbuf in (True, False):
                for flags in (0, 1):
                    gpre, gbuf = _delay(ntm, gyc, dc, gnbc if with_gnb else None, L, D, need_gbuf, flags)
                    what = (kind, with_gnb, need_gbuf, flags)
                    _same(gpre.numpy(), gpre_w, ("gpre",) + what)
                    if need_gbuf:
                        _same(gbuf.numpy(), gbuf_w, ("gbuf",) + what)


@pytest.mark.gpu
@pytest.mark.parametrize("L", C.DELAY_L)
@pytest.mark.parametrize("D", C.DELAY_D)
@pytest.mark.parametrize("kind", C.DELAY_TOL_KINDS)
def test_delay_adjoint_against_float64_autograd_at_the_tile_edges(ntm, kind, D, L):
    """tests/test_gpu_train_diffdel.py's bar and its gather == scan equality, at these shapes."""
    from test_gpu_train_diffdel import delay_ref
    B = C.DELAY_B
    g = torch.Generator().manual_seed(7 * L + D + C.DELAY_TOL_KINDS.index(kind))
    d = C.delay_trajectory(kind, B, L, D, g)
    gy, gnb = torch.randn(B, L, generator=g), torch.randn(B, D, generator=g)
    grads = {}
    for dt in (torch.float64, torch.float32):
        pre = torch.zeros(B, L, dtype=dt, requires_grad=True)
        buf = torch.zeros(B, D, dtype=dt, requires_grad=True)
        y, nb = delay_ref(pre, buf, d, False)
        grads[dt] = torch.autograd.grad((y * gy.to(dt)).sum() + (nb * gnb.to(dt)).sum(), [pre, buf])
    dc, gyc, gnbc = d.cuda(), gy.cuda(), gnb.cuda()
    gpre, gbuf = _delay(ntm, gyc, dc, gnbc, L, D, True, 0)
    for name, got, r64, r32 in (("gpre", gpre, grads[torch.float64][0], grads[torch.float32][0]),
                                ("gbuf", gbuf, grads[torch.float64][1], grads[torch.float32][1])):
        a = got.double()
        assert torch.isfinite(a).all(), name
        err = float((a - r64).abs().max())
        bar = max(4 * float((r32.double() - r64).abs().max()), 2e-6 * float(r64.abs().max()), 1e-30)
        assert err <= bar, (name, err, bar)
    gpre_s, gbuf_s = _delay(ntm, gyc, dc, gnbc, L, D, True, 1)
    assert torch.equal(gpre, gpre_s) and torch.equal(gbuf, gbuf_s)
    gpre_n, none = _delay(ntm, gyc, dc, gnbc, L, D, False, 0)
    assert none is None and torch.equal(gpre_n, gpre)
