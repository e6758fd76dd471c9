"""CPU: the references and case tables of tests/gru_train_cases.py, which tests/test_gpu_gru_train_edges.py holds the kernels of
csrc/gru_train.hip to -- the coverage claims of the shared edge list, the exactness conditions of every constructed BPTT case,
the BPTT reference against float64 autograd, the single-rounding fma against Fraction, and the delay line's exact scatter against
float64 autograd of the delay restatement."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import gru_train_cases as C


def test_the_edge_list_covers_what_it_claims():
    T = C.T_EDGES
    assert T == tuple(sorted(set(T))) and max(T) <= 514
    assert {t % C.PF for t in T} == set(range(C.PF))                       # every tail length of the backward's group loop
    assert {t % C.PF for t in T if t > C.PF} == set(range(C.PF))           # ... behind at least one whole group
    assert set(range(1, C.PF)) <= set(T)                                   # T < PF: the ring starts with clamped fetches
    for edge in (C.SC, C.X_PREFETCH, C.LT):                                # both sides of a stage, of the x prefetch, of a tile
        assert {edge - 1, edge, edge + 1} <= set(T), edge
    assert {C.previous_y_tile_stored_by_finish(t) for t in T} == {None, True, False}
    assert C.previous_y_tile_stored_by_finish(C.LT + C.Y_DEFER) is True and C.previous_y_tile_stored_by_finish(C.LT + C.Y_DEFER + 1) is False
    assert {C.LT + C.Y_DEFER, C.LT + C.Y_DEFER + 1} <= set(T)
    assert any(t > 2 * C.LT for t in T)                                    # a third tile: the x / y buffers come round
    assert any(C.X_PREFETCH < t < C.LT for t in T)                         # the prefetch runs past the end of x (the zero fill)
    assert set(C.BPTT_REPLICA_T) <= set(T) and {t % C.PF for t in C.BPTT_REPLICA_T} >= {1, 2, 3}
    assert set(C.FWD_REPLICA_T) <= set(T)
    assert C.ALLGATES_T == tuple(range(1, 9))
    assert C.BPTT_CASES == [("routing", t) for t in T] + [("allgates", t) for t in range(1, 9)]


def _bptt_table():
    rows = [(f, T, 3, 0, dy, dh) for f, T in C.BPTT_CASES for dy, dh in ((True, True), (False, True), (True, False))]
    rows += [(f, T, C.BPTT_BPER, r + 1, True, True) for f in ("routing", "allgates") for T in C.BPTT_REPLICA_T
             if f == "routing" or T in C.ALLGATES_T for r in range(C.BPTT_R)]
    return rows


@pytest.mark.parametrize("family,T,B,seed,with_dy,with_dh", _bptt_table())
def test_every_constructed_bptt_case_is_exact_in_any_order(family, T, B, seed, with_dy, with_dh):
    c = C.bptt_case(family, T, B, seed)
    assert all(v.dtype == np.int64 for v in c.values())                    # the grid 2^-k with k = 0: inputs and, by closure, intermediates
    part, dh0, bd = C.bptt_expected(family, T, B, seed, with_dy, with_dh)
    assert C.bounds_hold(bd), bd
    assert part.dtype == np.float32 and part.shape == (B, C.NGRAD) and dh0.shape == (B, C.H)
    g = C.reduce_reference(part)
    assert np.array_equal(g.astype(np.float64), part.astype(np.float64).sum(0, keepdims=True))   # the reduction rounds nothing
    z, r, n = c["ws"][:, :, 2], c["ws"][:, :, 1], c["ws"][:, :, 3]
    if family == "routing":
        assert set(np.unique(z)) <= {0, 1} and set(np.unique(r)) <= {0, 1} and set(np.unique(n)) <= {-1, 0, 1}
        W = c["w_hh"].reshape(3, C.H, C.H)
        assert all((np.abs(W[g_]).sum(0) == 1).all() and (np.abs(W[g_]).sum(1) == 1).all() for g_ in range(3))
        assert np.count_nonzero(part[:, C.OFF_WHH + 2 * 4096:C.OFF_BIH]) > 0
        assert np.count_nonzero(dh0) > 0 or not (with_dy or T <= 2 * C.PF)      # without dy, dh_T has died out over a long window
    else:
        assert set(np.unique(z)) == set(np.unique(r)) == set(np.unique(n)) == {-1, 0, 1, 2}
        blocks = [part[:, C.OFF_WHH + g_ * 4096:C.OFF_WHH + (g_ + 1) * 4096] for g_ in range(3)]
        assert all(np.count_nonzero(b) > 100 for b in blocks) and np.count_nonzero(dh0) > C.H // 2
        assert all(np.count_nonzero(part[:, o:o + 192]) > 0 for o in (0, C.OFF_BIH, C.OFF_BHH))
        assert not with_dy or np.count_nonzero(part[:, C.OFF_WO:C.OFF_BO]) > 0


def test_the_routing_family_carries_a_long_recurrence():
    """dh at the start of a long window still depends on the last steps' dy: zeroing dy over the last PF steps changes dh0."""
    chains = 0
    for T in (7, 33):
        c = C.routing_case(T)
        dy = c["dy"].copy()
        dy[:, -1] = 0
        a = C.bptt_reference(c["w_hh"], c["w_o"], c["x"], c["ws"], c["dy"], None)[1]
        b = C.bptt_reference(c["w_hh"], c["w_o"], c["x"], c["ws"], dy, None)[1]
        chains += int(not np.array_equal(a, b))
    assert chains >= 1


def _random_sd(seed, scale=1.0):
    from test_gpu_train import _random_sd as f
    return f(seed, scale)


@pytest.mark.parametrize("B,T,with_dy,with_dh", [(2, 1, True, True), (3, 7, True, True), (2, 33, True, False), (2, 33, False, True)])
def test_the_bptt_reference_is_the_adjoint_of_torchs_gru(B, T, with_dy, with_dh):
    from test_gpu_train import _torch_grads
    sd = _random_sd(5 + T)
    g = torch.Generator().manual_seed(T)
    x = torch.rand(B, 1, T, generator=g, dtype=torch.float64) - 0.5
    h0 = 0.5 * (torch.rand(1, B, 64, generator=g, dtype=torch.float64) - 0.5)
    dy = torch.randn(B, T, generator=g, dtype=torch.float64) if with_dy else None
    dh = torch.randn(1, B, 64, generator=g, dtype=torch.float64) if with_dh else None
    want = _torch_grads(sd, x, h0, dy, dh, torch.float64)
    ws = C.gru_forward_f64(sd, x[:, 0].numpy(), h0[0].numpy())
    part, dh0, _ = C.bptt_reference(np.asarray(sd["GRU.weight_hh_l0"], np.float64), np.asarray(sd["output.weight"], np.float64).reshape(-1),
                                    x[:, 0].numpy(), ws, None if dy is None else dy.numpy(), None if dh is None else dh[0].numpy())
    got = part.sum(0)
    cuts = [(0, 192), (C.OFF_WHH, C.OFF_BIH), (C.OFF_BIH, C.OFF_BHH), (C.OFF_BHH, C.OFF_WO), (C.OFF_WO, C.OFF_BO), (C.OFF_BO, C.NGRAD)]
    for (a, b), w in zip(cuts, want[:6]):
        w = w.numpy().reshape(-1)
        assert np.abs(got[a:b] - w).max() <= 1e-12 * max(np.abs(w).max(), 1e-300), (a, b)
        assert with_dy or a >= C.OFF_WO or np.abs(w).max() > 0
    w = want[6].numpy()[0]
    assert np.abs(dh0 - w).max() <= 1e-12 * np.abs(w).max()


# ---- the single-rounding fma
def _exact_fma32(a, b, c):
    """Fraction -> float32, rounded once: float64 of a Fraction is correctly rounded, so round by hand on the float32 grid."""
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        return np.float32(0.0)
    lo = np.float32(float(v))                                              # within one float32 ulp of v: pick among it and its neighbours
    cands = sorted({float(np.nextafter(lo, np.float32(-np.inf))), float(lo), float(np.nextafter(lo, np.float32(np.inf)))})
    best = min(cands, key=lambda f: (abs(Fraction(f) - v), int(np.float32(f).view(np.uint32)) & 1))
    return np.float32(best)


def _near_ties():
    """z d + n a hair off a float32 tie: the exact product (1 + 2^-23)(1 - 2^-23) 2^m = 2^m (1 - 2^-46) against n = 2^(m+24) (1 +
    j 2^-23): n + 2^m is half-way between two float32, the true sum lies 2^(m-46) below it -- far less than half a float64 ulp of
    n, so a float64 round-to-nearest lands ON the tie and then goes to even, which is wrong for every odd j."""
    a, b, c = [], [], []
    for m in (-30, -8, 0, 5, 17):
        for j in (1, 2, 3, 5, 8388607):
            for sp in (1.0, -1.0):
                for sn in (1.0, -1.0):
                    a.append(np.float32(sp * 2.0 ** m * (1 + 2.0 ** -23)))
                    b.append(np.float32(1 - 2.0 ** -23))
                    c.append(np.float32(sn * 2.0 ** (m + 24) * (1 + j * 2.0 ** -23)))
    return np.array(a, np.float32), np.array(b, np.float32), np.array(c, np.float32)


def test_fma32_rounds_once():
    rng = np.random.default_rng(3)
    n = 3000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c[: n // 3] = -(a[: n // 3] * b[: n // 3])                             # cancellation: the result is the product's rounding error
    c[n // 3: n // 2] = (a * b)[n // 3: n // 2] * np.float32(2.0 ** 24)     # the product sits at half an ulp of c
    ta, tb, tc = _near_ties()
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    want = np.array([_exact_fma32(*v) for v in zip(a, b, c)], np.float32)
    got = C.fma32(a, b, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the constructed near-ties do tell a double rounding apart
    naive = C.fma32_naive(ta, tb, tc)
    assert (naive != C.fma32(ta, tb, tc)).sum() >= len(ta) // 2
    # in the forward's range (z in (0, 1), h and n in (-1, 1)) as chain_next_h calls it
    z, hp, nn = rng.random(2000).astype(np.float32), (2 * rng.random(2000) - 1).astype(np.float32), (2 * rng.random(2000) - 1).astype(np.float32)
    ws = np.zeros((2000, C.NSAVE, 1), np.float32)
    ws[:, 0, 0], ws[:, 2, 0], ws[:, 3, 0] = hp, z, nn
    want = np.array([_exact_fma32(zz, np.float32(h - m), m) for zz, h, m in zip(z, hp, nn)], np.float32)
    assert np.array_equal(C.chain_next_h(ws)[:, 0], want)


def test_saved_gates_in_float64_are_the_forward_reference_and_the_float32_twin_is_close():
    sd = _random_sd(11)
    rng = np.random.default_rng(0)
    x, h0 = rng.random((3, 40)) - 0.5, 0.5 * (rng.random((3, 64)) - 0.5)
    ws = C.gru_forward_f64(sd, x, h0)
    r, z, n, gh, cond = C.saved_gates(sd, ws[:, :, 0], x, np.float64)
    w32 = {k: torch.as_tensor(v).float() for k, v in sd.items()}
    assert all(torch.equal(w32[k], torch.as_tensor(sd[k])) for k in sd)       # the weights are float32 already: both read the same
    for j, v in enumerate((r, z, n, gh), start=1):
        assert np.abs(v - ws[:, :, j]).max() <= 1e-15 * max(1.0, np.abs(v).max())
    assert np.abs(ws[:, 1:, 0] - (n + z * (ws[:, :, 0] - n))[:, :-1]).max() < 1e-15
    r32, z32, n32, gh32, _ = C.saved_gates(sd, ws[:, :, 0].astype(np.float32), x.astype(np.float32), np.float32)
    for a, b in ((r32, r), (z32, z), (n32, n), (gh32, gh)):
        assert a.dtype == np.float32 and np.abs(a - b).max() < 1e-5
    assert 0 < cond < 64


# ---- the delay line's adjoint
@pytest.mark.parametrize("L", C.DELAY_L)
@pytest.mark.parametrize("D", C.DELAY_D)
@pytest.mark.parametrize("kind", C.DELAY_EXACT_KINDS)
def test_the_exact_delay_scatter_is_the_adjoint_of_the_delay_line(kind, D, L):
    from test_gpu_train_diffdel import delay_ref
    d, gy, gnb = C.delay_exact_inputs(kind, L, D)
    assert d.dtype == torch.float32 and d.shape == (C.DELAY_B, L)
    assert torch.equal(2 * d, torch.round(2 * d)) and float(d.min()) >= 0 and float(d.max()) <= D      # weights 0, 1/2, 1 in float32 too
    if kind == "half":
        assert bool(((d - torch.floor(d)) == 0.5).any()) or D == 0
    for with_gnb in (True, False):
        pre = torch.zeros(C.DELAY_B, L, dtype=torch.float64, requires_grad=True)
        buf = torch.zeros(C.DELAY_B, D, dtype=torch.float64, requires_grad=True)
        y, nb = delay_ref(pre, buf, d, False)
        loss = (y * gy.double()).sum() + ((nb * gnb.double()).sum() if with_gnb else 0.0)
        gs = torch.autograd.grad(loss, [pre, buf], allow_unused=True)
        want = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, (pre, buf))]
        gpre, gbuf, top = C.delay_adjoint_exact(gy.numpy(), d.numpy(), gnb.numpy() if with_gnb else None, L, D)
        assert top < C.F24                                                 # every partial sum of a target is exact in float32
        assert np.array_equal(gpre.astype(np.float64), want[0].numpy()) and np.array_equal(gbuf.astype(np.float64), want[1].numpy())


def test_the_delay_table_sits_on_the_kernels_tile_and_ownership_edges():
    DB_T, DB_NT = 256, 2048          # gru_train.hip `constexpr int DB_T = 256, DB_NT = 2048`
    assert {DB_NT - 1, DB_NT, DB_NT + 1, 2 * DB_NT + 1, 1, 2} == set(C.DELAY_L)
    assert {DB_T - 1, DB_T, DB_T + 1, 1} == set(C.DELAY_D)


def test_the_backward_pairs_every_ring_slot_with_its_lds_parity():
    """The one property of gru_train_bwd_kernel that no value can show: the parity of ab[] only keeps a step's LDS reads apart from
    the next step's writes, and with one workgroup per CU the waves leave the barrier together, so a step on the wrong parity
    computes the same bits (measured: such a build passes every test of this suite).  Held on the source instead: every call
    step(j, t - j, P) of the kernel has P = j mod 2, in the group loop and in the tail."""
    import os
    import re

    from helpers import ROOT
    with open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "gru_train.hip")) as f:
        src = f.read()
    body = src[src.index("void gru_train_bwd_kernel"):src.index("float *ps = part + s * NGRAD;")]
    calls = [(int(j), off, int(p)) for j, off, p in re.findall(r"\bstep\((\d), t((?: - \d)?), P([01])\{\}\)", body)]
    assert [j for j, _, _ in calls] == list(range(C.PF)) + list(range(C.PF - 1)), calls
    assert all(off == (f" - {j}" if j else "") and p == j % 2 for j, off, p in calls), calls
    assert body.count("step(") == len(calls)                              # no call escaped the pattern
