"""Case tables and references for the edge tests of csrc/gru_train.hip (tests/test_gpu_gru_train_edges.py; the tables are
checked and the references pinned on the CPU by tests/test_gru_train_cases_cpu.py).

  * bptt_reference: the recurrence of gru_train_bwd_kernel's header comment in numpy int64 (exact) or float64, and the
    fixed-order reduction on top of it.  The two case families (routing_case, allgates_case) hand it -- and the kernel --
    a CONSTRUCTED workspace of small integers, for which every sum the kernel forms is exact in fp32 whatever its order.
  * fma32 and saved_gates: the forward's saved workspace -- the exact chain h_t = fma(z, fl(h_{t-1} - n), n) and a single
    GRU step from the saved h_{t-1} in float64 / float32.
  * delay_adjoint_exact: the scatter of delay_bwd_kernel in integers (half units), for delays with weights 0, 1/2, 1."""
import functools

import numpy as np

H = 64
NSAVE = 5                                # ws[s][t][j][u], j = h_{t-1}, r, z, n, gh_n          (gru_train.hip: NSAVE)
OFF_WHH, OFF_BIH, OFF_BHH, OFF_WO, OFF_BO = 192, 192 + 12288, 192 + 12288 + 192, 192 + 12288 + 384, 192 + 12288 + 384 + 64
NGRAD = OFF_BO + 1                       # w_ih | w_hh | b_ih | b_hh | w_o | b_o                  (gru_train.hip: NGRAD)
assert NGRAD == 12929

# ---- the constants behind the shared edge list, each the mirror of one line of the kernels
PF = 4              # gru_train.hip `constexpr int PF = 4`: the backward's register ring / steps per group of its time loop
SC = 32             # gru_train.hip `constexpr int SC = 32`: steps per LDS stage of the forward's saves
X_PREFETCH = 128    # gru_train.hip `if (c0 == 128 && tid < LT)`: the stage at which the forward loads the next x tile
LT = 256            # gru_lat_step.h `constexpr int LT = 256`: samples per x / y tile
Y_DEFER = 2         # gru_train.hip `if (ns > 2 && tile0 >= LT ...)` and gru_lat_step.h finish() `(T - 1 - last0) < 2`: a last
#                     tile of at most Y_DEFER samples leaves the previous y tile to finish()
T_EDGES = (1, 2, 3, 4, 6, 7, 8, 31, 32, 33, 127, 128, 129, 255, 256, 257, 258, 259, 513, 514)

F24, F53 = 1 << 24, 1 << 53


def previous_y_tile_stored_by_finish(T):
    """True / False: which of the two places writes the y tile before the last one (None: there is none)."""
    last0 = (T - 1) // LT * LT
    if last0 < LT:
        return None
    return (T - 1 - last0) < Y_DEFER


# ---- 1. BPTT
def bptt_reference(w_hh, w_o, x, ws, dy, dh_T):
    """gru_train_bwd_kernel per stream, t = T-1 .. 0, for unit k (W[g][u][k] = w_hh[g*64 + u][k]):
        g = w_o dy_t + dh;  a_n = g (1 - z)(1 - n^2);  a_z = g (h_{t-1} - n) z (1 - z);  a_r = a_n gh_n r (1 - r);  a_nh = a_n r;
        dh_{t-1}[k] = g z + sum_u W_r[u][k] a_r[u] + W_z[u][k] a_z[u] + W_n[u][k] a_nh[u];   dW_g[u][k] += a_g[u] h_{t-1}[k];
        d w_ih += (a_r, a_z, a_n) x_t;  d b_ih += (a_r, a_z, a_n);  d b_hh += (a_r, a_z, a_nh);  d w_o += dy_t h_t;  d b_o += dy_t
    with h_t = z (h_{t-1} - n) + n.  All arrays int64 (exact; bounds are tracked) or all float64 (the adjoint as such).
    w_hh (192, 64), w_o (64,), x (B, T), ws (B, T, 5, 64), dy (B, T) or None, dh_T (B, 64) or None
    -> (part (B, 12929), dh0 (B, 64), bounds): part and dh0 in the arrays' dtype;  bounds (int64 only) = the largest of
         elem: |any elementwise intermediate|            sum32: sum of |terms| of any fp32 sum (p0 + p1 + quad, g, dh, h_t)
         acc32: sum over t of |terms| of a dW_hh entry   acc64: the same of the nine fp64 accumulators."""
    exact = ws.dtype == np.int64
    assert all(a is None or a.dtype == ws.dtype for a in (w_hh, w_o, x, dy, dh_T))
    B, T = x.shape
    W = w_hh.reshape(3, H, H)
    Wabs = np.abs(W)
    dh = np.zeros((B, H), ws.dtype) if dh_T is None else dh_T.copy()
    dW, dWabs = np.zeros((B, 3, H, H), ws.dtype), np.zeros((B, 3, H, H), ws.dtype)
    acc = np.zeros((9, B, H), ws.dtype)                  # dwir dwiz dwin dbr dbz dbin dbhn dwo | dbo (unit 0 only)
    accabs = np.zeros_like(acc)
    bd = {"elem": 0, "sum32": 0, "acc32": 0, "acc64": 0}

    def note(key, *vals):
        if exact:
            bd[key] = max([bd[key]] + [int(np.abs(v).max()) for v in vals])

    for t in range(T - 1, -1, -1):
        hp, r, z, n, ghn = (ws[:, t, j] for j in range(NSAVE))
        xv = x[:, t, None]
        dyv = np.zeros((B, 1), ws.dtype) if dy is None else dy[:, t, None]
        wd = w_o[None] * dyv
        g = wd + dh
        omz, hmn, nn, omr = 1 - z, hp - n, n * n, 1 - r
        dn, dz, omn2, zz, rr = g * omz, g * hmn, 1 - nn, z * omz, r * omr
        an, az = dn * omn2, dz * zz
        agh = an * ghn
        ar, anh = agh * rr, an * r
        zh = z * hmn
        ht = zh + n
        a = np.stack([ar, az, anh], 1)                                    # (B, 3, u)
        q = np.einsum("guk,bgu->bk", W, a)
        gz = g * z
        terms = np.stack([ar * xv, az * xv, an * xv, ar, az, an, anh, dyv * ht, np.broadcast_to(dyv, (B, H))])
        if exact:
            qabs = np.einsum("guk,bgu->bk", Wabs, np.abs(a))
            note("elem", hp, r, z, n, ghn, xv, dyv, wd, g, omz, hmn, nn, omr, dn, dz, omn2, zz, rr, an, az, agh, ar, anh, zh, ht, gz, q)
            note("sum32", np.abs(wd) + np.abs(dh), qabs, np.abs(gz) + qabs, np.abs(zh) + np.abs(n))
            dWabs += np.abs(a)[:, :, :, None] * np.abs(hp)[:, None, None, :]
            accabs += np.abs(terms)
        dW += a[:, :, :, None] * hp[:, None, None, :]
        acc += terms
        dh = gz + q
    note("acc32", dWabs)
    note("acc64", accabs)
    part = np.zeros((B, NGRAD), ws.dtype)
    part[:, 0:192] = np.concatenate([acc[0], acc[1], acc[2]], 1)
    part[:, OFF_WHH:OFF_BIH] = dW.reshape(B, -1)
    part[:, OFF_BIH:OFF_BHH] = np.concatenate([acc[3], acc[4], acc[5]], 1)
    part[:, OFF_BHH:OFF_WO] = np.concatenate([acc[3], acc[4], acc[6]], 1)
    part[:, OFF_WO:OFF_BO] = acc[7]
    part[:, OFF_BO] = acc[8][:, 0]
    return part, dh, bd


def bounds_hold(bd):
    """The exactness condition on the integer grid (2^-k with k = 0): every fp32 value and every fp32 sum's absolute terms
    stay below 2^24, every fp64 accumulator's below 2^53 -- then any order of evaluation gives the same bits."""
    return max(bd["elem"], bd["sum32"], bd["acc32"]) < F24 and bd["acc64"] < F53


def reduce_reference(part32, bper=None):
    """ntm_gru_train_reduce(_replicas) on float32 partials: the streams of each model added in fp64 (exact here), then rounded."""
    B = part32.shape[0]
    bper = B if bper is None else bper
    assert part32.dtype == np.float32 and B % bper == 0
    s = part32.astype(np.float64).reshape(B // bper, bper, -1).sum(1)
    return s.astype(np.float32)


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape).astype(np.int64)


def _choice(rng, shape, values, p):
    return rng.choice(np.asarray(values, np.int64), size=shape, p=p)


def _signed_perm(rng):
    m = np.zeros((H, H), np.int64)
    m[np.arange(H), rng.permutation(H)] = rng.choice([-1, 1], H)
    return m


@functools.lru_cache(maxsize=None)
def routing_case(T, B=3, seed=0):
    """Routing family: saved z, r in {0, 1} and n in {-1, 0, 1} make a_z = a_r = 0, every gate block of W_hh is a signed
    permutation, so dh is only routed (through g z and W_hn^T a_nh) and sum_k |dh[k]| grows by at most sum_k |w_o[k] dy_t| per
    step: linearly in T.  dy is sparse so that the dW_hh accumulators stay below 2^24 at T = 514."""
    rng = np.random.default_rng(1000 * T + seed)
    ws = np.stack([_ints(rng, (B, T, H), -2, 2), _choice(rng, (B, T, H), (0, 1), (0.2, 0.8)), _choice(rng, (B, T, H), (0, 1), (0.15, 0.85)),
                   _choice(rng, (B, T, H), (-1, 0, 1), (0.2, 0.6, 0.2)), _ints(rng, (B, T, H), -2, 2)], 2)
    dy = _choice(rng, (B, T), (-2, -1, 0, 1, 2), (0.05, 0.1, 0.7, 0.1, 0.05))
    dy[:, -1] = rng.choice([-2, -1, 1, 2], B)                              # the first step of the walk always has a dy
    return {"w_hh": np.concatenate([_signed_perm(rng) for _ in range(3)]), "w_o": _ints(rng, (H,), -2, 2), "x": _ints(rng, (B, T), -2, 2),
            "ws": ws, "dy": dy, "dh_T": _ints(rng, (B, H), -2, 2)}


ALLGATES_T = tuple(range(1, 9))


@functools.lru_cache(maxsize=None)
def allgates_case(T, B=3, seed=0):
    """All-gates family: saved z, r, n in {-1, 0, 1, 2} -- outside the activations' range, so that 1 - z, z (1 - z), 1 - n^2 and
    r (1 - r) are non-zero integers -- and a sparse W_hh in {0, +-1}: every term of a_r, a_z, a_nh, all three W^T a products and
    all three dW_hh blocks is live.  The values grow geometrically, hence T <= 8 and mostly in-range entries."""
    rng = np.random.default_rng(7000 + 10 * T + seed)
    gate = lambda: _choice(rng, (B, T, H), (-1, 0, 1, 2), (0.1, 0.4, 0.4, 0.1))      # noqa: E731
    ws = np.stack([_ints(rng, (B, T, H), -2, 2), gate(), gate(), _choice(rng, (B, T, H), (-1, 0, 1, 2), (0.2, 0.55, 0.2, 0.05)),
                   _ints(rng, (B, T, H), -2, 2)], 2)
    w_hh = _choice(rng, (3 * H, H), (-1, 0, 1), (0.03, 0.94, 0.03))
    return {"w_hh": w_hh, "w_o": _ints(rng, (H,), -2, 2), "x": _ints(rng, (B, T), -2, 2), "ws": ws,
            "dy": _ints(rng, (B, T), -2, 2), "dh_T": _ints(rng, (B, H), -2, 2)}


BPTT_CASES = [("routing", T) for T in T_EDGES] + [("allgates", T) for T in ALLGATES_T]
BPTT_REPLICA_T = (2, 3, 6, 7, 33)       # through the `_replicas` entry, (R, Bper) = (3, 2)
BPTT_R, BPTT_BPER = 3, 2


def bptt_case(family, T, B=3, seed=0):
    return (routing_case if family == "routing" else allgates_case)(T, B, seed)


@functools.lru_cache(maxsize=None)
def bptt_expected(family, T, B=3, seed=0, with_dy=True, with_dh=True):
    """-> (part float32 (B, 12929), dh0 float32 (B, 64), bounds) of the case, dy / dh_T null on request."""
    c = bptt_case(family, T, B, seed)
    part, dh0, bd = bptt_reference(c["w_hh"], c["w_o"], c["x"], c["ws"], c["dy"] if with_dy else None, c["dh_T"] if with_dh else None)
    return part.astype(np.float32), dh0.astype(np.float32), bd


# ---- 2. the forward's workspace
def fma32(a, b, c):
    """fl32(a * b + c) of float32 arrays, rounded ONCE.  The product of two float32 is exact in float64; the float64 sum is
    rounded to odd (TwoSum gives its error: if the sum is inexact and its last bit even, step to the neighbour on the error's
    side), and a round-to-odd value of 53 bits rounds to 24 bits as the exact sum does (53 >= 24 + 2).  No intermediate
    round-to-nearest in float64, which would break ties the exact value does not have."""
    a, b, c = (np.asarray(v) for v in (a, b, c))
    assert a.dtype == b.dtype == c.dtype == np.float32
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                                        # s + e = p + c exactly
    odd = (s.view(np.int64) & 1) == 1
    fix = (e != 0) & ~odd
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def fma32_naive(a, b, c):
    """The same through a float64 round-to-nearest: wrong on near-ties (the CPU test shows that its cases tell the two apart)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def chain_next_h(ws):
    """h_t for every saved step from the saved rows alone, as the kernel forms `hold`: fma(z, fl(h_{t-1} - n), n)."""
    hp, z, n = ws[..., 0, :], ws[..., 2, :], ws[..., 3, :]
    return fma32(z, hp - n, n)


def saved_gates(sd, hp, x, dtype):
    """One GRU step per (s, t) from the saved h_{t-1} (B, T, 64) and x (B, T), float32 weights, arithmetic in `dtype`
    (np.float64, or np.float32 for the plain-float32 twin) -> (r, z, n, gh_n (unscaled: W_hn h + b_hn), cond) with
    cond = max over everything of sum |W_hn| |h| + |b_hn|."""
    w_ih = np.asarray(sd["GRU.weight_ih_l0"], np.float32).reshape(3, H).astype(dtype)
    w_hh = np.asarray(sd["GRU.weight_hh_l0"], np.float32).reshape(3, H, H).astype(dtype)
    b_ih = np.asarray(sd["GRU.bias_ih_l0"], np.float32).reshape(3, H).astype(dtype)
    b_hh = np.asarray(sd["GRU.bias_hh_l0"], np.float32).reshape(3, H).astype(dtype)
    hp, x = hp.astype(dtype), x.astype(dtype)[..., None]
    gh = [hp @ w_hh[g].T + b_hh[g] for g in range(3)]
    gi = [x * w_ih[g] + b_ih[g] for g in range(3)]
    one = dtype(1.0)
    r = one / (one + np.exp(-(gi[0] + gh[0])))
    z = one / (one + np.exp(-(gi[1] + gh[1])))
    n = np.tanh(gi[2] + r * gh[2])
    cond = float((np.abs(hp).astype(np.float64) @ np.abs(w_hh[2]).astype(np.float64).T + np.abs(b_hh[2]).astype(np.float64)).max())
    assert all(v.dtype == dtype for v in (r, z, n, gh[2]))
    return r, z, n, gh[2], cond


GATE_MARGIN = 4                          # the project's margin on the float32 twin's own error
GATE_FLOOR = 2.0 ** -22                  # exp2 and rcp are 1-ulp approximations, the tanh form is absolute to ~1 ulp of 1
FWD_B = (1, 3)
FWD_WEIGHTS = ("ckpt", "rand")
FWD_REPLICA_T = (2, 33, 257)
WS_GUARD = 1024                          # NaN floats behind the workspace
Y_PAD, X_PAD = 5, 3                      # y_stride_b = T + 5, x_stride_b = T + 3


def gru_forward_f64(sd, x, h0):
    """float64 GRU forward (torch's definition) -> ws (B, T, 5, 64) float64 and y (B, T): in-range saved values for the
    adjoint check of bptt_reference."""
    w_ih, w_hh = np.asarray(sd["GRU.weight_ih_l0"], np.float64).reshape(3, H), np.asarray(sd["GRU.weight_hh_l0"], np.float64).reshape(3, H, H)
    b_ih, b_hh = np.asarray(sd["GRU.bias_ih_l0"], np.float64).reshape(3, H), np.asarray(sd["GRU.bias_hh_l0"], np.float64).reshape(3, H)
    B, T = x.shape
    ws = np.zeros((B, T, NSAVE, H))
    h = np.asarray(h0, np.float64).copy()
    for t in range(T):
        gh = [h @ w_hh[g].T + b_hh[g] for g in range(3)]
        gi = [x[:, t, None] * w_ih[g] + b_ih[g] for g in range(3)]
        r = 1.0 / (1.0 + np.exp(-(gi[0] + gh[0])))
        z = 1.0 / (1.0 + np.exp(-(gi[1] + gh[1])))
        n = np.tanh(gi[2] + r * gh[2])
        ws[:, t] = np.stack([h, r, z, n, gh[2]], 1)
        h = n + z * (h - n)
    return ws


# ---- 4. the delay line's adjoint
DELAY_B = 2
DELAY_L = (1, 2, 2047, 2048, 2049, 4097)         # DB_NT = 2048 samples per tile
DELAY_D = (1, 255, 256, 257)                     # DB_T = 256 owners
DELAY_EXACT_KINDS = ("whole", "zero", "at_D", "half")
DELAY_TOL_KINDS = ("random", "rising")


def delay_trajectory(kind, B, L, D, g):
    """tests/test_gpu_train_diffdel.py's trajectories, and `half`: delays k + 0.5 clipped to [0, D] (weights 1/2 and 1/2)."""
    import torch
    if kind == "half":
        k = torch.randint(0, D + 1, (B, L // 16 + 1), generator=g).double().repeat_interleave(16, dim=1)[:, :L]
        return (k + 0.5).clamp(0, D).float().contiguous()
    from test_gpu_train_diffdel import trajectory
    return trajectory(kind, B, L, D, g)


def delay_adjoint_exact(gy, d, gnb, L, D):
    """delay_bwd_kernel's scatter in int64 HALF units for integer gy (B, L), g_newbuf (B, D) or None, and float32 delays whose
    weights 1 - |m - d| are 0, 1/2 or 1:  gz[i] = g_newbuf[i - L] (i >= L) + sum of w_m(n) gy[n] over D + n - m = i, for the
    taps m in {k + 1, k}, k = floor(d[n]), with 0 <= m <= D and w > 0.
    -> (gpre (B, L) float32, gbuf (B, D) float32, the largest sum of |terms| of a target in half units)."""
    gy, d = np.asarray(gy, np.int64), np.asarray(d, np.float64)
    B = gy.shape[0]
    gz2, ab2 = np.zeros((B, D + L), np.int64), np.zeros((B, D + L), np.int64)
    if gnb is not None:
        gz2[:, L:] += 2 * np.asarray(gnb, np.int64)
        ab2[:, L:] += 2 * np.abs(np.asarray(gnb, np.int64))
    kf = np.floor(d)
    n = np.broadcast_to(np.arange(L), (B, L))
    rows = np.broadcast_to(np.arange(B)[:, None], (B, L))
    for tap in (1, 0):
        m = kf + tap
        w2 = 2.0 * (1.0 - np.abs(m - d))
        assert np.all(w2 == np.round(w2)), "weights must be 0, 1/2 or 1"
        on = (m >= 0) & (m <= D) & (w2 > 0)
        tgt = (D + n - m.astype(np.int64))[on]
        assert tgt.size == 0 or (tgt.min() >= 0 and tgt.max() < D + L)
        np.add.at(gz2, (rows[on], tgt), w2.astype(np.int64)[on] * gy[on])
        np.add.at(ab2, (rows[on], tgt), w2.astype(np.int64)[on] * np.abs(gy[on]))
    out = (gz2.astype(np.float64) / 2.0).astype(np.float32)
    return out[:, D:], out[:, :D], int(ab2.max())


def delay_exact_inputs(kind, L, D):
    """(d float32 (B, L), gy int64 (B, L), g_newbuf int64 (B, D)) of one exact case, as torch CPU tensors."""
    import torch
    g = torch.Generator().manual_seed(100000 * DELAY_EXACT_KINDS.index(kind) + 10 * L + D)
    d = delay_trajectory(kind, DELAY_B, L, D, g)
    gy = torch.randint(-3, 4, (DELAY_B, L), generator=g)
    gnb = torch.randint(-3, 4, (DELAY_B, D), generator=g)
    return d, gy, gnb
