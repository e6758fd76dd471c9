"""What tests/test_tcn_cases_cpu.py and tests/test_gpu_tcn.py share: exact-integer TCNs, the float64 reference, the probe that
reads an inner block through the public API, the poisoned scratch, a mirror of launch_tcn's shape arithmetic and the case tables.

Exact networks.  Integer inputs, weights in {-1, 0, 1}, integer biases and PReLU slopes that are multiples of 1/8 make every
value of every block an integer multiple of a power-of-two unit (the unit shrinks by 8 per block).  As long as every sum of
magnitudes, counted in units, stays below 2^24, every partial sum in ANY order is a float32 number: the matrix pipe, the C oracle
and float64 give the same bits, and the bar of a test is `==`.  assert_exact asks for 2^22: the two bits of headroom cover the
partial sums of the fused output conv.  The condition is checked on the float64 reference, never on the code under test."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

C, K = 32, 13
EIGHTHS = tuple(k / 8.0 for k in range(-16, 16))          # 32 distinct slopes: negative, 0, 1 and above 1
HALVES = (0.0, 0.5, -0.5, 1.0, -1.0)                      # the fall-back for deep networks (the unit shrinks by 2 per block)
EXACT_LIMIT = float(2 ** 22)


# ---- exact networks -------------------------------------------------------------------------------------------------
def exact_tcn(dilations, seed, slopes=None):
    """A TCN whose parameters are overwritten in place: first block weights in {-1, 0, 1} on all 13 taps; 32-channel blocks
    with 3 non-zero input channels per (output channel, tap) and 2 non-zero residual entries per output channel; biases in
    [-2, 2]; a dense out_weight in {-1, 1}; a non-zero integer out_bias.  slopes: the values the PReLU slopes are drawn from;
    default: a permutation of k/8, k = -16..15 per block (32 distinct values) up to two blocks, HALVES for deeper networks,
    whose magnitudes counted in units pass 2^22 with eighths (three blocks: 4.7e6 at the output conv)."""
    import ntm_amd
    dilations = tuple(int(d) for d in dilations)
    if slopes is None:
        slopes = EIGHTHS if len(dilations) <= 2 else HALVES
    m = ntm_amd.TCN(dilations=dilations, seed=1)
    rng = np.random.default_rng(seed)
    cin = 1
    with torch.no_grad():
        for l in range(len(dilations)):
            if cin == 1:
                W = rng.integers(-1, 2, (C, 1, K)).astype(np.float32)
                R = rng.integers(-1, 2, (C, 1, 1)).astype(np.float32)
            else:
                Wk = np.zeros((C, K, cin), np.float32)                      # [co][k][ci]
                idx = np.argsort(rng.random((C, K, cin)), axis=-1)[..., :3]
                np.put_along_axis(Wk, idx, rng.choice([-1.0, 1.0], (C, K, 3)).astype(np.float32), axis=-1)
                W = np.ascontiguousarray(Wk.transpose(0, 2, 1))
                Rk = np.zeros((C, cin), np.float32)
                idx = np.argsort(rng.random((C, cin)), axis=-1)[:, :2]
                np.put_along_axis(Rk, idx, rng.choice([-1.0, 1.0], (C, 2)).astype(np.float32), axis=-1)
                R = Rk[:, :, None]
            if len(slopes) >= C:
                al = rng.permutation(np.asarray(slopes, np.float32))[:C]
            else:
                al = rng.choice(np.asarray(slopes, np.float32), C)
            m.conv_weight[l].copy_(torch.from_numpy(W))
            m.conv_bias[l].copy_(torch.from_numpy(rng.integers(-2, 3, C).astype(np.float32)))
            m.prelu[l].copy_(torch.from_numpy(np.ascontiguousarray(al)))
            m.res_weight[l].copy_(torch.from_numpy(R))
            cin = C
        m.out_weight.copy_(torch.from_numpy(rng.choice([-1.0, 1.0], (1, C, 1)).astype(np.float32)))
        m.out_bias.fill_(float(rng.choice([-3, -2, -1, 1, 2, 3])))
    return m


def exact_input(B, T, seed):
    """Integers in [-3, 3], (B, 1, T) float32."""
    return torch.from_numpy(np.random.default_rng(seed).integers(-3, 4, (B, 1, T)).astype(np.float32))


def unit_of(t):
    """The largest power of two <= 1 that every value of t is an integer multiple of (0.0: none down to 2^-40)."""
    t = t.detach().double()
    for s in range(41):
        v = t * 2.0 ** s
        if bool((v == v.round()).all()):
            return 2.0 ** -s
    return 0.0


def ref64(model, x):
    """The network in torch float64 on the CPU (F.pad, F.conv1d, F.prelu: what tests/test_oracle.py pins the C oracle to).
    x (B, 1, T) -> y [B, T] float64, the activation [B, T, 32] of every block, and the magnitude bounds: per block
    max over outputs of (max(1, |alpha|) (|b| + sum |W| |in|) + sum |R| |in|) counted in the block's power-of-two unit,
    then the same of the output conv.  Every partial sum of the block, the PReLU product and the residual sum are integers of
    at most that size in that unit.  (inf where a parameter or the input is no multiple of 2^-40: a dense float network.)"""
    a = x.detach().cpu().double()
    unit = unit_of(a)
    acts, bounds = [], []
    for W, b, al, R, d in zip(model.conv_weight, model.conv_bias, model.prelu, model.res_weight, model.dilations):
        W, b, al, R = (t.detach().cpu().double() for t in (W, b, al, R))
        u = F.conv1d(F.pad(a, ((K - 1) * d, 0)), W, b, dilation=d)
        nxt = F.prelu(u, al) + F.conv1d(a, R)
        mag = F.conv1d(F.pad(a.abs(), ((K - 1) * d, 0)), W.abs(), b.abs(), dilation=d) * al.abs().clamp(min=1.0)[None, :, None] \
            + F.conv1d(a.abs(), R.abs())
        u_unit = min(unit * unit_of(W), unit_of(b))
        unit = min(u_unit * unit_of(al), unit * unit_of(R))
        bounds.append(float(mag.max()) / unit if unit > 0 else float("inf"))
        acts.append(nxt.transpose(1, 2).contiguous())
        a = nxt
    ow, ob = model.out_weight.detach().cpu().double(), model.out_bias.detach().cpu().double()
    y = F.conv1d(a, ow, ob)[:, 0, :]
    unit = min(unit * unit_of(ow), unit_of(ob))
    bounds.append(float(F.conv1d(a.abs(), ow.abs(), ob.abs()).max()) / unit if unit > 0 else float("inf"))
    return y, acts, bounds


def assert_exact(bounds):
    """A condition on the case, not a measurement of the code: every magnitude, in units, is below 2^22."""
    assert all(b < EXACT_LIMIT for b in bounds), bounds


# ---- the probe: an inner block's activation through the public API -------------------------------------------------------------
def with_probe(model):
    """The model plus one block behind it: conv_weight = 0, bias = 0, res_weight = identity, dilation 1, and a zero output conv
    (probe() makes it one-hot).  For any finite input the probe block returns its input bit for bit: its products are 0 or 1 v."""
    import ntm_amd
    pm = ntm_amd.TCN(dilations=model.dilations + (1,), seed=1)
    with torch.no_grad():
        for l in range(len(model.dilations)):
            for name in ("conv_weight", "conv_bias", "prelu", "res_weight"):
                getattr(pm, name)[l].copy_(getattr(model, name)[l].detach().cpu())
        pm.conv_weight[-1].zero_()
        pm.conv_bias[-1].zero_()
        pm.res_weight[-1].copy_(torch.eye(C)[:, :, None])
        pm.out_weight.zero_()
        pm.out_bias.zero_()
    return pm


def probe(model, forward, place=None):
    """forward(probe_model) -> the network's output [B, T]; called once per channel c with out_weight one-hot at c and
    out_bias = 0.  place(probe_model) moves the model where forward wants it, once.  Returns the [B, T, 32] activation of
    the model's last block -- with FUSE_OUT = false: the probe block is the one that carries the output conv."""
    pm = with_probe(model)
    if place is not None:
        pm = place(pm)
    cols = []
    for c in range(C):
        with torch.no_grad():
            pm.out_weight.zero_()
            pm.out_weight[0, c, 0] = 1.0
        y = forward(pm)
        cols.append(y if torch.is_tensor(y) else torch.from_numpy(np.asarray(y)))
    return torch.stack(cols, dim=-1)


def poisoned_scratch(model, B, T, value):
    """model._scratch = exactly ntm_tcn_scratch_floats(B, T, 32) floats of `value` on the model's device: forward() reuses it
    (the caller checks that), so every row at and behind T, the padding included, holds `value` when the first kernel starts."""
    import ntm_amd
    n = int(ntm_amd._lib.lib().ntm_tcn_scratch_floats(B, T, C))
    model._scratch = torch.full((n,), float(value), device=model.out_weight.device, dtype=torch.float32)
    return model._scratch


def first_mismatch(got, want):
    """None, or the index of the first element where got (float32) is not the float64 value (NaN counts as a mismatch)."""
    g = got.detach().cpu().double()
    assert g.shape == want.shape, (g.shape, want.shape)
    bad = ~(g == want)
    if not bool(bad.any()):
        return None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return idx, float(g[idx]), float(want[idx]), int(bad.sum())


# ---- mirror of launch_tcn's shape arithmetic (csrc/tcn_kernels.hip) ------------------------------------------------------------
TPW, PG_MIN_DIL = 512, 512


def ceil_div(a, b):
    return -(-a // b)


def block_kernel(d):
    return "pg" if d >= PG_MIN_DIL else "poly"


def poly_shape(d, T):
    """tcn_block_mfma2_kernel: tiles of 16 outputs of one phase, tau = p * tpp + t, 512 tiles per workgroup, 8 per iteration."""
    M = ceil_div(T, d)
    tpp = ceil_div(M, 16)
    total = d * tpp
    wgs = ceil_div(total, TPW)
    niter = [ceil_div(min(TPW, total - TPW * w), 8) for w in range(wgs)]
    starts = [divmod(TPW * w, tpp) for w in range(wgs)]                   # (phase, tile of the phase) of each workgroup's first tile
    samples = [max(0, ceil_div(T - p, d)) for p in range(d)]              # outputs per phase
    return dict(tpp=tpp, total=total, wgs=wgs, niter=niter, starts=starts, empty_phases=sum(1 for s in samples if s == 0),
                empty_last_tiles=sum(1 for s in samples if s <= 16 * (tpp - 1)))


def pg_shape(d, T):
    """tcn_block_pg_kernel: groups of 16 adjacent phases, two groups per workgroup, two time indices per iteration."""
    groups = ceil_div(d, 16)
    mtot = ceil_div(T, d)
    return dict(groups=groups, wgs=(groups + 1) // 2, idle_pair=groups % 2 == 1, last_group_phases=d - 16 * (groups - 1), mtot=mtot,
                niter=(mtot + 1) // 2, zero_page_groups=sum(1 for g in range(groups) if 16 * g >= T), straddles=T % 16 != 0)


def first_shape(d, T):
    """tcn_first_d1_kernel (d = 1): chunks of 256 samples, 8 per workgroup; tcn_first_kernel: 32 samples per workgroup."""
    if d == 1:
        return dict(kernel="first_d1", chunks=ceil_div(T, 256), wgs=ceil_div(T, 2048))
    return dict(kernel="first", wgs=ceil_div(T, 32), taps_in_range=min(K, ceil_div(T, d)))


# ---- the case tables: (dilation, T, what the mirror must say about the row) ----------------------------------------------------
FIRST_D1 = [(1, T, e) for T, e in (
    (1, dict(chunks=1, wgs=1)), (12, dict(chunks=1)), (13, dict(chunks=1)),           # shorter than / exactly the 13 taps
    (255, dict(chunks=1)), (256, dict(chunks=1)), (257, dict(chunks=2)),              # the 256-sample chunk, either side
    (2047, dict(chunks=8, wgs=1)), (2048, dict(chunks=8, wgs=1)), (2049, dict(chunks=9, wgs=2)),     # the 8-chunk workgroup
    (4097, dict(chunks=17, wgs=3)))]
def _first_rows(d):
    rows = {}
    for T, e in ((1, dict(wgs=1, taps_in_range=1)), (31, dict(wgs=1)), (32, dict(wgs=1)), (33, dict(wgs=2)),
                 (d, dict(taps_in_range=1)),                                            # T = d: only the tap at the sample itself
                 (12 * d + 1, dict(taps_in_range=13))):                                 # the last sample is the first with all 13 taps
        rows.setdefault(T, {}).update(e)                                                # (d = 33: T = 33 is two of these at once)
    return [(d, T, e) for T, e in rows.items()]


FIRST = [row for d in (2, 33, 600) for row in _first_rows(d)]

POLY = [
    (1, 1, dict(tpp=1, total=1)), (1, 15, dict(tpp=1)), (1, 16, dict(tpp=1)), (1, 17, dict(tpp=2)),
    (1, 128, dict(tpp=8, niter=[1])), (1, 129, dict(tpp=9, niter=[2])),
    (1, 8191, dict(tpp=512, wgs=1)), (1, 8192, dict(tpp=512, total=512, wgs=1, niter=[64])),      # exactly one workgroup of tiles
    (1, 8193, dict(tpp=513, wgs=2, niter=[64, 1], starts=[(0, 0), (0, 512)])),      # second workgroup: one tile, history = the first's last tile
    (7, 336, dict(tpp=3, empty_last_tiles=0)),                                        # tpp = 3 exactly
    (7, 337, dict(tpp=4, empty_last_tiles=6)),                                        # the last tile of phases 1..6 is empty
    (37, 3000, dict(tpp=6)),
    (23, 23 * 16 * 5, dict(tpp=5, empty_last_tiles=0)),
    (11, 11 * 16 * 7, dict(tpp=7, empty_last_tiles=0)),                               # tpp = 7 exactly: 8 tiles = one phase and one tile
    (11, 11 * 16 * 7 + 3, dict(tpp=8)),                                               # just past the 7 x 16 mark
    (40, 25, dict(tpp=1, empty_phases=15)),                                           # T < dil: phases 25..39 have no sample
    (200, 8000, dict(tpp=3, total=600, wgs=2, starts=[(0, 0), (170, 2)])),            # second workgroup starts mid-phase
    (511, 511, dict(tpp=1, wgs=1)), (511, 512, dict(tpp=1, wgs=1, empty_last_tiles=0)),
    (511, 511 * 16 + 5, dict(tpp=2, total=1022, wgs=2)),                              # the largest dilation here, two workgroups
]

PG_DILS = {512: dict(groups=32, idle_pair=False, last_group_phases=16),
           513: dict(groups=33, idle_pair=True, last_group_phases=1),
           527: dict(groups=33, idle_pair=True, last_group_phases=15),
           528: dict(groups=33, idle_pair=True, last_group_phases=16)}


def pg_lengths(d):
    """T and what it gives: mtot, niter (the loop is unrolled over 8 iterations; the ring of 16 blocks wraps every 8)."""
    return [(1, dict(mtot=1, niter=1, zero_page_groups=PG_DILS[d]["groups"] - 1)),
            (16, dict(mtot=1, zero_page_groups=PG_DILS[d]["groups"] - 1, straddles=False)),
            (17, dict(mtot=1, zero_page_groups=PG_DILS[d]["groups"] - 2, straddles=True)),
            (d - 1, dict(mtot=1)), (d, dict(mtot=1, niter=1)), (d + 1, dict(mtot=2, niter=1)),
            (2 * d + 1, dict(mtot=3, niter=2)), (13 * d + 1, dict(mtot=14, niter=7)), (15 * d, dict(mtot=15, niter=8)),
            (16 * d + 1, dict(mtot=17, niter=9)),
            (30 * d + 1, dict(mtot=31, niter=16)),                                    # exactly two passes through the unrolled eight
            (32 * d + 1, dict(mtot=33, niter=17))]                                    # the ring wrapped twice, a third pass begun


PG = [(d, T, dict(PG_DILS[d], **e)) for d in PG_DILS for T, e in pg_lengths(d)]

# one T per kernel for the tests that repeat a run (other scratch contents, streams alone): a row block / tile that straddles T
REPEAT_ROWS = {"first_d1": (1, 257), "first": (33, 33), "poly": (7, 337), "pg": (513, 2 * 513 + 1)}
B_EXACT = 2


def row_id(row):
    return f"d{row[0]}-T{row[1]}"


def case_seed(dilations, T):
    return (sum((i + 1) * 7919 * d for i, d in enumerate(dilations)) + 31 * T) % (2 ** 31)


@functools.lru_cache(None)
def exact_case(dilations, T, B=B_EXACT):
    """(model on the CPU, x (B, 1, T), y64 [B, T], activations, bounds) of the exact network with these dilations: computed
    once, shared by every test that needs it, never modified (tests copy the model before they move it)."""
    seed = case_seed(dilations, T)
    m = exact_tcn(dilations, seed)
    x = exact_input(B, T, seed + 1)
    y, acts, bounds = ref64(m, x)
    return m, x, y, acts, bounds


# ---- dense float cases ---------------------------------------------------------------------------------------------------------
DENSE = [((1, 7), 700, 0.8), ((1, 511, 512), 9000, 0.8), ((1, 513), 17409, 0.8), ((1, 10, 100, 1000), 17500, 0.8),
         ((2, 5, 1, 3), 900, 0.8), ((2, 5, 1, 3), 900, 4.0)]                           # the last: a loud input


def dense_tcn(dilations, seed):
    """TCN(dilations, seed) with its own random weights, 32 distinct slopes in (-0.5, 1.5) per block and a non-zero out_bias."""
    import ntm_amd
    m = ntm_amd.TCN(dilations=dilations, seed=seed)
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for al in m.prelu:
            al.copy_(torch.from_numpy(rng.permutation(np.linspace(-0.47, 1.47, C)).astype(np.float32)))
        m.out_bias.fill_(0.3125 + 0.01 * float(rng.random()))
    return m


def rel_err(got, ref):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got.astype(np.float64) - ref)) / np.max(np.abs(ref)))


@functools.lru_cache(None)
def dense_case(dilations, T, amp, B=2):
    """(model, x, y64, bar): bar = 3 x the distance of the float32 C oracle from float64 on this very case (the project's margin
    for the device's summation order, tests/diffusion_cases.py), at least 2^-23 -- from the references alone."""
    import oracle
    seed = case_seed(dilations, T) + int(10 * amp)
    m = dense_tcn(dilations, seed)
    x = torch.from_numpy(np.random.default_rng(seed + 1).uniform(-amp, amp, (B, 1, T)).astype(np.float32))
    y64, _, _ = ref64(m, x)
    y32 = oracle.tcn_forward(m.packed_params().numpy(), len(dilations), C, K, dilations, x[:, 0].numpy(), threads=B)
    return m, x, y64, max(3.0 * rel_err(y32, y64), 2.0 ** -23)
