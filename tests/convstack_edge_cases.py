"""What tests/test_convstack_edges_cpu.py and tests/test_gpu_convstack_edges.py share: the case tables of the three critic conv
stacks (csrc/critic_kernels.hip `spc`, csrc/convstack_kernels.hip `dil`, csrc/sconv_kernels.hip `mel`; the shared core is
csrc/convstack_common.h) above 32 streams and at the chunk, segment and tile edges, the two constructions (exact and dense),
Python mirrors of the three chunk rules and of the workspace sizes, and a float32 emulation of the documented order of the weight
gradient.  The torch twins, the bar and the strided family's size functions are those of the existing test modules
(test_gpu_critic, test_gpu_convstack, melgan_cases), imported and not restated.

Exact cases.  x, gout and the biases are small integers, slope = 0.5, every row of v has entries in {+-1, +-2, +-3} whose sum of
squares is a power of 4 (so |v| = 2^m; a 0 entry only where no such row exists, e.g. length 9), g = |v| 2^-s, so the effective
weight v 2^-s is exact.  Every value of every tensor is then an integer multiple of a power-of-two unit, and as long as the sum
of MAGNITUDES of an accumulation, counted in the unit of its terms, stays below 2^24, every partial sum in ANY order is a float32
number: the matrix pipe, torch's float32 and float64 give the same bits and the bar is `==`.  exact_bits() computes that count
per tensor from the float64 twin on absolute values and from the units of the operands, never from the code under test.  The
spectral family's slope is fixed at 0.2 (no power of two): its exact stacks have one layer, or two with a first-layer bias that
makes every pre-activation positive, and no log head.

Dense cases.  The constructions of the existing modules (standard normal x, v ~ N(0, 1 / fan_in), g = (1 .. 1.3) |v|), with
seeds picked on the CPU so that the float32 and float64 twins agree on every LeakyReLU side; the bar is the existing one,
4 max(|ref32 - ref64|, E32(kind) max|ref64|), E32 over this table's own dense cases per family."""
import collections
import functools
import zlib

import numpy as np
import torch

import melgan_cases as mel
import test_gpu_convstack as dil
import test_gpu_critic as spc

KINDS = ("out", "gx", "dg", "dv", "dbias")
MODS = {"dil": dil, "spc": spc, "mel": mel}
FLOOR = spc.FLOOR
Z, R = mel.Z, mel.R
EXACT_BITS = 24.0

Case = collections.namedtuple("Case", "id fam group spec B F0 kind par")


# ---- the three families behind one face ----------------------------------------------------------------------------------------
def frames(fam, F0, spec):
    """Frames entering every layer and leaving the last."""
    if fam == "mel":
        return mel.frames(F0, spec)
    Fr = [int(F0)]
    for s in spec:
        Fr.append(Fr[-1] - (s[2] - 1) * (s[4] if fam == "dil" else 1))
    return Fr


def input_frames(fam, spec, Fo):
    """The input length at which the LAST layer of a stride-1 stack leaves Fo frames."""
    assert fam != "mel"
    return Fo + sum((s[2] - 1) * (s[4] if fam == "dil" else 1) for s in spec)


def twin(case, inputs, dtype):
    x, params, gout = inputs
    return MODS[case.fam].twin(x, params, case.spec, case.par, gout, dtype)


def tensors(case, r):
    return MODS[case.fam].tensors(r)


def named(case, r):
    return {name: a for _, name, a in tensors(case, r)}


def kind_of(name):
    return name.split("[")[0]


def slope_of(case):
    return 0.2 if case.fam == "spc" else case.par


def pre_activations(case, x, params, dtype):
    """Every layer's pre-activation (the last layer: its output) in `dtype`, as float64 numpy: the last output of the twin run on
    the stack cut behind that layer."""
    m = MODS[case.fam]
    h = torch.from_numpy(np.asarray(x)).to(dtype)
    ps = [tuple(torch.from_numpy(np.asarray(a)).to(dtype) for a in p) for p in params]
    res = []
    with torch.no_grad():
        for l in range(len(case.spec)):
            o = m.twin_forward(h, ps[:l + 1], case.spec[:l + 1], case.par)
            res.append((o[-1] if case.fam == "mel" else o).double().numpy())
    return res


def sides_agree(case, inputs):
    """Do the float32 and the float64 twin sit on the same side of every LeakyReLU?"""
    p64, p32 = (pre_activations(case, inputs[0], inputs[1], dt) for dt in (torch.float64, torch.float32))
    return all(np.array_equal(a > 0, b > 0) for a, b in zip(p64[:-1], p32[:-1]))


# ---- the exact construction -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_recipe(n):
    """(zeros, ones, twos, threes, m): the fewest zeros, then the smallest m, with ones + 4 twos + 9 threes = 4^m."""
    for z in range(n):
        nn = n - z
        for m in range(12):
            diff = 4 ** m - nn
            if diff < 0 or 4 ** m > 9 * nn:
                continue
            for b in range(diff // 8, -1, -1):
                if (diff - 8 * b) % 3 == 0 and (diff - 8 * b) // 3 + b <= nn:
                    a = (diff - 8 * b) // 3
                    return z, nn - a - b, a, b, m
    raise AssertionError(n)


def exact_rows(co, n, rng):
    """v (co, n) with entries in {0, +-1, +-2, +-3} and |v| = 2^m in every row -> (v, m).  The zeros of row o sit at
    (o z + i) mod n, so they move from row to row and every position is non-zero in some row."""
    z, ones, twos, threes, m = row_recipe(n)
    v = np.zeros((co, n))
    for o in range(co):
        mags = rng.permutation(np.array([1.0] * ones + [2.0] * twos + [3.0] * threes))
        free = [p for p in range(n) if (p - o * z) % n >= z]
        v[o, free] = mags * rng.choice([-1.0, 1.0], n - z)
    assert ((v * v).sum(axis=1) == 4.0 ** m).all()
    return v, m


def exact_inputs_at(case, keep):
    """(x, params, gout) of an exact case: float32 numpy holding small integers and powers of two; one of `keep` gradient
    entries is non-zero."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    f = np.float32
    x = rng.integers(-2, 3, (case.B, case.spec[0][0], case.F0)).astype(f)
    params = []
    for l, s in enumerate(case.spec):
        ci, co, k, g = s[:4]
        v, m = exact_rows(co, ci // g * k, rng)
        # g = |v| 2^-s: one s per layer in a deeper stack (every bit of spread between rows is a bit of every sum above them),
        # 2, 1 or 1/2 per row in a one-layer stack
        gg = 2.0 ** (m - (rng.integers(m - 1, m + 2, co) if len(case.spec) == 1 else np.full(co, m)))
        params.append((gg.astype(f), v.reshape(co, ci // g, k).astype(f), rng.integers(-2, 3, co).astype(f)))
    if case.fam == "spc" and len(case.spec) == 2:
        # a positive integer bias above the sum of magnitudes of the first layer: every pre-activation is > 0 and LeakyReLU(0.2)
        # is the identity, forward and backward
        g0, v0, _ = params[0]
        one = Case(case.id, case.fam, case.group, case.spec[:1], case.B, case.F0, case.kind, case.par)
        bound = pre_activations(one, np.abs(x), [(g0, np.abs(v0), np.zeros_like(g0))], torch.float64)[0].max()
        params[0] = (g0, v0, (np.floor(bound) + 1 + rng.integers(0, 3, len(g0))).astype(f))
    Fr = frames(case.fam, case.F0, case.spec)
    gouts = []
    for l in range(len(case.spec)):
        shape = (case.B, case.spec[l][1], Fr[l + 1])
        gouts.append((rng.integers(-1, 2, shape) * (rng.integers(0, keep, shape) == 0)).astype(f))
    return x, params, (gouts if case.fam == "mel" else gouts[-1])


def row_length(case, l):
    return case.spec[l][0] // case.spec[l][3] * case.spec[l][2]


def may_leave(case):
    """The tensors of an exact case that MAY leave instrument 1: dv of a layer whose rows are longer than 64."""
    return {f"dv[{l}]" for l in range(len(case.spec)) if row_length(case, l) > 64}


KEEP = (1, 4, 16, 64)
THINNED = {}


def exact_inputs(case):
    """The exact case with the densest gradient (every entry, then one of 4, 16, 64 at random places) at which every sum meets
    the exactness condition -- found from exact_bits(), that is from the float64 twin on the CPU alone."""
    for keep in KEEP:
        inputs = exact_inputs_at(case, keep)
        if all(b < EXACT_BITS for name, b in exact_bits(case, inputs).items() if name not in may_leave(case)):
            break
    THINNED[case.id] = keep
    return inputs


def unit_of(a):
    """The largest power of two <= 1 that every value of `a` is an integer multiple of."""
    a = np.asarray(a, np.float64)
    for s in range(80):
        t = a * 2.0 ** s
        if (t == np.round(t)).all():
            return 2.0 ** -s
    raise AssertionError("not a multiple of 2^-79")


def exact_bits(case, inputs):
    """{tensor name: log2 of the largest sum of magnitudes of any accumulation behind it, counted in the unit of its terms}.
    The sums: the conv (out[l]; for the stride-1 families only the last is returned, the inner ones are out_pre[l]), the data
    gradient (gx; the inner gz are bounded by dbias of their layer, whose sum over streams and frames contains each of them),
    dbias, the weight gradient dW and the dot <dW, v> (both under dg[l]), and dW - v dot / |v|^2 (with the former under dv[l]).
    Magnitudes come from the float64 twin run on absolute values (with them every pre-activation is >= 0 and every LeakyReLU
    derivative the largest, 1); units are propagated from the operands."""
    x, params, gout = inputs
    n, fam, slope = len(case.spec), case.fam, slope_of(case)
    ab = lambda a: None if a is None else np.abs(a)
    pabs = [(g, np.abs(v), np.abs(b)) for g, v, b in params]
    gabs = [ab(a) for a in gout] if fam == "mel" else ab(gout)
    pre_abs = pre_activations(case, np.abs(x), pabs, torch.float64)
    rabs = named(case, twin(case, (np.abs(x), pabs, gabs), torch.float64))
    act_unit = 1.0 if fam == "spc" else unit_of(slope)         # spc: pre-activations are asserted > 0, the slope never multiplies
    norm = [np.sqrt((v.astype(np.float64) ** 2).sum(axis=(1, 2))) for _, v, _ in params]
    w_unit = [unit_of(v * (g / nr)[:, None, None]) for (g, v, _), nr in zip(params, norm)]
    bits, u_h = {}, [unit_of(x)]
    for l in range(n):
        u_pre = min(w_unit[l] * u_h[l], unit_of(params[l][2]))
        bits[f"out[{l}]" if fam == "mel" else ("out" if l == n - 1 else f"out_pre[{l}]")] = float(np.log2(pre_abs[l].max() / u_pre))
        u_h.append(u_pre * (act_unit if l < n - 1 else 1.0))
    gouts = gout if fam == "mel" else [None] * (n - 1) + [gout]
    u_gz = [None] * n
    for l in range(n - 1, -1, -1):
        here = [unit_of(gouts[l])] if gouts[l] is not None else []
        above = [u_gz[l + 1] * w_unit[l + 1]] if l < n - 1 else []
        u_gz[l] = min(here + above) * (act_unit if l < n - 1 else 1.0)
    bits["gx"] = float(np.log2(rabs["gx"].max() / (u_gz[0] * w_unit[0])))
    for l in range(n):
        g, v, _ = params[l]
        g, v, nr = g.astype(np.float64), np.abs(v).astype(np.float64), norm[l]
        bits[f"dbias[{l}]"] = float(np.log2(rabs[f"dbias[{l}]"].max() / u_gz[l]))
        dot_abs = rabs[f"dg[{l}]"] * nr
        dW_abs = rabs[f"dv[{l}]"] * (nr / g)[:, None, None] + v * (dot_abs / nr ** 2)[:, None, None]
        u_dW, u_v = u_gz[l] * u_h[l], unit_of(v)
        b_dW, b_dot = float(np.log2(dW_abs.max() / u_dW)), float(np.log2(dot_abs.max() / (u_dW * u_v)))
        bits[f"dg[{l}]"] = max(b_dW, b_dot)
        u_proj = u_v * u_dW * u_v / float(nr.max()) ** 2
        sub = (dW_abs + v * (dot_abs / nr ** 2)[:, None, None]).max() / min(u_dW, u_proj)
        bits[f"dv[{l}]"] = max(bits[f"dg[{l}]"], float(np.log2(sub)))
    return bits


def covered_positions(params):
    """Is every (input channel, tap) position non-zero in at least one row of every layer?"""
    return all(bool((np.abs(v) > 0).any(axis=0).all()) for _, v, _ in params)


# ---- mirrors of the chunk rules and the workspace sizes --------------------------------------------------------------------------
cdiv = mel.cdiv


def stream_chunks(B, max_chunks=32):
    """stack_stream_chunks (csrc/convstack_common.h) -> (nchunk, per)."""
    nchunk = (B if B > 0 else 1) if B < max_chunks else max_chunks
    per = max(cdiv(B, nchunk), 1)
    return cdiv(B, per), per


def layer_rule(fam, B, Fo, W):
    """(nchunk, per, nseg) of one layer's weight gradient."""
    if fam == "mel":
        _, nseg, per, nchunk = mel.chunk_rule(B, Fo, W)
        return nchunk, per, nseg
    nchunk, per = stream_chunks(B)
    return nchunk, per, (cdiv(Fo, 1024) if fam == "dil" else 1)


def weights_of(spec):
    return [s[1] * (s[0] // s[3]) * s[2] for s in spec]


def rules(case):
    Fr = frames(case.fam, case.F0, case.spec)
    return [layer_rule(case.fam, case.B, Fr[l + 1], W) for l, W in enumerate(weights_of(case.spec))]


def partials(case):
    return [nchunk * nseg for nchunk, _, nseg in rules(case)]


def workspace_floats(case):
    """ws = gz ping | gz pong | (mel: fold) | per layer nchunk nseg (W + c_out), as include/ntm.h states it."""
    if case.fam == "mel":
        return mel.sizes(case.B, case.spec[0][0], case.F0, case.spec)[1]
    Fr = frames(case.fam, case.F0, case.spec)
    gz = max([case.B * s[1] * Fr[l + 1] for l, s in enumerate(case.spec[:-1])] + [0])
    return 2 * gz + sum(p * (W + s[1]) for p, W, s in zip(partials(case), weights_of(case.spec), case.spec))


def library_workspace_floats(case):
    import ntm_amd
    L, lib = ntm_amd._lib.lib(), ntm_amd._lib
    fn, lay = {"dil": (L.ntm_convstack_workspace_floats, lib.conv_layers_d), "spc": (L.ntm_speccrit_workspace_floats, lib.conv_layers),
               "mel": (L.ntm_sconvstack_workspace_floats, lib.conv_layers_s)}[case.fam]
    return int(fn(case.B, case.spec[0][0], case.F0, len(case.spec), lay(case.spec)))


# ---- the tables ------------------------------------------------------------------------------------------------------------------
STREAM_BS = (31, 32, 33, 64, 65)
STREAM_RULES = {31: (31, 1), 32: (32, 1), 33: (17, 2), 64: (32, 2), 65: (22, 3)}           # B -> (nchunk, per)
FRAMES = (63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2049)
PARTIAL_COUNTS = (1, 4, 5, 8, 9)

D_NARROW3 = ((3, 16, 3, 1, 7), (16, 17, 4, 1, 2), (17, 5, 2, 1, 3))
D_TWO = ((3, 16, 3, 1, 7), (16, 5, 4, 1, 2))
D_TWO_WIDE = ((4, 17, 4, 1, 2), (17, 20, 3, 1, 5))
D_WIDE3 = ((1, 64, 5, 1, 1), (64, 64, 5, 1, 3), (64, 1, 5, 1, 1))
D_GROUPS2 = ((8, 32, 3, 4, 1), (32, 8, 4, 4, 2))
S_TWO = ((4, 16, 3, 1), (16, 3, 4, 1))
S_TWO_WIDE = ((5, 17, 4, 1), (17, 16, 3, 1))
S_THREE = ((6, 16, 3, 1), (16, 32, 4, 4), (32, 1, 3, 1))
M_TWO = ((2, 8, 5, 1, 1, 2, R), (8, 4, 4, 2, 2, 1, Z))
M_LONG = ((2, 4, 3, 1, 1, 1, Z),)
M_THREE = ((1, 8, 15, 1, 1, 7, R), (8, 16, 8, 2, 4, 2, Z), (16, 1, 3, 1, 1, 1, Z))
# one layer (c_in, c_out, k, groups): cout_g in {1, 15, 16, 17, 64, 65}, cin_g in {15, 16, 17}, cin_g k in {63, 64, 65},
# k in {1, 3, 4, 5}, groups in {1, 4}
CHANNELS = ((15, 1, 4, 1), (16, 15, 4, 1), (17, 16, 1, 1), (21, 17, 3, 1), (13, 64, 5, 1), (16, 65, 4, 1), (60, 64, 3, 4), (64, 68, 4, 4),
            (68, 4, 5, 4))
CHANNELS_DENSE = (3, 5, 7, 8)                 # of them also as dense cases
# the strided family's dot kernel: one output channel per group and >= 128 reduction indices, forward and in the data gradient
M_DOT = ((64, 1, 5, 1, 2, 2, Z), (1, 64, 5, 1, 2, 2, Z))


def _strided(layer):
    ci, co, k, g = layer
    return (ci, co, k, g, 2, 1, Z) if k > 1 else (ci, co, k, g, 1, 0, Z)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case of the three tables, in a fixed order."""
    rows = []

    def add(fam, group, tag, spec, B, F0, kind, par=None):
        par = (0.5 if kind == "exact" else 0.2) if par is None else par
        if fam == "spc" and par in (0.5, 0.2):
            par = 0.0                                                      # the spectral family's parameter is the log floor
        rows.append(Case(f"{fam}-{group}-{tag}-{kind}", fam, group, tuple(spec), B, F0, kind, par))

    def stride1(fam, group, tag, spec, B, Fo, kind, par=None):
        add(fam, group, tag, spec, B, input_frames(fam, spec, Fo), kind, par)

    # ---- dilated ----
    for B in STREAM_BS:
        stride1("dil", "streams", f"B{B}", D_TWO, B, 150, "exact")
    for B in (33, 65):
        stride1("dil", "streams", f"B{B}", D_NARROW3, B, 150, "dense")
    stride1("dil", "streams", "wide-B65", D_TWO_WIDE, 65, 300, "exact")
    stride1("dil", "streams", "wide-B33", D_WIDE3, 33, 70, "dense")
    stride1("dil", "streams", "B33-F1025", D_TWO, 33, 1025, "exact")
    for Fo in FRAMES:
        for form, co in (("narrow", 16), ("wide", 17)):
            for kind in ("exact", "dense") if Fo in (65, 257, 1025, 2049) else ("exact",):
                stride1("dil", "frames", f"{form}-F{Fo}", ((5, co, 3, 1, 2),), 3 if Fo == 2049 else 2, Fo, kind)
    for i, (ci, co, k, g) in enumerate(CHANNELS):
        for kind in ("exact", "dense") if i in CHANNELS_DENSE else ("exact",):
            stride1("dil", "channels", f"{ci}x{co}k{k}g{g}", ((ci, co, k, g, 1 + i % 3),), 3, 70, kind)
    for kind in ("exact", "dense"):
        stride1("dil", "channels", "two-grouped", D_GROUPS2, 3, 70, kind)
    for B, Fo in ((1, 40), (4, 40), (5, 40), (8, 40), (9, 40), (4, 1025), (3, 2049)):
        stride1("dil", "partials", f"B{B}-F{Fo}", ((2, 4, 3, 1, 1),), B, Fo, "exact")
    # ---- spectral ----
    for B in STREAM_BS:
        stride1("spc", "streams", f"B{B}", S_TWO, B, 150, "exact")
    stride1("spc", "streams", "B33-head", S_THREE, 33, 150, "dense", FLOOR)
    stride1("spc", "streams", "B65", S_THREE, 65, 150, "dense", 0.0)
    for Fo in FRAMES[:9]:
        for form, co in (("narrow", 16), ("wide", 17)):
            for kind in ("exact", "dense") if Fo in (65, 129, 257) else ("exact",):
                stride1("spc", "frames", f"{form}-F{Fo}", ((5, co, 3, 1),), 2, Fo, kind)
    for Fo in (65, 257):
        stride1("spc", "frames", f"three-F{Fo}", S_THREE, 3, Fo, "dense", FLOOR)
    for i, layer in enumerate(CHANNELS):
        for kind in ("exact", "dense") if i in CHANNELS_DENSE else ("exact",):
            stride1("spc", "channels", "{}x{}k{}g{}".format(*layer), (layer,), 3, 70, kind)
    stride1("spc", "channels", "two-wide", S_TWO_WIDE, 3, 70, "exact")
    for B in PARTIAL_COUNTS:
        stride1("spc", "partials", f"B{B}", ((2, 4, 3, 1),), B, 40, "exact")
    # ---- MelGAN ----
    for kind in ("exact", "dense"):
        add("mel", "streams", "B5-F700", M_TWO, 5, 700, kind)
    for B in (33, 65):
        add("mel", "streams", f"B{B}-F2048", M_LONG, B, 2048, "exact")
    add("mel", "streams", "B65-F2048", M_LONG, 65, 2048, "dense")
    for Fo in FRAMES:
        for s in (2, 3, 4):
            for rem, co in ((0, 8), (s - 1, 17)):                           # no remainder on the narrow tile, s - 1 on the wide one
                for kind in ("exact", "dense") if Fo in (65, 1025) else ("exact",):
                    add("mel", "frames", f"s{s}r{rem}-F{Fo}", ((3, co, 5, 1, s, 2, Z),), 2, (Fo - 1) * s + 1 + rem, kind)
    for i, layer in enumerate(CHANNELS):
        for kind in ("exact", "dense") if i in CHANNELS_DENSE else ("exact",):
            add("mel", "channels", "{}x{}k{}g{}".format(*layer), (_strided(layer),), 3, 141, kind)
    for layer in M_DOT:
        for kind in ("exact", "dense"):
            add("mel", "channels", f"dot-{layer[0]}x{layer[1]}", (layer,), 3, 141, kind)
    for kind in ("exact", "dense"):
        add("mel", "channels", "three", M_THREE, 3, 300, kind)
    for B, F0 in ((1, 50), (8, 1024), (9, 1024), (8, 2048), (6, 2049)):
        add("mel", "partials", f"B{B}-F{F0}", M_LONG, B, F0, "exact")
    assert len({c.id for c in rows}) == len(rows)
    return tuple(rows)


def case(cid):
    return next(c for c in cases() if c.id == cid)


def groups(kind):
    """[(family, group)] that hold cases of this kind, in table order."""
    seen = []
    for c in cases():
        if c.kind == kind and (c.fam, c.group) not in seen:
            seen.append((c.fam, c.group))
    return seen


# seeds of the dense cases, picked on the CPU so that the float32 and float64 twins agree on every LeakyReLU side
# (tests/test_convstack_edges_cpu.py asserts it): 6100 + the case's index in cases() unless named here
SEEDS = {}
# the dv tensors of exact cases that leave instrument 1 for the float bar, {case id: (tensor names)}: rows longer than 64 whose
# <dW, v> is no float32 number (tests/test_convstack_edges_cpu.py fails if this holds anything else than exact_bits() says)
DV_INEXACT = {}

# the order test: one dilated layer, B = 65 (22 chunks of 3, the last of 2), 1030 output frames (two segments: 16 steps and 1)
ORDER = Case("dil-order-B65-F1030-dense", "dil", "order", ((2, 3, 3, 1, 2),), 65, 1034, "dense", 0.2)
ORDER_SEED = 7001


def seed_of(c):
    return SEEDS.get(c.id, 6100 + cases().index(c))


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(inputs, ref64, ref32) of a case -- computed once, shared, never written to."""
    c = ORDER if cid == ORDER.id else case(cid)
    if c.kind == "exact":
        inputs = exact_inputs(c)
    else:
        seed = ORDER_SEED if c is ORDER else seed_of(c)
        m = MODS[c.fam]
        inputs = m.make_case(seed, c.B, c.spec[0][0], c.F0, c.spec, c.par) if c.fam == "spc" else m.make_case(seed, c.B, c.F0, c.spec)
    return inputs, twin(c, inputs, torch.float64), twin(c, inputs, torch.float32)


@functools.lru_cache(maxsize=None)
def e32(fam):
    """E32 per tensor kind over the dense cases of one family's table, from the two torch twins only."""
    refs = [reference(c.id) for c in cases() if c.fam == fam and c.kind == "dense"]
    return MODS[fam].e32_of([(r[1], r[2]) for r in refs])


# ---- the documented order of the weight gradient, in float32 ---------------------------------------------------------------------
def tree_sum(vals):
    """block_sum<256>: 256 slots, red[i] += red[i + s] for s = 128 .. 1."""
    red = np.zeros(256, np.float32)
    red[:len(vals)] = vals
    s = 128
    while s > 0:
        red[:s] = red[:s] + red[s:2 * s]
        s //= 2
    return red[0]


def emulate_order(c, inputs):
    """dg, dv, dbias of a ONE-layer dilated stack in float32 in the order csrc/convstack_kernels.hip and convstack_common.h
    document: a workgroup per (stream chunk, segment of 1024 frames) walks the streams of its chunk in order and the frames in
    steps of 64, adds kSub = 4 steps from 0 and then that sum to its total (the tail at the end), the bias gradient 64 frames
    from 0 at a time; stack_wnorm_kernel adds the partials chunk-major, segment-minor, then <dW, v> over 256 slots in a tree.
    Inside a step the frames are taken in ascending order with an unrounded product (the MFMA's own inner order is not
    documented: this is one guess, and the reason the comparison with it is a float bar plus a printed count); dv takes
    dW - v proj as one fused multiply-subtract, as the compiler contracts it."""
    assert len(c.spec) == 1 and c.fam == "dil"
    f = np.float32
    x, ((g, v, _),), gout = inputs
    (ci, co, K, _, d), B = c.spec[0], c.B
    Fo, n = gout.shape[2], ci * K
    X = np.stack([x[:, j // K, (j % K) * d:(j % K) * d + Fo] for j in range(n)], axis=1).astype(np.float64)     # (B, n, Fo)
    G = gout.astype(np.float64)
    (nchunk, per, nseg), = rules(c)
    parts, bparts = [], []
    for chunk in range(nchunk):
        for seg in range(nseg):
            fs0, fs1 = seg * 1024, min(Fo, (seg + 1) * 1024)
            steps = [(b, f0) for b in range(chunk * per, min((chunk + 1) * per, B)) for f0 in range(fs0, fs1, 64)]
            tot, acc, bsum = np.zeros((co, n), f), np.zeros((co, n), f), np.zeros(co, f)
            for it, (b, f0) in enumerate(steps):
                s = np.zeros(co, f)
                for t in range(f0, min(f0 + 64, fs1)):
                    acc = (acc.astype(np.float64) + G[b, :, t, None] * X[b, None, :, t]).astype(f)
                    s = s + gout[b, :, t]
                bsum = bsum + s
                if (it + 1) % 4 == 0 or it + 1 == len(steps):
                    tot, acc = tot + acc, np.zeros((co, n), f)
            parts.append(tot)
            bparts.append(bsum)
    dW, db = parts[0], bparts[0]
    for p, q in zip(parts[1:], bparts[1:]):
        dW, db = dW + p, db + q
    vv = v.reshape(co, n)
    dg, dv = np.zeros(co, f), np.zeros((co, n), f)
    for o in range(co):
        inv = f(1.0) / np.sqrt(tree_sum(vv[o] * vv[o]))
        dot = tree_sum(dW[o] * vv[o])
        scale, proj = g[o] * inv, dot * inv * inv
        dv[o] = scale * (dW[o].astype(np.float64) - vv[o].astype(np.float64) * np.float64(proj)).astype(f)      # one fused multiply-subtract
        dg[o] = dot * inv
    assert dW.dtype == f and dv.dtype == f and dg.dtype == f and db.dtype == f
    return {"dg[0]": dg, "dv[0]": dv.reshape(v.shape), "dbias[0]": db}
