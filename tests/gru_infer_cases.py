"""Case tables, inputs, weights and references for the edge tests of the GRU inference kernels off the headline
(tests/test_gpu_gru_infer_edges.py; the tables and builders are checked on the CPU by tests/test_gru_infer_cases_cpu.py):

  csrc/gru_small.hip   gru_small_kernel<8|16|32|64, PAD>   every H < 64       "small"
                       gru_wide_kernel<REGW>               64 < H <= 1024     "wide"
                       gru_io_kernel                       input_size / output_size other than 1   "io"
  csrc/gru_lat.hip     gru_lat_kernel<HEADW, REP>          H = 64 with NTM_GRU_LAT                 "lat"

Every reference is computed here from the oracle (fp32 and fp64 mode) or, for the io kernel's fp64, from torch.nn.GRU + nn.Linear
in float64 -- once per hidden size at the longest T, in segments that end at every T of the list (the GRU is causal: a shorter run
is the prefix, and the state carried between two segments is the final state of the shorter run).  Nothing in this module loads
the device library."""
import functools

import numpy as np

# ---- the constants behind the length lists, each the mirror of one line of the kernels (the CPU test reads them back)
TT = 64             # gru_small.hip `constexpr int TT = 64`: samples per x / y tile of gru_small_kernel and gru_wide_kernel
LT = 256            # gru_lat_step.h `constexpr int LT = 256`: samples per x / y tile of gru_lat_kernel
X_PREFETCH = 128    # gru_lat.hip `if (ns > 128 && tid < LT)`: the step behind which the next x tile comes in
Y_DEFER = 2         # gru_lat.hip `if (ns > 2 && tile0 >= LT ...)` and gru_lat_step.h finish() `(T - 1 - last0) < 2`
H_LAT = 64          # ntm.h NTM_HIDDEN: the low-latency kernel's hidden size
H_SMALL_MAX = 64    # gru_small.hip `if (H > 64)`: above it a workgroup per stream
H_REGW_MAX = 128    # gru_small.hip `if (H <= 128)`: gru_wide_kernel<true> (weights in registers), above it <false> (from L2)
H_MAX = 1024        # gru_small.hip `H > 1024` is refused
WIDE_THREADS = 256  # gru_wide_kernel<false> strides the units by the workgroup's 256 threads ...
WAVE = 64           # ... and the columns by the wave's 64 lanes

TILE64_T = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)
LAT_T = (1, 2, 3, 4, 127, 128, 129, 130, 255, 256, 257, 258, 259, 383, 384, 385, 386, 511, 512, 513, 514, 515)

H_EXACT = (8, 16, 32)
H_PADDED = {1: 8, 5: 8, 7: 8, 9: 16, 15: 16, 17: 32, 31: 32, 33: 64, 48: 64, 63: 64}     # H -> HP of gru_small_kernel<HP, true>
H_REGW = (65, 96, 127, 128)
H_L2 = (129, 200, 255, 256, 257, 300)
H_HUGE, HUGE_B, HUGE_T = 1024, 2, (3,)
SMALL_H = tuple(sorted(H_EXACT + tuple(H_PADDED)))
WIDE_H = H_REGW + H_L2 + (H_HUGE,)
WIDE_B = IO_B = (1, 3)
LAT_SMALL_B = (1, 3)                    # and CUs + 1, known on the device only
MI355X_CUS = 256                        # the count the CPU test assumes when it checks the rows of the large `lat` batch
PAD_PAIRS = ((5, 8), (12, 16), (24, 32), (96, 128), (200, 256))     # (H, HP): the padding identity, small <HP, true> and both wide forms
# (H, input_size, output_size) of the io kernel: I below / above its 256-thread load loop, O below / above its four waves, H below /
# above the 64-lane column stride and the 256-thread unit stride
IO_CASES = ((5, 3, 2), (64, 2, 5), (257, 1, 4), (16, 257, 3), (300, 4, 1))
REP_T, REP_R, REP_BPER = (258, 385), 2, 2

W_G = "GRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE]_BEST"
KEYS = ("GRU.weight_ih_l0", "GRU.weight_hh_l0", "GRU.bias_ih_l0", "GRU.bias_hh_l0", "output.weight", "output.bias")

GATE = 1e-5                             # the project's gate on |hip - oracle32| (BASELINE.json north_star); it stays
MARGIN = 4                              # the project's margin over a reference's own float32
ULP = 2.0 ** -23                        # the floor: one ulp of the largest |f64|
E_REF_MAX = GATE / MARGIN               # 2.5e-6: above it MARGIN * E_ref would exceed the gate and say nothing
SEED = {}                               # (kernel, H[, I, O]) -> input seed, default 0: change a SEED, never a bar


def padded_size(H):
    """gru_small.hip `int HP = 8; while (HP < H) HP *= 2;`"""
    assert 1 <= H <= H_SMALL_MAX
    HP = 8
    while HP < H:
        HP *= 2
    return HP


def streams_per_wave(H):
    return WAVE // padded_size(H)


def kernel_of(H):
    """The instantiation launch_gru_small picks for a hidden size other than 64."""
    assert 1 <= H <= H_MAX and H != H_LAT
    if H > H_SMALL_MAX:
        return "wide<true>" if H <= H_REGW_MAX else "wide<false>"
    HP = padded_size(H)
    return f"small<{HP}{',true' if HP != H else ''}>"


def small_batches(H):
    """B in {1, S - 1, S, S + 1, 2 S + 1} for S streams per wave, zeros and duplicates dropped."""
    S = streams_per_wave(H)
    return tuple(sorted({1, S - 1, S, S + 1, 2 * S + 1} - {0}))


def lat_batches(cus):
    return LAT_SMALL_B + (cus + 1,)


def lat_big_rows(cus):
    """The rows of the B = CUs + 1 batch that are compared with the oracle (every row is checked for prefix equality)."""
    return (0, cus // 2, cus)


def wide_lengths(H):
    return HUGE_T if H == H_HUGE else TILE64_T


def wide_batches(H):
    return (HUGE_B,) if H == H_HUGE else WIDE_B


def previous_y_tile_stored_by_finish(T):
    """True / False: which of the two places of gru_lat_kernel writes the y tile before the last one (None: there is none)."""
    last0 = (T - 1) // LT * LT
    if last0 < LT:
        return None
    return (T - 1 - last0) < Y_DEFER


# ---- inputs: one generator per (kernel, H, row), so that row r is the same whatever the batch size
def inputs(kernel, H, rows, T, width=1, seed=None):
    """x (len(rows), T * width) uniform +-0.7 and h0 (len(rows), H) uniform +-0.9, float32; `rows`: an int B (rows 0 .. B-1) or
    the row numbers."""
    rows = range(rows) if isinstance(rows, int) else rows
    seed = SEED.get((kernel, H), 0) if seed is None else seed
    x, h0 = [], []
    for r in rows:
        rng = np.random.default_rng([{"small": 1, "wide": 2, "io": 3, "lat": 4}[kernel], H, seed, r])
        h0.append(rng.uniform(-0.9, 0.9, H))
        x.append(rng.uniform(-0.7, 0.7, T * width))
    return np.asarray(x, np.float32), np.asarray(h0, np.float32)


# ---- weights
@functools.lru_cache(maxsize=None)
def random_sd(H, I=1, O=1):
    """torch.manual_seed(H) + ntm.RNN(I, H, O): nn.GRU's and nn.Linear's default initialisation -> {key: float32 array}."""
    import ntm_amd
    import torch
    torch.manual_seed(H)
    m = ntm_amd.RNN(I, H, O)
    sd = {k: v.detach().cpu().numpy().astype(np.float32).copy() for k, v in m.state_dict().items()}
    assert set(KEYS) <= set(sd)
    return {k: sd[k] for k in KEYS}


@functools.lru_cache(maxsize=None)
def ckpt_sd():
    from helpers import state_dict_np
    sd = state_dict_np(W_G)
    return {k: np.asarray(sd[k], np.float32) for k in KEYS}


def lat_sd(weights):
    return ckpt_sd() if weights == "ckpt" else random_sd(H_LAT)


LAT_WEIGHTS = ("ckpt", "rand")


def zero_padded(sd, HP):
    """The H-unit parameters embedded in HP-unit tensors: in every gate block the rows and columns at or beyond H are zero, and
    w_o is padded with zeros (input_size = output_size = 1)."""
    H = sd["GRU.weight_hh_l0"].shape[1]
    assert HP >= H and sd["GRU.weight_ih_l0"].shape == (3 * H, 1) and sd["output.weight"].shape == (1, H)
    out = {"GRU.weight_ih_l0": np.zeros((3 * HP, 1), np.float32), "GRU.weight_hh_l0": np.zeros((3 * HP, HP), np.float32),
           "GRU.bias_ih_l0": np.zeros(3 * HP, np.float32), "GRU.bias_hh_l0": np.zeros(3 * HP, np.float32),
           "output.weight": np.zeros((1, HP), np.float32), "output.bias": sd["output.bias"].copy()}
    for g in range(3):
        out["GRU.weight_ih_l0"][g * HP:g * HP + H] = sd["GRU.weight_ih_l0"][g * H:(g + 1) * H]
        out["GRU.weight_hh_l0"][g * HP:g * HP + H, :H] = sd["GRU.weight_hh_l0"][g * H:(g + 1) * H]
        out["GRU.bias_ih_l0"][g * HP:g * HP + H] = sd["GRU.bias_ih_l0"][g * H:(g + 1) * H]
        out["GRU.bias_hh_l0"][g * HP:g * HP + H] = sd["GRU.bias_hh_l0"][g * H:(g + 1) * H]
    out["output.weight"][0, :H] = sd["output.weight"][0]
    return out


def zero_padded_state(h0, HP):
    out = np.zeros((h0.shape[0], HP), h0.dtype)
    out[:, :h0.shape[1]] = h0
    return out


# ---- references
class Ref:
    """y32 / y64 (B, T_max * width) and h32[T] / h64[T] (B, H) for every T of `lengths`; e_y, e_h = max |oracle32 - f64| pooled
    over the rows and lengths (for y: all samples of the longest run, of which every case is a prefix)."""

    def __init__(self, lengths, y32, h32, y64, h64, pooled=None):
        self.lengths, self.y32, self.h32, self.y64, self.h64 = tuple(lengths), y32, h32, y64, h64
        self.e_y, self.e_h = pooled or (float(np.abs(y32 - y64).max()), float(max(np.abs(h32[T] - h64[T]).max() for T in lengths)))
        for a in (y32, y64, *h32.values(), *h64.values()):
            a.setflags(write=False)

    def rows(self, idx):
        """The references of some rows; E_ref stays the pooled one of the whole table."""
        return Ref(self.lengths, self.y32[idx], {T: h[idx] for T, h in self.h32.items()}, self.y64[idx],
                   {T: h[idx] for T, h in self.h64.items()}, pooled=(self.e_y, self.e_h))


def _segments(step, x, h0, lengths, width_in, width_out):
    """Run `step(x_segment, h) -> (y_segment, h)` over [0, T_1), [T_1, T_2), ... and keep the state behind every segment."""
    ys, hs, h, t0 = [], {}, h0, 0
    for T in lengths:
        y, h = step(x[:, t0 * width_in:T * width_in], h)
        ys.append(y.reshape(x.shape[0], (T - t0) * width_out))
        hs[T] = h.copy()
        t0 = T
    return np.concatenate(ys, 1), hs


def reference(sd, x, h0, lengths):
    """oracle.gru_forward / gru_forward_f64 in segments (input_size = output_size = 1) -> Ref."""
    import oracle
    w = oracle.Weights.from_state_dict(sd)
    lengths = tuple(sorted(lengths))
    assert x.shape[1] == lengths[-1]
    y32, h32 = _segments(lambda xs, h: oracle.gru_forward(w, xs, h), x, h0, lengths, 1, 1)
    y64, h64 = _segments(lambda xs, h: oracle.gru_forward_f64(w, xs, h), x, h0.astype(np.float64), lengths, 1, 1)
    return Ref(lengths, y32, h32, y64, h64)


def io_forward_f64(sd, xflat, h0):
    """The io case in float64: torch.nn.GRU(I, H, batch_first=True) + nn.Linear(H, O) on the CPU with the reference's reshape
    semantics, which oracle.gru_forward_io documents: per stream the input row of T * I floats IS the [T][I] matrix the GRU
    reads and the output row of T * O floats IS the [T][O] matrix the head writes.  -> (y (B, T * O), h (B, H)) float64."""
    import torch
    H, I = sd["GRU.weight_hh_l0"].shape[1], sd["GRU.weight_ih_l0"].shape[1]
    O = sd["output.weight"].shape[0]
    B, T = xflat.shape[0], xflat.shape[1] // I
    gru = torch.nn.GRU(I, H, batch_first=True).double()
    lin = torch.nn.Linear(H, O).double()
    with torch.no_grad():
        for p, k in ((gru.weight_ih_l0, KEYS[0]), (gru.weight_hh_l0, KEYS[1]), (gru.bias_ih_l0, KEYS[2]), (gru.bias_hh_l0, KEYS[3]),
                     (lin.weight, KEYS[4]), (lin.bias, KEYS[5])):
            p.copy_(torch.from_numpy(np.asarray(sd[k], np.float64)).reshape(p.shape))
        o, hn = gru(torch.from_numpy(np.asarray(xflat, np.float64)).reshape(B, T, I), torch.from_numpy(np.asarray(h0, np.float64)).reshape(1, B, H))
        y = lin(o).reshape(B, T * O)
    return y.numpy(), hn.reshape(B, H).numpy()


def io_forward_f32(sd, xflat, h0):
    """oracle.gru_forward_io on flat rows -> (y (B, T * O), h (B, H)) float32."""
    import oracle
    I, O = sd["GRU.weight_ih_l0"].shape[1], sd["output.weight"].shape[0]
    B, T = xflat.shape[0], xflat.shape[1] // I
    y, h = oracle.gru_forward_io(sd, xflat.reshape(B, I, T), h0)
    return y.reshape(B, T * O), h


# one reference per hidden size at the largest batch and the longest T, shared by every test that needs it
@functools.lru_cache(maxsize=None)
def small_ref(H):
    B, lengths = max(small_batches(H)), TILE64_T
    x, h0 = inputs("small", H, B, max(lengths))
    return x, h0, reference(random_sd(H), x, h0, lengths)


@functools.lru_cache(maxsize=None)
def wide_ref(H):
    B, lengths = max(wide_batches(H)), wide_lengths(H)
    x, h0 = inputs("wide", H, B, max(lengths))
    return x, h0, reference(random_sd(H), x, h0, lengths)


@functools.lru_cache(maxsize=None)
def io_ref(H, I, O):
    sd, lengths = random_sd(H, I, O), TILE64_T
    x, h0 = inputs("io", H, max(IO_B), max(lengths), width=I, seed=SEED.get(("io", H, I, O)))
    y32, h32 = _segments(lambda xs, h: io_forward_f32(sd, xs, h), x, h0, lengths, I, O)
    y64, h64 = _segments(lambda xs, h: io_forward_f64(sd, xs, h), x, h0.astype(np.float64), lengths, I, O)
    return x, h0, Ref(lengths, y32, h32, y64, h64)


@functools.lru_cache(maxsize=None)
def lat_ref(weights, rows):
    """`rows`: a tuple of row numbers of the `lat` batch (row r is the same in every batch size)."""
    x, h0 = inputs("lat", H_LAT, rows, max(LAT_T))
    return x, h0, reference(lat_sd(weights), x, h0, LAT_T)


def rep_sds():
    """The two replicas of the REP call: the shipped checkpoint and the random model."""
    return [ckpt_sd(), random_sd(H_LAT)]


def bar(e_ref, f64):
    """MARGIN * max(E_ref, one ulp of the largest |f64|)"""
    return MARGIN * max(e_ref, ULP * float(np.abs(f64).max()))
