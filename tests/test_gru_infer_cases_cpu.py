"""CPU: the case tables, builders and references of tests/gru_infer_cases.py, which tests/test_gpu_gru_infer_edges.py holds the
kernels of csrc/gru_small.hip and csrc/gru_lat.hip to -- the coverage claims of the length, hidden-size and batch lists (with
the constants read back from the sources), the zero-padding builder, the float64 reference of the io kernel, and the condition
under which the accuracy bar of the GPU tests says anything: every case's fp32 oracle within 2.5e-6 of fp64."""
import os
import re

import numpy as np
import pytest

import gru_infer_cases as C
import oracle
from helpers import ROOT

CSRC = os.path.join(ROOT, "neural-tape-modeling_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(set(m)) == 1, (pattern, m)
    return int(m[0])


def test_the_constants_are_the_ones_in_the_sources():
    small, lat, step = _src("gru_small.hip"), _src("gru_lat.hip"), _src("gru_lat_step.h")
    assert small.count("constexpr int TT = 64;") == 2 and _one(r"constexpr int TT = (\d+);", small) == C.TT
    assert _one(r"constexpr int LT = (\d+);", step) == C.LT
    assert _one(r"if \(ns > (\d+) && tid < LT\) \{", lat) == C.X_PREFETCH
    assert _one(r"run\(3, ns < (\d+) \? ns : \1, step, tb\);", lat) == C.X_PREFETCH + 1
    assert _one(r"if \(ns > (\d+) && tile0 >= LT && tid < LT\)", lat) == C.Y_DEFER
    assert _one(r"run\(0, ns < (\d+) \? ns : \1, step, tb\);", lat) == C.Y_DEFER + 1
    assert _one(r"if \(last0 >= LT && \(T - 1 - last0\) < (\d+)\)", step) == C.Y_DEFER
    assert C.LT == 1 << 8 and "(T - 1) >> 8" in step and "tile0 >> 8" in lat
    # the launch conditions of launch_gru_small
    launch = small[small.index("hipError_t launch_gru_small"):]
    assert _one(r"if \(H > (\d+)\) \{", launch) == C.H_SMALL_MAX
    assert _one(r"if \(H <= (\d+)\) hipLaunchKernelGGL\(gru_wide_kernel<true>", launch) == C.H_REGW_MAX
    assert _one(r"if \(H < 1 \|\| H > (\d+)\) return hipErrorInvalidValue;", launch) == C.H_MAX
    assert re.search(r"int HP = 8;\s*while \(HP < H\) HP \*= 2;\s*const int S = 64 / HP;", launch)
    assert sorted(int(v) for v in re.findall(r"case (\d+):", launch)) == [8, 16, 32, 64]
    assert _one(r"constexpr int HMAX = REGW \? (\d+) : 1024;", small) == C.H_REGW_MAX
    assert _one(r"for \(int uu = tid; uu < H; uu \+= (\d+)\)", small) == C.WIDE_THREADS
    assert _one(r"for \(int c = lane; c < H; c \+= (\d+)\) acc = __builtin_fmaf\(row\[c\], hs\[cur\]\[c\], acc\);", small) == C.WAVE
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    assert _one(r"#define NTM_HIDDEN (\d+)", header) == C.H_LAT and _one(r"#define NTM_MAX_HIDDEN (\d+)", header) == C.H_MAX
    # the CU count decides the head form of gru_lat_kernel
    assert re.search(r"if \(a\.B <= device_cus\(\)\) hipLaunchKernelGGL\(gru_lat_kernel<true>", lat)
    assert re.search(r"if \(a\.B <= device_cus\(\)\) hipLaunchKernelGGL\(\(gru_lat_kernel<true, true>\)", lat)


def test_lat_lengths_hold_both_sides_of_every_branch():
    T = C.LAT_T
    assert T == tuple(sorted(set(T)))
    for tiles in (0, 1, 2):                    # the edges inside the first, second and third tile
        base = tiles * C.LT
        if tiles:
            assert {base - 1, base, base + 1} <= set(T)                      # the tile itself
            assert {base + C.Y_DEFER, base + C.Y_DEFER + 1} <= set(T)        # `ns > 2`: the flush behind step 2 runs or not
            assert C.previous_y_tile_stored_by_finish(base + 1) is True and C.previous_y_tile_stored_by_finish(base + C.Y_DEFER) is True
            assert C.previous_y_tile_stored_by_finish(base + C.Y_DEFER + 1) is False
        if tiles < 2:
            assert {base + C.X_PREFETCH, base + C.X_PREFETCH + 1} <= set(T)  # `ns > 128`: the prefetch runs or not
    assert {C.previous_y_tile_stored_by_finish(t) for t in T} == {None, True, False}
    assert {1, C.Y_DEFER, C.Y_DEFER + 1, C.Y_DEFER + 2} <= set(T)            # the first tile's run(0, 3) cut short and complete
    assert {t & 1 for t in T if t > C.LT} == {0, 1}                          # finish() reads hb[T & 1]: both parities behind a tile
    assert max(T) > 2 * C.LT + C.Y_DEFER                                     # a third tile: x / y buffers come round, xnext was fetched in-kernel
    assert any(C.LT + C.X_PREFETCH < t < 2 * C.LT for t in T)                # a prefetch that runs past the end of x (the zero fill)
    assert set(C.REP_T) <= set(T) and C.previous_y_tile_stored_by_finish(C.REP_T[0]) is True


def test_tile64_lengths_hold_both_sides_of_every_tile():
    T = C.TILE64_T
    assert T == tuple(sorted(set(T)))
    for k in (1, 2, 3):
        assert {k * C.TT - 1, k * C.TT, k * C.TT + 1} <= set(T)
    assert {1, 2} <= set(T)                                                  # gru_wide's late y: no previous step, one previous step
    assert max(T) > 3 * C.TT                                                 # gru_small's xnext: a tile fetched two tiles ahead is used
    assert C.HUGE_T == (3,) and C.HUGE_B == 2


def test_hidden_sizes_hold_both_sides_of_every_kernel_boundary():
    hs = set(C.SMALL_H) | set(C.WIDE_H)
    assert C.H_LAT not in hs and len(C.SMALL_H) == 13
    for edge in (8, 16, 32):
        assert {edge - 1, edge, edge + 1} <= hs, edge
    for edge in (C.H_SMALL_MAX, C.H_REGW_MAX, C.WIDE_THREADS):               # 64 itself belongs to the other kernels
        assert {edge - 1, edge + 1} <= hs and (edge == C.H_LAT or edge in hs), edge
    assert 1 in hs and C.H_MAX in hs
    assert all(C.kernel_of(H) == f"small<{H}>" for H in C.H_EXACT)
    assert all(C.kernel_of(H) == f"small<{HP},true>" and C.padded_size(H) == HP for H, HP in C.H_PADDED.items())
    assert {C.padded_size(H) for H in C.H_PADDED} == {8, 16, 32, 64}
    assert all(C.kernel_of(H) == "wide<true>" for H in C.H_REGW) and all(C.kernel_of(H) == "wide<false>" for H in C.H_L2 + (C.H_HUGE,))
    assert any(H % C.WAVE for H in C.H_L2) and any(H > C.WIDE_THREADS for H in C.H_L2)
    want = {(5, 8): "small<8,true>", (12, 16): "small<16,true>", (24, 32): "small<32,true>", (96, 128): "wide<true>", (200, 256): "wide<false>"}
    assert dict.fromkeys(C.PAD_PAIRS) == dict.fromkeys(want)
    for (H, HP), k in want.items():
        assert C.kernel_of(H) == k and C.kernel_of(HP) == k.replace(",true", "")
    # the io kernel: both sides of its own strides
    assert {(I > C.WIDE_THREADS) for _, I, _ in C.IO_CASES} == {False, True} and {(O > 4) for _, _, O in C.IO_CASES} == {False, True}
    assert {(H > C.WAVE) for H, _, _ in C.IO_CASES} == {False, True} and any(H > C.WIDE_THREADS for H, _, _ in C.IO_CASES)
    assert any(I == 1 for _, I, _ in C.IO_CASES) and any(O == 1 for _, _, O in C.IO_CASES)


def test_batch_sizes_hold_both_sides_of_the_streams_per_wave():
    seen = set()
    for H in C.SMALL_H:
        S, B = C.streams_per_wave(H), C.small_batches(H)
        seen.add(S)
        assert S * C.padded_size(H) == C.WAVE and 0 not in B and B == tuple(sorted(set(B)))
        assert {1, S, S + 1, 2 * S + 1} <= set(B) and (S == 1 or S - 1 in B)
    assert seen == {1, 2, 4, 8}
    assert C.small_batches(8) == (1, 7, 8, 9, 17) and C.small_batches(33) == (1, 2, 3)
    assert C.WIDE_B == C.IO_B == (1, 3)
    assert C.lat_batches(C.MI355X_CUS) == (1, 3, 257) and C.lat_big_rows(C.MI355X_CUS) == (0, 128, 256)


def test_inputs_are_seeded_per_row_and_in_range():
    x, h0 = C.inputs("small", 8, 17, 193)
    assert x.dtype == h0.dtype == np.float32 and x.shape == (17, 193) and h0.shape == (17, 8)
    assert 0.6 < np.abs(x).max() <= 0.7 and 0.7 < np.abs(h0).max() <= 0.9
    x2, h2 = C.inputs("small", 8, (16, 3), 193)
    assert np.array_equal(x2, x[[16, 3]]) and np.array_equal(h2, h0[[16, 3]])
    x3, _ = C.inputs("small", 8, 2, 64)
    assert np.array_equal(x3, x[:2, :64])
    assert not np.array_equal(C.inputs("wide", 8, 1, 8)[0], x[:1, :8])


@pytest.mark.parametrize("H,HP", C.PAD_PAIRS + ((1, 8), (63, 64)))
def test_zero_padded_weights_give_the_unpadded_model_exactly(H, HP):
    """In fp64 and in fp32: y and h[:, :H] of the padded model are those of the unpadded one, and the padded units stay 0 --
    the claim the kernels' PAD forms rest on, here for the oracle's own order of summation."""
    sd = C.random_sd(H)
    sp = C.zero_padded(sd, HP)
    assert sp["GRU.weight_hh_l0"].shape == (3 * HP, HP) and sp["output.weight"].shape == (1, HP)
    for g in range(3):
        blk = sp["GRU.weight_hh_l0"][g * HP:(g + 1) * HP]
        assert np.array_equal(blk[:H, :H], sd["GRU.weight_hh_l0"][g * H:(g + 1) * H])
        assert not blk[H:].any() and not blk[:, H:].any()
        for k in ("GRU.weight_ih_l0", "GRU.bias_ih_l0", "GRU.bias_hh_l0"):
            assert not sp[k][g * HP + H:(g + 1) * HP].any() and np.array_equal(sp[k][g * HP:g * HP + H], sd[k][g * H:(g + 1) * H])
    assert not sp["output.weight"][0, H:].any()
    x, h0 = C.inputs("small" if H < 64 else "wide", H, 3, 70)
    hp0 = C.zero_padded_state(h0, HP)
    w, wp = oracle.Weights.from_state_dict(sd), oracle.Weights.from_state_dict(sp)
    for fwd in (oracle.gru_forward_f64, oracle.gru_forward):
        y, h = fwd(w, x, h0)
        yp, hp = fwd(wp, x, hp0)
        assert np.array_equal(y, yp) and np.array_equal(h, hp[:, :H])
        assert hp.shape == (3, HP) and not hp[:, H:].any()
        assert np.abs(y).max() > 1e-3


def test_segmented_references_equal_the_one_shot_run():
    """The carried state of the oracle is its whole state: segments that end at every T of the list give the bits of one run."""
    H = 16
    x, h0, ref = C.small_ref(H)
    w = oracle.Weights.from_state_dict(C.random_sd(H))
    y, h = oracle.gru_forward(w, x, h0)
    y64, h64 = oracle.gru_forward_f64(w, x, h0)
    T = max(C.TILE64_T)
    assert np.array_equal(ref.y32, y) and np.array_equal(ref.h32[T], h) and np.array_equal(ref.y64, y64) and np.array_equal(ref.h64[T], h64)
    y, h = oracle.gru_forward(w, x[:, :65], h0)
    assert np.array_equal(ref.y32[:, :65], y) and np.array_equal(ref.h32[65], h)
    sub = ref.rows([2, 0])
    assert np.array_equal(sub.y64, ref.y64[[2, 0]]) and np.array_equal(sub.h32[64], ref.h32[64][[2, 0]])


@pytest.mark.parametrize("H,I,O", C.IO_CASES)
def test_the_float64_io_reference_agrees_with_the_oracle(H, I, O):
    x, h0, ref = C.io_ref(H, I, O)
    assert ref.y32.shape == ref.y64.shape == (max(C.IO_B), max(C.TILE64_T) * O) and x.shape[1] == max(C.TILE64_T) * I
    print(f"io H={H} I={I} O={O}: E_ref y {ref.e_y:.2e} h {ref.e_h:.2e}")
    assert ref.e_y < C.GATE and ref.e_h < C.GATE                             # the existing gate
    assert max(ref.e_y, ref.e_h) <= C.E_REF_MAX
    # one shot == segments, in both precisions (torch carries its whole state too)
    sd = C.random_sd(H, I, O)
    y, h = C.io_forward_f64(sd, x, h0)
    assert np.abs(y - ref.y64).max() < 1e-14 and np.abs(h - ref.h64[max(C.TILE64_T)]).max() < 1e-14
    y, h = C.io_forward_f32(sd, x, h0)
    assert np.array_equal(y, ref.y32) and np.array_equal(h, ref.h32[max(C.TILE64_T)])


@pytest.mark.parametrize("H", (8, 65))
def test_the_float64_io_reference_at_size_one_is_gru_forward_f64(H):
    sd = C.random_sd(H)
    x, h0 = C.inputs("io", H, 3, 130)
    y, h = C.io_forward_f64(sd, x, h0)
    yo, ho = oracle.gru_forward_f64(oracle.Weights.from_state_dict(sd), x, h0)
    assert np.abs(y - yo).max() <= 1e-12 and np.abs(h - ho).max() <= 1e-12
    y32, h32 = C.io_forward_f32(sd, x, h0)
    assert np.abs(y32 - yo).max() < C.GATE and np.abs(h32 - ho).max() < C.GATE


def _check_e_ref(name, ref):
    print(f"E_REF {name}: y {ref.e_y:.2e} h {ref.e_h:.2e}")
    assert 0 < ref.e_y <= C.E_REF_MAX and 0 < ref.e_h <= C.E_REF_MAX, name
    assert np.abs(ref.y64).max() > 1e-3                                      # a live output: the ulp floor is not what carries the bar


@pytest.mark.parametrize("H", C.SMALL_H)
def test_the_fp32_oracle_is_within_a_quarter_of_the_gate_small(H):
    _check_e_ref(f"small H={H}", C.small_ref(H)[2])


@pytest.mark.parametrize("H", C.WIDE_H)
def test_the_fp32_oracle_is_within_a_quarter_of_the_gate_wide(H):
    _check_e_ref(f"wide H={H}", C.wide_ref(H)[2])


@pytest.mark.parametrize("weights", C.LAT_WEIGHTS)
def test_the_fp32_oracle_is_within_a_quarter_of_the_gate_lat(weights):
    """Rows 0 .. 2 (the small batches) and the three rows of the large batch at the MI355X's CU count; the GPU test repeats the
    check for the rows of the device it runs on."""
    rows = tuple(sorted(set(range(max(C.LAT_SMALL_B))) | set(C.lat_big_rows(C.MI355X_CUS))))
    _check_e_ref(f"lat {weights}", C.lat_ref(weights, rows)[2])
