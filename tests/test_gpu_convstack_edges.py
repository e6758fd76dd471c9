"""GPU: the three critic conv stacks (csrc/critic_kernels.hip, convstack_kernels.hip, sconv_kernels.hip over convstack_common.h)
above 32 streams and at the chunk, segment and tile edges -- the shapes tests/test_gpu_critic.py, test_gpu_convstack.py and
test_gpu_melgan.py leave unrun (last paragraph).  The tables, both constructions and the mirrors of the chunk
rules are in tests/convstack_edge_cases.py; tests/test_convstack_edges_cpu.py asserts on the CPU that every row is the edge it
names and that every case meets the condition of its instrument.

Two instruments.  EXACT cases (integer data, |v| a power of two, slope 1/2: every sum is a float32 number in any order) are
compared with `==` against the float64 twin: out, gx, dg, dv and dbias of every layer, no exception (no dv of this table left
the instrument, rows of 65, 85 and 320 entries included).  DENSE cases are held to the existing bar,
4 max(|ref32 - ref64|, E32(kind) max|ref64|), E32 over this table's own dense cases per family; the two twins agree on every
LeakyReLU side in all of them, so this is the tight form of the bar.

What the tables cover: B in {31, 32, 33, 64, 65} (per = 1, 2, 3; ragged last chunks of one and two streams; sub-sum chains that
cross a stream boundary), B = 33 at 1025 frames, the MelGAN rule at B = 5 (need), 33 and 65 (ceil(B / 32)); 63 .. 2049 output
frames around 64, 128, 256, 1024 on both tile forms (MelGAN: strides 2, 3, 4 with and without a remainder); cout_g in {1, 15, 16,
17, 64, 65}, cin_g in {15, 16, 17}, rows of 63, 64, 65, k in {1, 3, 4, 5}, groups in {1, 4}, the dot kernel; 1, 4, 5, 8, 9 partials;
NULL gx / dg at B = 33; stream independence at B = 65; the order of the weight-gradient join against a float32 emulation.

Measured on an MI355X ("Edges of the three conv stacks"):
    exact cases (dil 50, spc 38, mel 98)   every tensor of every case equal to the float64 twin bit for bit; no dv exception
    dense, worst |got - ref64| / bar       dil (16 cases)  out 0.24  gx 0.27  dg 0.13  dv 0.15  dbias 0.06
                                           spc (14 cases)  out 0.28  gx 0.31  dg 0.26  dv 0.25  dbias 0.30
                                           mel (21 cases)  out 0.25  gx 0.22  dg 0.21  dv 0.07  dbias 0.07
    order case                             dg 3 of 3, dbias 3 of 3, dv 18 of 18 elements equal the emulation bit for bit (the
                                           float32 twin: none of them); printed, not asserted
    run time                               this file 4.4 - 5.0 s (29 tests), tests/test_convstack_edges_cpu.py 4.9 s (24 tests)
No defect was found: the kernels are as they were."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_convstack as dil
import test_gpu_critic as spc
import test_gpu_melgan as melgpu
from convstack_edge_cases import DV_INEXACT, KINDS, MODS, ORDER, case, cases, e32, emulate_order, groups, kind_of, named, reference, rules, tensors

RUN = {"dil": dil.run_raw, "spc": spc.run_raw, "mel": melgpu.run_raw}


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def run(ntm, c, inputs, **kw):
    """The family's raw forward + backward (every device buffer starts as NaN)."""
    x, params, gout = inputs
    return RUN[c.fam](ntm, x, params, c.spec, c.par, gout, **kw)


@functools.lru_cache(maxsize=None)
def device_result(ntm, cid):
    c = ORDER if cid == ORDER.id else case(cid)
    return run(ntm, c, reference(cid)[0])


def one_stream(c, inputs, s):
    x, params, gout = inputs
    return x[s:s + 1], params, ([g[s:s + 1] for g in gout] if c.fam == "mel" else gout[s:s + 1])


def same(c, a, b):
    ta, tb = tensors(c, a), tensors(c, b)
    return len(ta) == len(tb) and all(np.array_equal(u, v, equal_nan=False) for (_, _, u), (_, _, v) in zip(ta, tb))


def bar_ratio(got, a64, a32, e):
    bar = 4.0 * np.maximum(np.abs(a32 - a64), e * float(np.abs(a64).max()))
    return float((np.abs(np.asarray(got, np.float64) - a64) / bar).max())


# ---- instrument 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fam,group", groups("exact"))
def test_exact_cases_equal_the_float64_twin_bit_for_bit(ntm, fam, group):
    bad, ran = [], 0
    for c in cases():
        if (c.fam, c.group, c.kind) != (fam, group, "exact"):
            continue
        _, r64, r32 = reference(c.id)
        got, n32 = named(c, device_result(ntm, c.id)), named(c, r32)
        for name, a64 in named(c, r64).items():
            g = np.asarray(got[name], np.float64).reshape(a64.shape)
            if name in DV_INEXACT.get(c.id, ()):
                ratio = bar_ratio(g, a64, n32[name], e32(fam)["dv"])
                print(f"{c.id} {name}: float bar, worst err / bar {ratio:.3f}")
                if not ratio <= 1.0:
                    bad.append((c.id, name, ratio))
                continue
            miss = ~(g == a64)
            if miss.any():
                at = tuple(int(i) for i in np.argwhere(miss)[0])
                bad.append((c.id, name, int(miss.sum()), miss.size, at, float(g[at]), float(a64[at])))
                print("MISMATCH (case, tensor, elements off, of, first index, got, want):", bad[-1])
        ran += 1
    print(f"{fam} {group}: {ran} exact cases, {len(bad)} tensors off")
    assert ran > 0 and not bad, bad[:8]


# ---- instrument 2 --------------------------------------------------------------------------------------------------------------
def dense_worst(ntm, fam, group=None):
    worst = {}
    for c in cases():
        if c.fam == fam and c.kind == "dense" and group in (None, c.group):
            _, r64, r32 = reference(c.id)
            for k, v in MODS[fam].check_result(device_result(ntm, c.id), r64, r32, e32(fam), c.id).items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("fam,group", groups("dense"))
def test_dense_cases_against_float64(ntm, fam, group):
    print("E32:", {k: f"{v:.2e}" for k, v in e32(fam).items()})
    worst = dense_worst(ntm, fam, group)
    assert set(worst) == set(KINDS)
    print(f"WORST dense {fam} {group}:", {k: f"{v:.3f}" for k, v in worst.items()})


# ---- streams, flags, repeats ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["dil-streams-B65-dense", "spc-streams-B65-dense", "mel-streams-B65-F2048-dense"])
def test_equal_calls_equal_bits_and_streams_0_63_64_do_not_depend_on_their_batch(ntm, cid):
    """B = 65 is 22 chunks of 3 (MelGAN: of 3 by ceil(B / 32)): stream 63 opens the last, ragged chunk, stream 64 closes it."""
    c, inputs = case(cid), reference(cid)[0]
    a, b = device_result(ntm, cid), run(ntm, c, inputs)
    assert same(c, a, b) and all(np.isfinite(t).all() for _, _, t in tensors(c, a))
    fa = named(c, a)
    for s in (0, 63, 64):
        one = named(c, run(ntm, c, one_stream(c, inputs, s), want_pg=False))
        assert set(one) == {k for k in fa if kind_of(k) in ("out", "gx")}
        for name, t in one.items():
            assert np.array_equal(t, fa[name][s:s + 1]), (cid, s, name)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["dil-streams-B33-dense", "spc-streams-B33-head-dense", "mel-streams-B33-F2048-exact"])
def test_null_gx_and_null_dg_give_the_bits_of_the_full_call_at_33_streams(ntm, cid):
    c, inputs = case(cid), reference(cid)[0]
    a = device_result(ntm, cid)
    no_gx = run(ntm, c, inputs, want_gx=False)
    assert no_gx["gx"] is None and same(c, no_gx, dict(a, gx=None))
    no_pg = run(ntm, c, inputs, want_pg=False)
    assert "dg" not in no_pg and same(c, no_pg, {k: v for k, v in a.items() if k in ("out", "gx")})


# ---- the order of the weight-gradient join ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_weight_gradient_join_follows_the_documented_order(ntm):
    """One dense dilated layer at B = 65 and 1030 output frames (22 chunks x 2 segments = 44 partials): dg, dv and dbias against a
    float32 emulation in numpy of the documented order -- the streams of a chunk in order, steps of 64 frames, a join every four
    steps and at the tail, the partials chunk-major and segment-minor, <dW, v> in the tree of block_sum -- to within the float64
    bar of this case.  How many elements equal the emulation bit for bit is PRINTED, not asserted: the MFMA's inner order is not
    documented."""
    assert rules(ORDER) == [(22, 3, 2)]
    inputs, r64, r32 = reference(ORDER.id)
    got, n64, n32 = named(ORDER, device_result(ntm, ORDER.id)), named(ORDER, r64), named(ORDER, r32)
    MODS["dil"].check_result(device_result(ntm, ORDER.id), r64, r32, e32("dil"), ORDER.id)
    for name, emu in emulate_order(ORDER, inputs).items():
        bar = 4.0 * np.maximum(np.abs(n32[name] - n64[name]), e32("dil")[kind_of(name)] * float(np.abs(n64[name]).max()))
        g = got[name].reshape(emu.shape)
        err = np.abs(g.astype(np.float64) - emu.astype(np.float64))
        print(f"order {name}: {int((g == emu).sum())} of {emu.size} elements equal the emulation bit for bit "
              f"(the float32 twin: {int((n32[name].astype(np.float32).reshape(emu.shape) == g).sum())}); worst |got - emulation| / bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all(), name


@pytest.mark.gpu
def test_worst_ratios_per_tensor_kind_and_family(ntm):
    """Prints the worst |got - ref64| / bar of the dense table per family (what the docstring and DESIGN.md 11.8 record)."""
    for fam in ("dil", "spc", "mel"):
        worst = dense_worst(ntm, fam)
        n = sum(1 for c in cases() if c.fam == fam and c.kind == "dense")
        print(f"WORST {fam}, {n} dense cases:", {k: f"{worst[k]:.3f}" for k in KINDS})
        assert set(worst) == set(KINDS) and max(worst.values()) <= 1.0
    print("exact cases:", {fam: sum(1 for c in cases() if c.fam == fam and c.kind == "exact") for fam in ("dil", "spc", "mel")})
