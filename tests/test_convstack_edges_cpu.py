"""CPU: the cases of tests/test_gpu_convstack_edges.py are what they claim to be.  Every table row sits on the edge it names (the
chunk rules recomputed in tests/convstack_edge_cases.py, and the library's own workspace size at the same B); every exact case
meets the exactness condition per tensor (the sum of magnitudes of every accumulation below 2^24 units, float32 autograd equal
to float64 autograd elementwise) and leaves no (input channel, tap) position zero in every row; the float32 and float64 twins of
every dense case agree on every LeakyReLU side; the dv tensors that leave the `==` instrument are exactly the listed ones; and
the float32 emulation of the weight gradient's documented order is within the bar of the float64 twin."""
import numpy as np
import pytest
import torch

import melgan_cases as mel
from convstack_edge_cases import (CHANNELS, DV_INEXACT, EXACT_BITS, FRAMES, ORDER, PARTIAL_COUNTS, STREAM_BS, STREAM_RULES, THINNED, R, case,
                                  cases, covered_positions, e32, emulate_order, exact_bits, frames, groups, layer_rule, library_workspace_floats,
                                  may_leave, named, partials, pre_activations, reference, row_length, row_recipe, rules, sides_agree,
                                  stream_chunks, workspace_floats)


def test_the_stream_rule_by_hand():
    assert {B: stream_chunks(B) for B in STREAM_BS} == STREAM_RULES
    assert stream_chunks(1) == (1, 1) and stream_chunks(0) == (0, 1) and stream_chunks(96) == (32, 3) and stream_chunks(97) == (25, 4)
    # the ragged last chunk: 33 = 16 x 2 + 1, 65 = 21 x 3 + 2
    assert 33 - 16 * 2 == 1 and 65 - 21 * 3 == 2


def test_every_row_against_the_mirror_and_the_library():
    for c in cases() + (ORDER,):
        assert library_workspace_floats(c) == workspace_floats(c), c.id
        if c.fam != "mel":
            assert all(r[:2] == stream_chunks(c.B) for r in rules(c)), c.id


def test_the_stream_rows_are_the_edges_they_name():
    for fam in ("dil", "spc"):
        rows = [c for c in cases() if c.fam == fam and c.group == "streams"]
        assert {c.B for c in rows if c.kind == "exact"} == set(STREAM_BS) and {c.B for c in rows if c.kind == "dense"} >= {33, 65}
        for c in rows:
            Fr = frames(fam, c.F0, c.spec)
            assert all(r[:2] == STREAM_RULES[c.B] for r in rules(c)) and max(s[1] for s in c.spec) <= 64, c.id
            assert Fr[-1] <= 300 or c.id == "dil-streams-B33-F1025-exact", c.id
            # a segment whose steps per stream are no multiple of kSub: a chain of sub-sums continues across a stream boundary
            if c.B > 32 and fam == "dil":
                assert any(mel.cdiv(min(f, s0 + 1024) - s0, 64) % 4 for f in Fr[1:] for s0 in range(0, f, 1024)), c.id
    c = case("dil-streams-B33-F1025-exact")
    assert frames("dil", c.F0, c.spec)[-1] == 1025 and rules(c)[-1] == (17, 2, 2)
    # MelGAN: the `need` term at B = 5 (2048 / 700 -> 3 streams per partial, ragged), ceil(B / 32) at 65 (3 > need = 2); at
    # B = 33 the two terms are both 2
    c = case("mel-streams-B5-F700-exact")
    assert frames("mel", c.F0, c.spec)[1] == 700 and rules(c)[0] == (2, 3, 1) and c.spec[0][6] == R
    for B, term in ((33, 2), (65, 3)):
        c = case(f"mel-streams-B{B}-F2048-exact")
        assert frames("mel", c.F0, c.spec)[1] == 2048 and mel.cdiv(B, 32) == term and mel.cdiv(2048, 1024) == 2
        assert rules(c)[0] == (mel.cdiv(B, term), term, 2), c.id
    assert case("mel-streams-B65-F2048-dense").B == 65
    # the 2^24-float cap (planner only): 1024 x 1024 x 8 = 2^23 weights, 4 streams of 2048 frames -> two segments of 2^23 floats
    # are the whole allowance, so ONE partial per segment takes all four streams although ceil(B / 32) = 1 and need = 2
    W = 1024 * 1024 * 8
    assert mel.chunk_rule(4, 2048, W) == (1024, 2, 4, 1) and layer_rule("mel", 4, 2048, W) == (1, 4, 2)
    assert mel.chunk_rule(4, 2048, W // 2) == (1024, 2, 2, 2)                       # half the weights: need = 2 binds again
    assert mel.chunk_rule(4, 2048, 2 * W) == (2048, 1, 4, 1)                        # twice: the segment doubles first
    import ntm_amd
    ws = ntm_amd._lib.lib().ntm_sconvstack_workspace_floats(4, 1024, 2048 + 7, 1, ntm_amd._lib.conv_layers_s(((1024, 1024, 8, 1, 1, 0, 0),)))
    assert ws == 2 * 4 * 1024 * 2048 + 2 * (W + 1024)


def test_the_frame_rows_are_the_edges_they_name():
    for fam, want in (("dil", FRAMES), ("spc", FRAMES[:9]), ("mel", FRAMES)):
        rows = [c for c in cases() if c.fam == fam and c.group == "frames" and c.kind == "exact"]
        assert all(len(c.spec) == 1 for c in rows)
        got = {}
        for c in rows:
            got.setdefault(frames(fam, c.F0, c.spec)[1], []).append(c)
        assert tuple(sorted(got)) == want
        for Fo, cs in got.items():
            assert {c.spec[0][1] <= 16 for c in cs} == {True, False}, (fam, Fo)              # both tile forms
            if fam == "mel":                                                                  # strides 2, 3, 4, with and without a remainder
                assert {(c.spec[0][4], (c.F0 + 2 * c.spec[0][5] - c.spec[0][2]) % c.spec[0][4] > 0) for c in cs} == {(s, r) for s in (2, 3, 4) for r in (False, True)}
    assert set(FRAMES) >= {64 - 1, 64, 64 + 1, 128 - 1, 128, 128 + 1, 256 - 1, 256, 256 + 1, 1024 - 1, 1024, 1024 + 1, 2049}


def test_the_channel_rows_are_the_edges_they_name():
    cg = lambda l: (l[0] // l[3], l[1] // l[3])
    assert {cg(l)[1] for l in CHANNELS} >= {1, 15, 16, 17, 64, 65} and {cg(l)[0] for l in CHANNELS} >= {15, 16, 17}
    assert {cg(l)[0] * l[2] for l in CHANNELS} >= {63, 64, 65} and {l[2] for l in CHANNELS} == {1, 3, 4, 5} and {l[3] for l in CHANNELS} == {1, 4}
    for fam in ("dil", "spc", "mel"):
        rows = [c.spec[0][:4] for c in cases() if c.fam == fam and c.group == "channels" and c.kind == "exact" and len(c.spec) == 1]
        assert set(rows) >= set(CHANNELS), fam
    # the strided family's dot kernel, forward (64 x 5 indices) and in the data gradient (64 channels x 3 taps of a phase)
    assert case("mel-channels-dot-64x1-exact").spec[0][:3] == (64, 1, 5) and case("mel-channels-dot-1x64-exact").spec[0][:3] == (1, 64, 5)


def test_the_partial_counts():
    for fam in ("dil", "spc", "mel"):
        counts = {partials(c)[0] for c in cases() if c.fam == fam and c.group == "partials"}
        assert counts >= set(PARTIAL_COUNTS), (fam, counts)
    # ... and counts that are 2 mod 4, where the remainder loop of stack_wnorm_kernel takes exactly one partial
    assert any(p % 4 == 2 for c in cases() for p in partials(c))


def test_rows_of_v():
    assert row_recipe(9)[0] == 1 and row_recipe(8) == (0, 7, 0, 1, 2) and row_recipe(4) == (0, 4, 0, 0, 1) and row_recipe(1) == (0, 1, 0, 0, 0)
    assert all(row_recipe(n)[0] == 0 for n in (5, 17, 45, 60, 63, 64, 65, 85))


@pytest.mark.parametrize("fam,group", groups("exact"))
def test_exact_cases_meet_the_exactness_condition(fam, group):
    """Per tensor: the sum of magnitudes of every accumulation behind it, in units of the operands' last place, is below 2^24
    (float64, absolute values), and float32 autograd equals float64 autograd elementwise.  A dv with rows longer than 64 may miss
    the condition, and then it is listed in DV_INEXACT -- which holds nothing else."""
    ran = 0
    for c in cases():
        if (c.fam, c.group, c.kind) != (fam, group, "exact"):
            continue
        inputs, r64, r32 = reference(c.id)
        bits = exact_bits(c, inputs)
        n64, n32 = named(c, r64), named(c, r32)
        assert set(n64) <= set(bits) and covered_positions(inputs[1]), c.id
        left = {k for k in n64 if not (bits[k] < EXACT_BITS and np.array_equal(n64[k], n32[k]))}
        assert all(b < EXACT_BITS for k, b in bits.items() if k not in n64), (c.id, bits)          # the inner pre-activations
        assert left == set(DV_INEXACT.get(c.id, ())) and left <= may_leave(c), (c.id, left, {k: bits[k] for k in left})
        assert all(float(np.abs(a).max()) > 0 for a in n64.values()), c.id
        if fam == "spc":
            assert c.par == 0.0 and len(c.spec) <= 2
            if len(c.spec) == 2:
                assert pre_activations(c, inputs[0], inputs[1], torch.float64)[0].min() > 0, c.id
        else:
            assert c.par == 0.5
        print(f"{c.id}: most bits {max(bits.values()):.1f} ({max(bits, key=bits.get)}), one gradient entry of {THINNED[c.id]}")
        ran += 1
    assert ran > 0


def test_the_dv_exceptions():
    """No dv of this table leaves instrument 1: the rows of 65, 85 and 320 entries meet the condition too."""
    assert DV_INEXACT == {}
    assert {row_length(c, 0) for c in cases() if c.kind == "exact" and may_leave(c)} == {65, 85, 320}


@pytest.mark.parametrize("fam", ["dil", "spc", "mel"])
def test_dense_cases_agree_on_every_leaky_relu_side(fam):
    rows = [c for c in cases() if c.fam == fam and c.kind == "dense"]
    assert len(rows) >= 10 and any(len(c.spec) == 3 for c in rows)                  # the mask path is on in three-layer stacks
    for c in rows + ([ORDER] if fam == "dil" else []):
        assert sides_agree(c, reference(c.id)[0]), c.id
    print(fam, "E32:", {k: f"{v:.2e}" for k, v in e32(fam).items()})
    assert set(e32(fam)) == {"out", "gx", "dg", "dv", "dbias"}
    if fam == "spc":
        assert any(c.par > 0 for c in rows) and any(c.par == 0 for c in rows)      # with and without the log head


def test_the_order_case_and_its_emulation():
    """B = 65, two segments; the emulation of the documented order in float32 is within the bar of the float64 twin, and is not
    the float32 twin bit for bit (the order is visible in this case)."""
    assert rules(ORDER) == [(22, 3, 2)] and frames("dil", ORDER.F0, ORDER.spec)[1] == 1030
    inputs, r64, r32 = reference(ORDER.id)
    emu, n64, n32 = emulate_order(ORDER, inputs), named(ORDER, r64), named(ORDER, r32)
    for name, a in emu.items():
        kind = name.split("[")[0]
        bar = 4.0 * np.maximum(np.abs(n32[name] - n64[name]), e32("dil")[kind] * np.abs(n64[name]).max())
        assert (np.abs(a - n64[name]) <= bar).all(), name
    assert any(not np.array_equal(emu[name], n32[name]) for name in emu)
