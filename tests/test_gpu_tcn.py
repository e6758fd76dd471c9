"""GPU: the TCN forward (csrc/tcn_kernels.hip) at the edges its code has -- tile counters, window limits, the ring of the
phase-group kernel, the fused output conv, the rows at and behind T -- against float64 with NO tolerance.

A. Exact-integer networks (tests/tcn_cases.py): every table row as the last block (fused output conv) and as an inner block
   (activation written, read back through the probe), from a scratch full of NaN; `==` against float64.
B. Streams are independent and a repeated call gives the same bits.
C. PReLU / bias placement in arbitrary floats: one rounding per step, expected values computed in numpy float32, `==`.
D. Dense float networks against float64, bar = 3 x the float32 C oracle's own distance on the case."""
import copy

import numpy as np
import pytest
import torch

from tcn_cases import (C, DENSE, FIRST, FIRST_D1, K, PG, POLY, REPEAT_ROWS, assert_exact, dense_case, exact_case, first_mismatch,
                       poisoned_scratch, probe, rel_err, row_id)

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def on_device(model):
    return copy.deepcopy(model).to("cuda")


def run(model_dev, x_dev, poison=NAN):
    """One forward from a scratch of exactly the size the library asks for, filled with `poison`; -> [B, T] on the device."""
    B, T = x_dev.shape[0], x_dev.shape[2]
    s = poisoned_scratch(model_dev, B, T, poison)
    y = model_dev(x_dev)
    assert model_dev._scratch is s, "forward() replaced the scratch it was given"
    return y[:, 0, :]


def run_last(model, x, poison=NAN):
    return run(on_device(model), x.cuda(), poison).cpu()


def run_inner(model, x, poison=NAN):
    """The [B, T, 32] activation of the model's last block, computed as an inner block (32 runs through the probe)."""
    xd = x.cuda()
    return probe(model, lambda pm: run(pm, xd, poison), place=lambda pm: pm.to("cuda")).cpu()


def check(got, want, what):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    bad = first_mismatch(got, want)
    assert bad is None, (f"{what}: device != float64 first at index (stream, sample[, channel]) {bad[0]}: got {bad[1]!r}, "
                         f"want {bad[2]!r}; {bad[3]} of {want.numel()} differ")


# ---- A. exact cases, zero tolerance ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", FIRST_D1 + FIRST, ids=row_id)
def test_first_block_exact(ntm, row):
    """tcn_first_d1_kernel (d = 1) and tcn_first_kernel, read through the probe directly behind block 1."""
    d, T, _ = row
    m, x, _, acts, bounds = exact_case((d,), T)
    assert_exact(bounds)
    check(run_inner(m, x), acts[0], f"first block d={d} T={T}")


@pytest.mark.parametrize("row", POLY + PG, ids=row_id)
def test_block_exact_as_last_block(ntm, row):
    """dilations (1, d): the block kernel with the fused output conv; y == float64."""
    d, T, _ = row
    m, x, y64, _, bounds = exact_case((1, d), T)
    assert_exact(bounds)
    check(run_last(m, x), y64, f"last block d={d} T={T}")


@pytest.mark.parametrize("row", POLY + PG, ids=row_id)
def test_block_exact_as_inner_block(ntm, row):
    """dilations (1, d) plus the probe: the block kernel writes its activation; all 32 channels == float64."""
    d, T, _ = row
    m, x, _, acts, bounds = exact_case((1, d), T)
    assert_exact(bounds)
    check(run_inner(m, x), acts[1], f"inner block d={d} T={T}")


@pytest.mark.parametrize("dilations,T", [((1, 7, 3), 300), ((1, 600, 2), 1500), ((1, 10, 100, 1000), 2100)], ids=lambda v: str(v))
def test_deep_exact_networks(ntm, dilations, T):
    """Three and four blocks (inner polyphase / phase-group blocks feeding further blocks), y == float64."""
    m, x, y64, _, bounds = exact_case(dilations, T)
    assert_exact(bounds)
    check(run_last(m, x), y64, f"{dilations} T={T}")


@pytest.mark.parametrize("kernel", list(REPEAT_ROWS))
def test_the_result_does_not_depend_on_what_the_scratch_held(ntm, kernel):
    """NaN, 0.0 and 1e30 in every row at and behind T, in the padding and in the other activation buffer: the same bits."""
    d, T = REPEAT_ROWS[kernel]
    first = kernel.startswith("first")
    m, x, y64, acts, _ = exact_case((d,) if first else (1, d), T)
    roles = [("inner", run_inner, acts[-1])] + ([] if first else [("last", run_last, y64)])
    for role, fn, want in roles:
        got = [fn(m, x, poison) for poison in (NAN, 0.0, 1e30)]
        check(got[0], want, f"{kernel} {role} d={d} T={T}")
        assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]), f"{kernel} {role}: the output depends on stale scratch"


# ---- B. streams are independent ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", list(REPEAT_ROWS))
def test_streams_are_independent_and_calls_repeat(ntm, kernel):
    d, T = REPEAT_ROWS[kernel]
    first = kernel.startswith("first")
    m, x, y64, acts, bounds = exact_case((d,) if first else (1, d), T, 3)
    assert_exact(bounds)
    assert not torch.equal(x[0], x[1]) and not torch.equal(x[1], x[2])
    roles = [("inner", run_inner, acts[-1])] + ([] if first else [("last", run_last, y64)])
    for role, fn, want in roles:
        got = fn(m, x)
        check(got, want, f"{kernel} {role} B=3 d={d} T={T}")
        assert torch.equal(fn(m, x), got), f"{kernel} {role}: a repeated call gave other bits"
        for i in range(3):
            assert torch.equal(fn(m, x[i:i + 1]), got[i:i + 1]), f"{kernel} {role}: stream {i} alone differs from stream {i} of 3"


# ---- C. PReLU and bias placement, exact in floats -------------------------------------------------------------------------------
def float_inputs(B, T, seed):
    """Exact zeros and magnitudes from 1e-30 to 1e30, both signs; no subnormal, no infinity."""
    rng = np.random.default_rng(seed)
    x = (rng.choice([-1.0, 1.0], (B, T)) * 10.0 ** rng.uniform(-30, 30, (B, T))).astype(np.float32)
    x[rng.random((B, T)) < 0.05] = 0.0
    x[0, :4] = [1e30, -1e30, 1e-30, -1e-30]
    return x


def slopes_and_gains(seed):
    """32 distinct slopes -- 0, 1, above 1, negative, non-dyadic -- and 32 gains; |.| in [1e-3, 3] or 0, so that no product of
    an input of 1e-30 or 1e30 with them is subnormal or infinite."""
    rng = np.random.default_rng(seed)
    al = np.concatenate([[0.0, 1.0, -1.0, 1.5, 2.5, -0.3, 0.1, 0.001, -1.7, 1.0 / 3.0], rng.uniform(-2, 2, C - 10)]).astype(np.float32)
    assert len(set(al.tolist())) == C and all(a == 0 or 1e-3 <= abs(a) <= 3 for a in al.tolist())
    r = (rng.choice([-1.0, 1.0], C) * rng.uniform(0.25, 3.0, C)).astype(np.float32)
    return rng.permutation(al), r


OUT_BIAS = np.float32(0.7)


def expected_prelu(u, al):
    """numpy float32: u >= 0 ? u : float32(alpha u), then + out_bias (one rounding each)."""
    assert u.dtype == np.float32 and al.dtype == np.float32
    v = np.where(u >= 0, u, (al[None, None, :] * u).astype(np.float32)).astype(np.float32)
    return (v + OUT_BIAS).astype(np.float32)


def run_channels(m, x):
    """y for every one-hot output conv with out_bias = OUT_BIAS: [B, T, 32] float32 numpy."""
    md, xd = on_device(m), torch.from_numpy(x).cuda().unsqueeze(1)
    cols = []
    for c in range(C):
        with torch.no_grad():
            md.out_weight.zero_()
            md.out_weight[0, c, 0] = 1.0
            md.out_bias.fill_(float(OUT_BIAS))
        cols.append(run(md, xd))
    return torch.stack(cols, dim=-1).cpu().numpy()


def check_floats(got, want, what):
    assert np.isfinite(want).all() and not ((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)).any()
    bad = np.argwhere(~(got == want))
    assert len(bad) == 0, (f"{what}: first differing (stream, sample, channel) {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, "
                           f"want {want[tuple(bad[0])]!r}; {len(bad)} of {want.size} differ")


@pytest.mark.parametrize("d", [3, 600])
def test_prelu_and_bias_placement_in_floats(ntm, d):
    """Block 1: W = 0, bias = 0, R[c] = r_c: its activation is float32(r_c x).  Block 2 (polyphase for d = 3, phase-group for
    d = 600, fused output conv): an identity tap, bias = 0, R = 0, slope alpha_c: prelu_plus must give `u >= 0 ? u : alpha u`
    with the slope of ITS channel, and the epilogue adds out_bias once."""
    B, T = 2, 650
    x = float_inputs(B, T, 40 + d)
    al, r = slopes_and_gains(d)
    m = ntm.TCN(dilations=(1, d))
    with torch.no_grad():
        m.conv_weight[0].zero_(); m.conv_bias[0].zero_(); m.res_weight[0].copy_(torch.from_numpy(r)[:, None, None])
        m.conv_weight[1].zero_(); m.conv_bias[1].zero_(); m.res_weight[1].zero_()
        for c in range(C):
            m.conv_weight[1][c, c, K - 1] = 1.0
        m.prelu[1].copy_(torch.from_numpy(al))
    u = (r[None, None, :] * x[:, :, None]).astype(np.float32)
    check_floats(run_channels(m, x), expected_prelu(u, al), f"(1, {d})")


@pytest.mark.parametrize("d", [1, 3])
def test_single_block_network_in_floats(ntm, d):
    """dilations (d,): tcn_first_d1_kernel / tcn_first_kernel and tcn_out_kernel.  One tap w_c at the sample itself, bias = 0,
    R = 0: u = float32(w_c x), PReLU with the channel's slope, then out_bias."""
    B, T = 2, 300
    x = float_inputs(B, T, 50 + d)
    al, w = slopes_and_gains(10 + d)
    m = ntm.TCN(dilations=(d,))
    with torch.no_grad():
        m.conv_weight[0].zero_(); m.conv_bias[0].zero_(); m.res_weight[0].zero_()
        m.conv_weight[0][:, 0, K - 1] = torch.from_numpy(w)
        m.prelu[0].copy_(torch.from_numpy(al))
    u = (w[None, None, :] * x[:, :, None]).astype(np.float32)
    check_floats(run_channels(m, x), expected_prelu(u, al), f"({d},)")


# ---- D. dense float cases against float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dilations,T,amp", DENSE, ids=lambda v: str(v))
def test_dense_networks_against_float64(ntm, dilations, T, amp):
    m, x, y64, bar = dense_case(dilations, T, amp)
    got = run_last(m, x)
    assert bool(torch.isfinite(got).all())
    err = rel_err(got, y64)
    print(f"TCN dense {dilations} T={T} amp={amp}: err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
    assert err <= bar, (err, bar)
