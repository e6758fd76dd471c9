"""The exact-fp32 matrix-pipe GRU step (gru_mfma2_kernel, ENGINE 0) at the edges of its compile-time copies: kernel_variant
"mfma2" at the smallest batches it accepts -- 16 streams (one group), 17 (a ragged second group), 16 x (CUs + 1) (more groups
than CUs: the small-LDS build, YPN = 4) -- over the step counts of mfma2_step_cases.STEP_T, which reach steps 0-1, the phase-2,
phase-34 and phase-36 copies, both two-step loops and the run-time tail behind a whole tile.

Against the C oracle within 1e-5 (BASELINE.json north_star), and bit for bit against tests/golden/mfma2_step_bits.npz, recorded
by tools/make_goldens_mfma2_bits.py from the build BEFORE the step's LDS reads were spread over the MFMA gaps: a change of the
step's instruction order must not move a bit.  References are computed once per batch size at T_MAX (the GRU is causal: a shorter
run is the prefix) and shared."""
import functools

import numpy as np
import pytest
import torch

import oracle
from helpers import load, oracle_weights, rel_err
from mfma2_step_cases import CUTS, MANY_GROUPS_T, SMALL_B, STEP_T, T_MAX, inputs

pytestmark = pytest.mark.gpu

TOL = 1e-5
W_G = "GRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE]_BEST"
W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()       # raises if libntm.so is missing: no silent fallback
    return ntm_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model(ntm, variant="mfma2"):
    m = ntm.harness.build_model(W_G)
    m.kernel_variant = variant
    return m


def _run(m, x, h0):
    """forward from the state h0 -> (y (B, T) on the device, final state (B, 64) on the device)."""
    m.hidden = dev(h0).view(1, -1, 64)
    y = m.forward(dev(x).unsqueeze(1))[:, 0]
    return y, m.hidden[0].clone()


@functools.lru_cache(maxsize=None)
def _oracle(B):
    x, h0 = inputs(B)
    y, _ = oracle.gru_forward(oracle_weights(W_G), x, h0, threads=4)
    y.setflags(write=False)
    return y


def _many_groups():
    return 16 * (torch.cuda.get_device_properties(0).multi_processor_count + 1)


@pytest.mark.parametrize("T", STEP_T)
@pytest.mark.parametrize("B", SMALL_B)
def test_step_copies_against_oracle_and_recorded_bits(ntm, B, T):
    x, h0 = inputs(B, T)
    m = _model(ntm)
    y, _ = _run(m, x, h0)
    err = float(np.abs(y.cpu().numpy() - _oracle(B)[:, :T]).max())
    print(f"B={B} T={T}: max|y - oracle| = {err:.2e}")
    assert err < TOL
    g = load("mfma2_step_bits.npz")
    assert np.array_equal(y.cpu().numpy(), g[f"y_{B}"][:, :T])
    if T == T_MAX:
        assert np.array_equal(m.hidden[0].cpu().numpy(), g[f"h_{B}"])


@pytest.mark.parametrize("T", STEP_T)
@pytest.mark.parametrize("B", SMALL_B)
def test_one_input_tiled_over_all_streams_gives_identical_bits(ntm, B, T):
    """Every stream (every lane column, both groups) computes the same bits from the same input, and so do two launches."""
    x, h0 = inputs(B, T)
    xt, ht = np.repeat(x[:1], B, 0), np.repeat(h0[:1], B, 0)
    m = _model(ntm)
    y1, s1 = _run(m, xt, ht)
    y2, s2 = _run(m, xt, ht)
    assert torch.equal(y1, y2) and torch.equal(s1, s2)
    assert torch.equal(y1, y1[:1].expand_as(y1)) and torch.equal(s1, s1[:1].expand_as(s1))


def test_many_groups_build(ntm):
    """16 x (CUs + 1) streams, T = 130: the YPN = 4 build (two workgroups share a CU).  Scattered and edge streams against the
    oracle; the tiled input; two launches; chunked == one shot."""
    B, T = _many_groups(), MANY_GROUPS_T
    rng = np.random.default_rng(B + T)
    x = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)
    h0 = rng.uniform(-0.3, 0.3, (B, 64)).astype(np.float32)
    m = _model(ntm)
    y, s = _run(m, x, h0)
    rows = sorted({0, 15, 16, B // 2 + 1, B - 17, B - 16, B - 1})
    yo, ho = oracle.gru_forward(oracle_weights(W_G), x[rows], h0[rows], threads=4)
    err = float(np.abs(y[rows].cpu().numpy() - yo).max())
    print(f"B={B} T={T}: max|y - oracle| = {err:.2e}")
    assert err < TOL and float(np.abs(s[rows].cpu().numpy() - ho).max()) < TOL
    y2, s2 = _run(m, x, h0)
    assert torch.equal(y, y2) and torch.equal(s, s2)
    m.hidden = dev(h0).view(1, B, 64)
    c = (3, 64, T - 67)
    ys = [m.forward(dev(x[:, a:a + n]).unsqueeze(1))[:, 0] for a, n in zip(np.cumsum((0,) + c[:-1]), c)]
    assert torch.equal(torch.cat(ys, 1), y) and torch.equal(m.hidden[0], s)
    yt, st = _run(m, np.repeat(x[:1], B, 0), np.repeat(h0[:1], B, 0))
    assert torch.equal(yt, yt[:1].expand_as(yt)) and torch.equal(st, st[:1].expand_as(st))
    assert torch.equal(yt[0], y[0])


@pytest.mark.parametrize("B", SMALL_B)
def test_chunked_run_equals_one_shot(ntm, B):
    """T = 200 cut at 3 + 64 + 133: every chunk starts the kernel's step sequence anew from the carried state."""
    x, h0 = inputs(B)
    m = _model(ntm)
    y, s = _run(m, x, h0)
    m.hidden = dev(h0).view(1, B, 64)
    ys = [m.forward(dev(x[:, a:a + n]).unsqueeze(1))[:, 0] for a, n in zip(np.cumsum((0,) + CUTS[:-1]), CUTS)]
    assert torch.equal(torch.cat(ys, 1), y) and torch.equal(m.hidden[0], s)


def _esr_case(ntm, variant, B, T, x, h0):
    t = (0.3 * np.tanh(2 * x) + 0.02 * np.random.default_rng(B + T).standard_normal(x.shape)).astype(np.float32)
    m = _model(ntm, variant)
    y, s = _run(m, x, h0)
    for skip in (0, 64):
        if skip > T:         # no window [skip, T)
            continue
        m.hidden = dev(h0).view(1, B, 64)
        y1, sums = m.forward_esr(dev(x).unsqueeze(1), dev(t).unsqueeze(1), skip)
        assert torch.equal(y1[:, 0], y) and torch.equal(m.hidden[0], s)
        rows = sorted({0, B // 2, B - 1})
        so = oracle.esr_sums(y[rows].cpu().numpy(), t[rows], skip)
        r = float(rel_err(sums[rows].cpu().numpy(), so).max())
        print(f"{variant} B={B} T={T} skip={skip}: ESR sums rel err {r:.1e}")
        assert r <= 1e-9


@pytest.mark.parametrize("T", STEP_T)
@pytest.mark.parametrize("B", SMALL_B)
def test_forward_esr_same_bits_and_sums(ntm, B, T):
    """forward_esr: the y bits of forward; the per-stream sums against oracle.esr_sums to rel 1e-9, skip 0 and (T >= 64) 64."""
    x, h0 = inputs(B, T)
    _esr_case(ntm, "mfma2", B, T, x, h0)


@pytest.mark.parametrize("T", (3, 67, 200))
def test_forward_esr_in_the_recurrent_launch(ntm, T):
    """The same with the sums formed in the kernel's own tile flush (the ESR instantiation of the step: `auto` from 1025
    streams up); the first 16 streams carry the recorded case, whose bits they must reproduce."""
    B = 1040
    rng = np.random.default_rng(B + T)
    x = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)
    h0 = rng.uniform(-0.3, 0.3, (B, 64)).astype(np.float32)
    x[:16], h0[:16] = inputs(16, T)
    _esr_case(ntm, "auto", B, T, x, h0)
    y, _ = _run(_model(ntm, "auto"), x, h0)
    assert np.array_equal(y[:16].cpu().numpy(), load("mfma2_step_bits.npz")["y_16"][:, :T])


@pytest.mark.parametrize("T", STEP_T)
def test_fused_diffdel_step_equals_two_pass(ntm, T):
    """The FUSE instantiation of the step (delay line in the tile housekeeping) at 16 streams, D = 5: y, pre_d, the carried
    state and the delay buffer equal the GRU launch + streaming delay pass bit for bit."""
    B, D = 16, 5
    x, h0 = inputs(B, T)
    rng = np.random.default_rng(T)
    d = rng.uniform(0.0, D - 0.01, (B, T)).astype(np.float32)
    b0 = rng.uniform(-0.3, 0.3, (B, D)).astype(np.float32)
    res = {}
    for mode in ("two_pass", "fused"):
        m = ntm.DiffDelRNN(1, 64, 1, max_delay=D - 1)
        m.load_state_dict(ntm.weights.load_state_dict(W_D))
        m = m.to("cuda").eval()
        m.delay_mode = mode
        if mode == "two_pass":
            m.kernel_variant = "mfma2"      # the same GRU kernel as the fused step
        m.initialize_hidden(B, D - 1)
        m.hidden, m.diffdel.buffer = dev(h0).view(1, B, 64), dev(b0).view(B, 1, D)
        y, pre = m(dev(x).unsqueeze(1), dev(d).unsqueeze(1))
        res[mode] = (y.clone(), pre.clone(), m.hidden.clone(), m.diffdel.buffer.clone())
    for a, b, what in zip(res["two_pass"], res["fused"], ("y", "pre_d", "hidden", "buffer")):
        assert torch.equal(a, b), what
