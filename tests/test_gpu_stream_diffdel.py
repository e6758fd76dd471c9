"""GPU: DiffDelRNN block by block through harness.BlockStreamer -- ntm_diffdel_stream_block (csrc/diffdel_stream.hip: the
low-latency recurrence and the delay line on a per-stream ring, one launch per block), the ring's seed / export entries, graph
replay, the fallback for other hidden sizes and the argument checks.

The reference throughout is the model's own forward() called block by block in the same process, with kernel_variant "lat" and
delay_mode "two_pass" (ntm_gru_forward_ex + ntm_delay_forward, pinned to the reference implementation by tests/test_gpu_parity.py
and tests/test_gpu_round3.py).  Both sides are built from csrc/gru_lat_step.h and csrc/delay_math.h, so every comparison is
equality of bits (torch.equal): a difference is a wrong index, a missed wrap of the ring or a restated formula.

A DiffDelRNN built with max_delay = D carries a delay line of D + 1 samples (initialize_hidden, as in the reference); that length
is what the kernel and the C ABI call D, and BlockStreamer.D holds it."""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

W_G = "GRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE]_BEST"
W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def _model(ntm, D, H=64):
    """A fresh DiffDelRNN(1, H, 1, max_delay=D): the shipped checkpoint for H = 64 on the low-latency kernel and the two-pass
    delay line, seeded random parameters otherwise; the range assert deferred, as every block-by-block caller does."""
    torch.manual_seed(H)
    m = ntm.DiffDelRNN(1, H, 1, skip=False, max_delay=D)
    if H == 64:
        m.load_state_dict(ntm.weights.load_state_dict(W_D))
        m.kernel_variant, m.delay_mode = "lat", "two_pass"
    m = m.to("cuda").eval()
    m.diffdel.defer_check = True
    return m


def _start(m, B):
    """What DiffDelRNN.predict does ahead of its forward: a fresh state, the warm start, one stream broadcast to B."""
    m.initialize_hidden(1, m.max_delay)
    m.warm_start()
    m.hidden = m.hidden.expand(1, B, m.hidden_size).contiguous()
    m.diffdel.buffer = m.diffdel.buffer.expand(B, 1, -1).contiguous()


TRAJECTORIES = ("zero", "const_D", "integers", "uniform", "sine", "line_length")


def _delays(kind, B, N, D, gen):
    """(B,1,N) delays in samples for a model with max_delay = D (delay line D + 1)."""
    if kind == "zero":
        d = torch.zeros(B, 1, N)
    elif kind == "const_D":
        d = torch.full((B, 1, N), float(D))
    elif kind == "line_length":                   # the longest delay the line takes: k = its length, the tap k + 1 is cut
        d = torch.full((B, 1, N), float(D + 1))
    elif kind == "integers":
        d = torch.randint(0, D + 1, (B, 1, N), generator=gen).float()
    elif kind == "uniform":
        d = torch.rand(B, 1, N, generator=gen) * D
        d[:, :, ::11] = float(D)                  # the bounds among them
        d[:, :, 5::11] = 0.0
    else:                                         # a slow sine around D / 2, fractional, one phase per stream
        n = torch.arange(N, dtype=torch.float64)
        ph = torch.arange(B, dtype=torch.float64).view(B, 1, 1)
        d = (0.5 * D + 0.45 * D * torch.sin(2 * math.pi * n / 997.0 + ph)).float().clamp_(0.0, float(D))
    return d.cuda()


def _signal(B, N, gen):
    return (torch.rand(B, 1, N, generator=gen) - 0.5).cuda()


@torch.no_grad()
def _run_both(s, m, x, d, block, warmup_first=False):
    """Every block through the streamer and through the model: (y, pre_d) of both, (B,1,N) each."""
    out = [torch.empty_like(x) for _ in range(4)]
    for k in range(x.shape[-1] // block):
        sl = slice(k * block, (k + 1) * block)
        wu = warmup_first and k == 0
        out[0][:, :, sl] = s.process(x[:, :, sl], d[:, :, sl], warmup=wu) if wu else s.process(x[:, :, sl], d[:, :, sl])
        out[1][:, :, sl] = s.pre
        out[2][:, :, sl], out[3][:, :, sl] = m(x[:, :, sl], d[:, :, sl], warmup=wu)
    return out


def _assert_same(got, want, block, what):
    if not torch.equal(got, want):
        n = int((got != want).any(0).any(0).nonzero()[0])
        raise AssertionError(f"{what}: first difference at sample {n} (block {n // block}, offset {n % block}): "
                             f"{got[:, 0, n].tolist()} vs {want[:, 0, n].tolist()}")


def _assert_state(s, m):
    h, buf = s.export_state()
    assert h.shape == m.hidden.shape and buf.shape == m.diffdel.buffer.shape
    assert torch.equal(h, m.hidden), "hidden state"
    assert torch.equal(buf, m.diffdel.buffer), "delay buffer"
    s.raise_if_violated()
    m.diffdel.raise_if_violated()


def _cases():
    """Every (block, D) pair once, B and the trajectory cycling; the pairs around the kernel's tile again with the other B and
    another trajectory; one block of three tiles: 33 cases."""
    pairs = list(itertools.product((1, 5, 64, 256, 300), (1, 7, 300, 1000)))
    out = [((1, 3)[i % 2], blk, D, TRAJECTORIES[i % 6]) for i, (blk, D) in enumerate(pairs)]
    out += [((3, 1)[i % 2], blk, D, TRAJECTORIES[(i + 3) % 6]) for i, (blk, D) in enumerate(pairs) if blk in (5, 256, 300)]
    return out + [(2, 600, 300, "uniform")]       # three tiles per block: the kernel's two y tile buffers both come round again


@pytest.mark.parametrize("B,block,D,traj", _cases())
def test_blocks_against_the_model_block_by_block(ntm, B, block, D, traj):
    """Enough blocks that the ring wraps at least twice (n_blocks * block >= 2 C + block): y and pre_d of every block, then
    the exported hidden state and delay buffer, against the model called with the same blocks."""
    m = _model(ntm, D)
    s = ntm.harness.BlockStreamer(m, B, block)
    assert s.one_launch and s.D == D + 1 and s.C >= s.D + block and s.C & (s.C - 1) == 0
    nblk = -(-(2 * s.C + block) // block)
    gen = torch.Generator().manual_seed(1000 * D + 10 * block + B)
    x, d = _signal(B, nblk * block, gen), _delays(traj, B, nblk * block, D, gen)
    _start(m, B)
    y, pre, y_m, pre_m = _run_both(s, m, x, d, block)
    _assert_same(pre, pre_m, block, "pre_d")
    _assert_same(y, y_m, block, "y")
    _assert_state(s, m)


@pytest.mark.parametrize("B,block,D", [(1, 64, 300), (3, 300, 7)])
def test_warmup_call_first(ntm, B, block, D):
    """process(..., warmup=True) returns pre_d and moves the state on, as the model's warm-up call does; normal blocks follow."""
    m = _model(ntm, D)
    s = ntm.harness.BlockStreamer(m, B, block)
    gen = torch.Generator().manual_seed(D + block)
    x, d = _signal(B, 5 * block, gen), _delays("uniform", B, 5 * block, D, gen)
    _start(m, B)
    y, pre, y_m, pre_m = _run_both(s, m, x, d, block, warmup_first=True)
    assert torch.equal(y[:, :, :block], pre[:, :, :block])
    _assert_same(pre, pre_m, block, "pre_d")
    _assert_same(y, y_m, block, "y")
    _assert_state(s, m)


@pytest.mark.parametrize("B,block,D", [(1, 5, 300), (3, 64, 7)])
def test_seeded_from_a_running_model(ntm, B, block, D):
    """A streamer built on a model whose hidden state and delay buffer an earlier forward() moved on continues where the model does."""
    m = _model(ntm, D)
    gen = torch.Generator().manual_seed(7 * D + B)
    _start(m, B)
    with torch.no_grad():
        m(_signal(B, 333, gen), _delays("sine", B, 333, D, gen))
    h0, buf0 = m.hidden.clone(), m.diffdel.buffer.clone()
    s = ntm.harness.BlockStreamer(m, B, block)
    assert torch.equal(m.hidden, h0) and torch.equal(m.diffdel.buffer, buf0)      # taken over, not restarted
    x, d = _signal(B, 6 * block, gen), _delays("uniform", B, 6 * block, D, gen)
    y, pre, y_m, pre_m = _run_both(s, m, x, d, block)
    _assert_same(y, y_m, block, "y")
    _assert_state(s, m)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("D", [1, 7, 1000])
def test_raw_seed_then_export_returns_the_buffer(ntm, D):
    L = ntm._lib.lib()
    B, block = 3, 64
    C = L.ntm_diffdel_stream_ring_floats(D, block)
    assert C >= D + block and C & (C - 1) == 0 and C < 2 * (D + block)
    buf = torch.randn(B, D, generator=torch.Generator().manual_seed(D)).cuda()
    ring = torch.full((B, C), 7.0, device="cuda")
    pos = torch.full((B,), -1, device="cuda", dtype=torch.int64)
    out = torch.full((B, D), 9.0, device="cuda")
    assert L.ntm_diffdel_stream_seed(_p(buf), _p(ring), _p(pos), B, D, C, _stream()) == 0, L.ntm_last_error()
    assert L.ntm_diffdel_stream_export(_p(ring), _p(pos), _p(out), B, D, C, _stream()) == 0, L.ntm_last_error()
    assert torch.equal(out, buf)
    assert bool((pos == D).all()) and bool((ring[:, D:] == 7.0).all())


@pytest.mark.parametrize("block", [5, 300, 600])
def test_raw_block_without_pre_d(ntm, block):
    """pre_d = NULL through the raw ABI (the kernel then parks pre_d in the y rows until the delay phase): the y, the hidden state
    and the ring of the call that returns pre_d; in a warm-up call y is pre_d."""
    B, D = 3, 300
    m = _model(ntm, D)
    a, b = ntm.harness.BlockStreamer(m, B, block), ntm.harness.BlockStreamer(m, B, block)
    L, g = ntm._lib.lib(), m.GRU
    gen = torch.Generator().manual_seed(block)
    x, d = _signal(B, 4 * block, gen), _delays("uniform", B, 4 * block, D, gen)
    for k in range(4):
        sl = slice(k * block, (k + 1) * block)
        want = a.process(x[:, :, sl], d[:, :, sl], warmup=(k == 1)).clone()
        b.x.copy_(x[:, :, sl])
        b.d.copy_(d[:, :, sl])
        rc = L.ntm_diffdel_stream_block(_p(g.weight_ih_l0), _p(g.weight_hh_l0), _p(g.bias_ih_l0), _p(g.bias_hh_l0), _p(m.output.weight),
                                        _p(b.x), _p(b.d), _p(b.y), None, B, block, block, block, block, _p(b.h), _p(b.buf), b.C,
                                        _p(b.pos), b.D, int(k == 1), _p(b.err), _stream())
        assert rc == 0, L.ntm_last_error()
        assert torch.equal(b.y, want), k
        if k == 1:
            assert torch.equal(want, a.pre)
    for u, v in zip(a.export_state(), b.export_state()):
        assert torch.equal(u, v)
    assert torch.equal(a.pos, b.pos) and bool((a.pos == a.D + 4 * block).all())


def test_graph_replay_gives_the_plain_launches_outputs(ntm):
    B, block, D = 3, 64, 300
    m = _model(ntm, D)
    plain = ntm.harness.BlockStreamer(m, B, block)
    graph = ntm.harness.BlockStreamer(m, B, block, use_graph=True)
    assert graph.graph is not None and plain.graph is None
    nblk = -(-(2 * plain.C + block) // block)
    gen = torch.Generator().manual_seed(5)
    x, d = _signal(B, nblk * block, gen), _delays("uniform", B, nblk * block, D, gen)
    for k in range(nblk):
        sl = slice(k * block, (k + 1) * block)
        yp, yg = plain.process(x[:, :, sl], d[:, :, sl]), graph.process(x[:, :, sl], d[:, :, sl])
        assert torch.equal(yp, yg) and torch.equal(plain.pre, graph.pre), k
    for a, b in zip(plain.export_state(), graph.export_state()):
        assert torch.equal(a, b)
    graph.raise_if_violated()


def test_other_hidden_size_runs_the_two_launch_path(ntm):
    """H = 16: ntm_diffdel_gru_forward per block on the streamer's own buffers, the bits of the model's forward()."""
    B, block, D = 3, 37, 50
    m = _model(ntm, D, H=16)
    s = ntm.harness.BlockStreamer(m, B, block)
    assert not s.one_launch
    gen = torch.Generator().manual_seed(16)
    x, d = _signal(B, 6 * block, gen), _delays("uniform", B, 6 * block, D, gen)
    _start(m, B)
    y, pre, y_m, pre_m = _run_both(s, m, x, d, block)
    _assert_same(pre, pre_m, block, "pre_d")
    _assert_same(y, y_m, block, "y")
    _assert_state(s, m)


def test_range_violation_raises_and_leaves_the_model_alone(ntm):
    """One delay of (delay-line length) + 1 -- the D + 1 of the kernel's D: raise_if_violated() raises like the model, the model
    object's own state has not moved, and a new streamer on the same model works."""
    B, block, D = 3, 64, 300
    m = _model(ntm, D)
    s = ntm.harness.BlockStreamer(m, B, block)
    h0, buf0 = m.hidden.clone(), m.diffdel.buffer.clone()
    gen = torch.Generator().manual_seed(6)
    x, d = _signal(B, 3 * block, gen), _delays("uniform", B, 3 * block, D, gen)
    s.process(x[:, :, :block], d[:, :, :block])
    s.raise_if_violated()                                      # nothing so far
    bad = d[:, :, block:2 * block].clone()
    bad[1, 0, 17] = s.D + 1
    s.process(x[:, :, block:2 * block], bad)
    with pytest.raises(AssertionError):
        s.raise_if_violated()
    assert torch.equal(m.hidden, h0) and torch.equal(m.diffdel.buffer, buf0)
    s2 = ntm.harness.BlockStreamer(m, B, block)
    _start(m, B)
    y, pre, y_m, pre_m = _run_both(s2, m, x, d, block)
    _assert_same(y, y_m, block, "y")
    _assert_state(s2, m)


def test_signatures(ntm):
    B, block = 2, 64
    md = _model(ntm, 7)
    sd = ntm.harness.BlockStreamer(md, B, block)
    x = torch.zeros(B, 1, block, device="cuda")
    with pytest.raises(TypeError):
        sd.process(x)                                          # d_block missing
    for shape in [(B, 1, block + 1), (B + 1, 1, block), (1, B, block), (B * block,)]:
        with pytest.raises((ValueError, RuntimeError)):
            sd.process(x, torch.zeros(shape, device="cuda"))
    mg = ntm.harness.build_model(W_G)
    sg = ntm.harness.BlockStreamer(mg, B, block)
    with pytest.raises(TypeError):
        sg.process(x, x)                                       # d_block to an RNN streamer
    with pytest.raises(TypeError):
        ntm.harness.BlockStreamer(torch.nn.Linear(1, 1), B, block)
    # the RNN streamer is what it was: model.forward on the concatenated blocks
    xs = _signal(B, 5 * block, torch.Generator().manual_seed(2))
    got = torch.cat([sg.process(xs[:, :, k * block:(k + 1) * block]).clone() for k in range(5)], 2)
    mg.initialize_hidden()
    mg.warm_start()
    mg.hidden = mg.hidden.expand(1, B, mg.hidden_size).contiguous()
    with torch.no_grad():
        assert torch.equal(got, mg(xs))


def test_empty_calls_through_the_raw_abi(ntm):
    """B = 0 and block = 0 return success and touch nothing (the pointers are not looked at)."""
    L = ntm._lib.lib()
    one = 16
    for B, block in [(0, 64), (3, 0), (0, 0)]:
        rc = L.ntm_diffdel_stream_block(one, one, one, one, one, one, one, one, None, B, block, block, block, block, one, one, 64,
                                        one, 7, 0, None, None)
        assert rc == 0, L.ntm_last_error()
    assert L.ntm_diffdel_stream_seed(None, None, None, 0, 7, 8, None) == 0
    assert L.ntm_diffdel_stream_export(None, None, None, 0, 7, 8, None) == 0
    # ... and what is wrong is refused before anything is enqueued
    assert L.ntm_diffdel_stream_block(one, one, one, one, one, one, one, 32, None, 3, 64, 64, 64, 64, one, one, 64, one, 7, 0, None, None) == -1
    assert b"D + block" in L.ntm_last_error()
    assert L.ntm_diffdel_stream_block(one, one, one, one, one, one, one, 32, None, 3, 64, 64, 64, 64, one, one, 96, one, 7, 0, None, None) == -1
    assert b"power of two" in L.ntm_last_error()
    assert L.ntm_diffdel_stream_block(one, one, one, one, one, one, one, 32, None, 3, 64, 64, 64, 64, None, one, 128, one, 7, 0, None, None) == -1
    assert b"null pointer" in L.ntm_last_error()
