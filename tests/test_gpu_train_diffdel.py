"""GPU: the training path of DiffDelGRU-HS[64] (ntm_delay_backward in csrc/gru_train.hip, training.DelayLineStep,
DiffDelRNN.train_epoch) -- the delay line's adjoint against float64 torch autograd of a restatement of the reference's delay line,
the training forward against the inference path bit for bit, a warm-up and two windows chained without detaching against float64
autograd, one epoch of the reference's train_epoch (golden g24, tools/make_goldens_train_diffdel.py), determinism, the range
assert, the two batch formats, and no change to the inference path."""
import numpy as np
import pytest
import torch

from helpers import load

W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"
KEYS = ["GRU.weight_ih_l0", "GRU.weight_hh_l0", "GRU.bias_ih_l0", "GRU.bias_hh_l0", "output.weight"]


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def delay_ref(pre, buf, d, warmup):
    """The reference's delay line (code/model.py:269-320) restated on [B,L] / [B,D] tensors, differentiable in pre and buf: the
    interpolation weights relu(1 - |m - d|) of the taps m = D..0 formed in fp32 from the fp32 delays, as the reference forms
    them, then everything in the dtype of pre.  -> (y, new_buffer)."""
    B, L = pre.shape
    D = buf.shape[1]
    z = torch.cat([buf, pre], dim=1)
    nb = z[:, L:L + D]
    if warmup:
        return pre, nb
    y = torch.zeros_like(pre)
    kf = torch.floor(d)
    n = torch.arange(L).expand(B, L)
    for tap in (1, 0):
        m = kf + tap
        w = torch.relu(1.0 - torch.abs(m - d))
        on = (m >= 0) & (m <= D) & (w > 0)
        idx = (D + n - torch.where(on, m, torch.zeros_like(m)).long()).clamp(0, D + L - 1)
        y = y + torch.where(on, w.to(pre.dtype) * torch.gather(z, 1, idx), torch.zeros_like(pre))
    return y, nb


def trajectory(kind, B, L, D, g):
    n = torch.arange(L, dtype=torch.float64)
    if kind == "random":
        d = torch.rand(B, L, generator=g, dtype=torch.float64) * D
    elif kind == "smooth":
        d = 0.5 * D + 0.4 * D * torch.sin(2 * np.pi * n / 1500 + torch.rand(B, 1, generator=g, dtype=torch.float64) * 6)
    elif kind == "whole":
        d = torch.randint(0, D + 1, (B, L // 64 + 1), generator=g).double().repeat_interleave(64, dim=1)[:, :L]
    elif kind == "zero":
        d = torch.zeros(B, L, dtype=torch.float64)
    elif kind == "at_D":
        d = torch.full((B, L), float(D), dtype=torch.float64)
    elif kind == "falling":     # falls fast: gaps between the buffer positions that receive terms
        d = (D - (n * 3.7) % (D + 1)).clamp(0, D).expand(B, L)
    elif kind == "rising":      # rising at ~1 and ~1.6 samples per sample: many terms per target, and q not monotone
        d = torch.where(n % 400 < 300, (n % 400) * 0.9991, 300 + (n % 400 - 300) * 1.6).clamp(0, D).expand(B, L)
    return d.float().contiguous()


def _backward(ntm, gy, d, gnb, B, L, D, warmup, need_gbuf, flags=0):
    L_ = ntm._lib.lib()
    p = ntm._lib.ptr
    gpre = torch.full((B, L), float("nan"), device="cuda")
    gbuf = torch.full((B, D), float("nan"), device="cuda") if need_gbuf else None
    ntm._lib.check(L_.ntm_delay_backward(p(gy), p(d), p(gnb), p(gpre), p(gbuf), B, L, D, int(warmup), flags,
                                         ntm._lib.current_stream()), "ntm_delay_backward")
    return gpre, gbuf


CASES = [(3, 300, 700), (3, 2048, 552), (2, 5000, 300), (2, 64, 11001)]
KINDS = ["random", "smooth", "whole", "zero", "at_D", "falling", "rising"]


# (kind, warmup, with g_newbuf, with gbuf): every trajectory in a window; the warm-up (which reads no delays) once per option
FLOWS = [(k, False, gn, gb) for k in KINDS for gn, gb in ((False, True), (True, True), (True, False))] + \
        [("random", True, True, True), ("random", True, False, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,D", CASES)
@pytest.mark.parametrize("kind,warmup,with_gnb,need_gbuf", FLOWS)
def test_delay_adjoint_against_float64_autograd(ntm, B, L, D, kind, warmup, with_gnb, need_gbuf):
    g = torch.Generator().manual_seed(B * 131 + L + D + KINDS.index(kind))
    d = trajectory(kind, B, L, D, g)
    gy = torch.randn(B, L, generator=g)
    gnb = torch.randn(B, D, generator=g) if with_gnb else None
    grads = {}
    for dt in (torch.float64, torch.float32):
        pre = torch.zeros(B, L, dtype=dt, requires_grad=True)
        buf = torch.zeros(B, D, dtype=dt, requires_grad=True)
        y, nb = delay_ref(pre, buf, d, warmup)
        loss = (y * gy.to(dt)).sum() + ((nb * gnb.to(dt)).sum() if with_gnb else 0.0)
        gs = torch.autograd.grad(loss, [pre, buf], allow_unused=True)      # the warm-up without g_newbuf: buf is unused
        grads[dt] = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(gs, (pre, buf))]
    dc = d.cuda()
    gyc, gnbc = gy.cuda(), (gnb.cuda() if with_gnb else None)
    gpre, gbuf = _backward(ntm, gyc, dc, gnbc, B, L, D, warmup, need_gbuf)
    for name, got, r64, r32 in (("gpre", gpre, grads[torch.float64][0], grads[torch.float32][0]),
                                ("gbuf", gbuf, grads[torch.float64][1], grads[torch.float32][1])):
        if got is None:
            continue
        a = got.double().cpu()
        assert torch.isfinite(a).all(), name
        err = float((a - r64).abs().max())
        bar = max(4 * float((r32.double() - r64).abs().max()), 2e-6 * float(r64.abs().max()), 1e-30)
        assert err <= bar, (name, err, bar)
    # the general path gives the same bits, and so does a repeated call
    gpre_s, gbuf_s = _backward(ntm, gyc, dc, gnbc, B, L, D, warmup, need_gbuf, flags=1)
    gpre_r, gbuf_r = _backward(ntm, gyc, dc, gnbc, B, L, D, warmup, need_gbuf)
    assert torch.equal(gpre, gpre_s) and torch.equal(gpre, gpre_r)
    if need_gbuf:
        assert torch.equal(gbuf, gbuf_s) and torch.equal(gbuf, gbuf_r)


def _model(ntm, sd=None, grad=True, max_delay=551):
    m = ntm.DiffDelRNN(1, 64, 1, max_delay=max_delay).cuda()
    if sd is not None:
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    for p in m.parameters():
        p.requires_grad_(grad)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("B,T0,T1", [(1, 256, 700), (5, 1024, 2048), (32, 512, 2048)])
def test_training_forward_is_bit_identical_to_the_inference_path(ntm, B, T0, T1):
    sd = ntm.weights.load_state_dict(W_D)
    g = torch.Generator().manual_seed(B + T0)
    x = (torch.rand(B, 1, T0 + T1, generator=g) - 0.5).cuda()
    d = (trajectory("smooth", B, T0 + T1, 552, g) * 0.9).unsqueeze(1).cuda()
    ref = _model(ntm, sd, grad=False)
    ref.kernel_variant, ref.delay_mode = "lat", "two_pass"
    m = _model(ntm, sd)
    outs = []
    for mod in (ref, m):
        mod.initialize_hidden(B, mod.max_delay)
        with torch.enable_grad():
            a = mod(x[:, :, :T0], d[:, :, :T0], warmup=True)
            b = mod(x[:, :, T0:], d[:, :, T0:])
        outs.append([t.detach() for t in a + b] + [mod.hidden.detach(), mod.diffdel.buffer.detach()])
    assert all(t.requires_grad for t in b) and m.hidden.requires_grad and m.diffdel.buffer.requires_grad
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def _torch_chain(sd, x, d, D, gys, dtype):
    """float64 (or float32) autograd on the CPU of torch.nn.GRU + Linear(bias=False) + the delay restatement over a warm-up and
    the windows that follow, nothing detached: d/d(params) of sum_w sum(gy_w * y_w)."""
    gru = torch.nn.GRU(1, 64, batch_first=True).to(dtype)
    lin = torch.nn.Linear(64, 1, bias=False).to(dtype)
    with torch.no_grad():
        for n, p in list(gru.named_parameters()) + [("w", lin.weight)]:
            p.copy_(torch.as_tensor(sd["output.weight" if n == "w" else "GRU." + n]).to(dtype))
    B = x[0].shape[0]
    h = None
    buf = torch.zeros(B, D, dtype=dtype)
    loss = 0.0
    for i, (xw, dw) in enumerate(zip(x, d)):
        out, h = gru(xw.to(dtype).reshape(B, -1, 1), h)
        pre = lin(out)[..., 0]
        y, buf = delay_ref(pre, buf, dw, warmup=(i == 0))
        if i > 0:
            loss = loss + (y * gys[i - 1].to(dtype)).sum()
    ps = [gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, lin.weight]
    return [g.double() for g in torch.autograd.grad(loss, ps)]


# test_gpu_train.py's small-scale term: the training forward repeats the low-latency kernel's tanh form 1 - 2/(1 + e^(2v)), whose
# ABSOLUTE error of ~1 ulp of 1 the three chained calls (warm-up and two windows, ~2300 steps) carry into the gradients at ~1e-5
# relative, where torch's CPU fp32 has ~1e-7.  1e-4 of the largest entry still catches any wrong term of an adjoint (those are O(1)).
SMALL_SCALE_REL = 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,T0,L,kind", [(3, 300, 256, 512, "smooth"), (4, 552, 512, 1024, "rising"), (2, 200, 512, 700, "random")])
def test_warmup_and_two_windows_chained_against_float64_autograd(ntm, B, D, T0, L, kind):
    sd = ntm.weights.load_state_dict(W_D)
    g = torch.Generator().manual_seed(B * 7 + D)
    x = [torch.rand(B, T, generator=g) - 0.5 for T in (T0, L, L)]
    d = [trajectory(kind, B, T, D, g) for T in (T0, L, L)]
    gys = [torch.randn(B, L, generator=g) for _ in range(2)]
    g64 = _torch_chain(sd, x, d, D, gys, torch.float64)
    g32 = _torch_chain(sd, x, d, D, gys, torch.float32)
    m = _model(ntm, sd, max_delay=D - 1)
    m.initialize_hidden(B, m.max_delay)
    loss = 0.0
    for i, (xw, dw) in enumerate(zip(x, d)):
        y, _ = m(xw.unsqueeze(1).cuda(), dw.unsqueeze(1).cuda(), warmup=(i == 0))
        if i > 0:
            loss = loss + (y[:, 0, :] * gys[i - 1].cuda()).sum()
    got = torch.autograd.grad(loss, list(m.parameters()))
    for name, a, r64, r32 in zip(KEYS, got, g64, g32):
        a = a.double().cpu().reshape(r64.shape)
        err = float((a - r64).abs().max())
        bar = max(4 * float((r32 - r64).abs().max()), SMALL_SCALE_REL * float(r64.abs().max()))
        assert err <= bar, (name, err, bar, float(r64.abs().max()))


class RecordingAdam(torch.optim.Adam):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.grads = []

    def step(self, closure=None):
        self.grads.append([p.grad.detach().double().cpu().clone() for g in self.param_groups for p in g["params"]])
        return super().step(closure)


class _Loader(list):
    """The reference's DataLoader as train_epoch sees it: (x, t, meta) batches and .dataset.fs / .dataset.delay_analyzer."""

    def __init__(self, batches, fs, max_delay_s):
        super().__init__(batches)
        self.dataset = type("DS", (), {"fs": fs, "delay_analyzer": type("DA", (), {"max_delay": max_delay_s})})


def _g24_loader(inp):
    fs = int(inp["meta"][7])
    return _Loader([(torch.from_numpy(x), torch.from_numpy(t), {"delay_trajectory": torch.from_numpy(tr)})
                    for x, t, tr in zip(inp["x"], inp["t"], inp["traj_s"])], fs, float(inp["analyser_max_delay_s"]))


def _epoch(ntm, loss_name, loader=None, dataset=None):
    inp = load("g24_train_diffdel_inputs.npz")
    m = _model(ntm, ntm.weights.load_state_dict(W_D), grad=False, max_delay=int(inp["meta"][6]))
    opt = RecordingAdam(m.parameters(), lr=float(inp["lr"]))
    fn = ntm.ESRLoss() if loss_name == "esr" else ntm.DCPreESR(dc_pre=True)
    losses = []

    def loss_fcn(p, t):
        v = fn(p, t)
        losses.append(float(v.detach()))
        return v

    epoch = m.train_epoch(_g24_loader(inp) if loader is None else loader, loss_fcn, opt, dataset=dataset)
    return m, opt, losses, epoch


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name", ["esr", "dcpreesr"])
def test_train_epoch_against_the_reference_g24(ntm, loss_name):
    ref = load(f"g24_train_diffdel_{loss_name}.npz")
    m, opt, losses, epoch = _epoch(ntm, loss_name)
    assert len(opt.grads) == len(ref["losses"]) == 6
    for w, gw in enumerate(opt.grads):
        for key, a in zip(KEYS, gw):
            r = ref[f"grad__{key}"][w].astype(np.float64)
            err = float(np.abs(a.numpy().reshape(r.shape) - r).max())
            assert err <= 1e-4 * float(np.abs(r).max()), (w, key, err, float(np.abs(r).max()))
    np.testing.assert_allclose(losses, ref["losses"], rtol=1e-5, atol=0)
    assert abs(epoch / float(ref["epoch_loss"]) - 1) < 1e-5
    steps = len(ref["losses"])
    lr = float(load("g24_train_diffdel_inputs.npz")["lr"])
    sd = m.state_dict()
    for key in KEYS:
        a, r = sd[key].detach().cpu().numpy(), ref[f"final__{key}"]
        dd = np.abs(a - r)
        assert float(dd.max()) <= 2 * lr * steps, (key, float(dd.max()))
        assert float((dd <= 1e-5).mean()) >= 0.999, (key, float((dd <= 1e-5).mean()))


@pytest.mark.gpu
def test_train_epoch_is_deterministic_and_the_loss_falls_over_epochs(ntm):
    m1, _, l1, _ = _epoch(ntm, "dcpreesr")
    m2, _, l2, _ = _epoch(ntm, "dcpreesr")
    assert l1 == l2
    for a, b in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    inp = load("g24_train_diffdel_inputs.npz")
    m = _model(ntm, ntm.weights.load_state_dict(W_D), grad=False, max_delay=int(inp["meta"][6]))
    opt = torch.optim.Adam(m.parameters(), 1e-3)
    curve = [m.train_epoch(_g24_loader(inp), ntm.ESRLoss(), opt) for _ in range(4)]
    assert all(b < a for a, b in zip(curve, curve[1:])), curve


@pytest.mark.gpu
def test_segment_feeder_batches_give_the_same_epoch(ntm):
    """SegmentFeeder.batches' format: (x, t, d_seconds (B,1,T) on the device, metas), `dataset` with fs and max_delay."""
    inp = load("g24_train_diffdel_inputs.npz")
    fs = int(inp["meta"][7])
    ds = type("Feeder", (), {"fs": fs, "max_delay": float(inp["analyser_max_delay_s"])})

    def batches():
        for x, t, tr in zip(inp["x"], inp["t"], inp["traj_s"]):
            yield (torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(tr).unsqueeze(1).cuda(), [{}] * len(x))
    ma, _, la, ea = _epoch(ntm, "esr")
    mb, _, lb, eb = _epoch(ntm, "esr", loader=batches(), dataset=ds)
    assert la == lb and ea == eb
    for a, b in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_a_delay_above_the_buffer_raises_and_leaves_buffer_and_parameters(ntm):
    sd = ntm.weights.load_state_dict(W_D)
    B, D = 2, 300
    m = _model(ntm, sd, max_delay=D - 1)
    m.initialize_hidden(B, m.max_delay)
    x = (torch.rand(B, 1, 512) - 0.5).cuda()
    d = torch.full((B, 1, 512), 100.0, device="cuda")
    m(x, d, warmup=True)
    buf = m.diffdel.buffer.detach().clone()
    params = [p.detach().clone() for p in m.parameters()]
    bad = d.clone()
    bad[1, 0, 77] = D + 0.5
    with pytest.raises(AssertionError):
        m(x, bad)
    assert torch.equal(m.diffdel.buffer.detach(), buf)
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), params))
    # the flag is cleared: the next good window runs
    y, _ = m(x, d)
    assert y.requires_grad


@pytest.mark.gpu
def test_inference_is_unchanged_with_default_parameters_and_under_no_grad(ntm):
    sd = ntm.weights.load_state_dict(W_D)
    x = (torch.rand(3, 1, 700, generator=torch.Generator().manual_seed(1)) - 0.5).cuda()
    d = (trajectory("smooth", 3, 700, 552, torch.Generator().manual_seed(2)) * 0.9).unsqueeze(1).cuda()

    def run(m, ctx):
        m.initialize_hidden(3, m.max_delay)
        with ctx():
            return m(x, d)
    ref = run(_model(ntm, sd, grad=False), torch.no_grad)
    y1 = run(_model(ntm, sd, grad=False), torch.enable_grad)
    y2 = run(_model(ntm, sd, grad=True), torch.no_grad)
    for a, b, c in zip(ref, y1, y2):
        assert not b.requires_grad and not c.requires_grad
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.gpu
def test_diffdel_training_refusals_on_the_device(ntm):
    m = _model(ntm, ntm.weights.load_state_dict(W_D), max_delay=99)
    m.initialize_hidden(2, m.max_delay)
    x = (torch.rand(2, 1, 64) - 0.5).cuda()
    d = torch.full((2, 1, 64), 10.0, device="cuda")
    want = r"DiffDelRNN\(input_size=1, hidden_size=64, output_size=1, skip=False\)"
    with pytest.raises(RuntimeError, match=want):
        m(x.clone().requires_grad_(True), d)
    with pytest.raises(RuntimeError, match=want):
        m(x, d.clone().requires_grad_(True))
    short = _Loader([(x.cpu(), x.cpu(), {"delay_trajectory": torch.zeros(2, 64)})], 44100, 0.001)
    with pytest.raises(ZeroDivisionError):
        m.train_epoch(short, ntm.ESRLoss(), torch.optim.Adam(m.parameters(), 1e-3))
