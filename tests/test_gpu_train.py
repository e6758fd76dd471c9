"""GPU: the training path of GRU-HS[64] (csrc/gru_train.hip, training.py, RNN.train_epoch) -- the training forward against the
low-latency kernel bit for bit, the BPTT gradients against float64 torch autograd on the CPU, the loss adjoints, one epoch of
the reference's train_epoch (golden g23, tools/make_goldens_train.py), determinism, and no change to the inference path."""
import numpy as np
import pytest
import torch

from gru_train_cases import T_EDGES
from helpers import load

W_G = "GRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE]_BEST"
KEYS = ["GRU.weight_ih_l0", "GRU.weight_hh_l0", "GRU.bias_ih_l0", "GRU.bias_hh_l0", "output.weight", "output.bias"]


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def _model(ntm, sd=None, grad=True):
    m = ntm.RNN(1, 64, 1).cuda()
    if sd is not None:
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    for p in m.parameters():
        p.requires_grad_(grad)
    return m


def _random_sd(seed, scale):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / 8.0
    shapes = {"GRU.weight_ih_l0": (192, 1), "GRU.weight_hh_l0": (192, 64), "GRU.bias_ih_l0": (192,), "GRU.bias_hh_l0": (192,),
              "output.weight": (1, 64), "output.bias": (1,)}
    return {n: ((torch.rand(*s, generator=g) * 2 - 1) * k * scale).float() for n, s in shapes.items()}


# the grid of batch sizes and lengths, and B = 1, 3 at every length of the edge list of tests/gru_train_cases.py (the tail of the
# step pairs, the 32-step save stage, the x prefetch at step 128, the 256-sample tile and finish()'s two ways to the previous y tile)
FORWARD_GRID = list(dict.fromkeys([(T, B) for T in (1, 5, 256, 1024, 1500) for B in (1, 7, 32, 300, 1100)] +
                                  [(T, B) for B in (1, 3) for T in T_EDGES]))


@pytest.mark.gpu
@pytest.mark.parametrize("T,B", FORWARD_GRID)
def test_training_forward_is_bit_identical_to_the_low_latency_kernel(ntm, B, T):
    sd = ntm.weights.load_state_dict(W_G)
    g = torch.Generator().manual_seed(B * 7919 + T)
    x = (torch.rand(B, 1, T, generator=g) - 0.5).cuda()
    h0 = (0.5 * (torch.rand(1, B, 64, generator=g) - 0.5)).cuda()
    ref = _model(ntm, sd, grad=False)
    ref.kernel_variant = "lat"
    ref.hidden = h0.clone()
    y_ref = ref(x)
    m = _model(ntm, sd)
    m.hidden = h0.clone()
    y = m(x)
    assert y.requires_grad and m.hidden.requires_grad
    assert torch.equal(y.detach(), y_ref) and torch.equal(m.hidden.detach(), ref.hidden)


def _torch_grads(sd, x, h0, dy, dh, dtype):
    """float64 (or float32) autograd of torch.nn.GRU + Linear on the CPU: d/d(params, h0) of sum(dy * y) + sum(dh * h_T)."""
    gru = torch.nn.GRU(1, 64, batch_first=True).to(dtype)
    lin = torch.nn.Linear(64, 1).to(dtype)
    with torch.no_grad():
        for n, p in list(gru.named_parameters()) + [("w", lin.weight), ("b", lin.bias)]:
            key = {"w": "output.weight", "b": "output.bias"}.get(n, "GRU." + n)
            p.copy_(torch.as_tensor(sd[key]).to(dtype))
    h = h0.to(dtype).clone().requires_grad_(True)
    out, hT = gru(x.to(dtype).reshape(x.shape[0], x.shape[2], 1), h)
    y = lin(out)[..., 0]
    L = (y * dy.to(dtype)).sum() if dy is not None else 0.0
    L = L + (hT * dh.to(dtype)).sum() if dh is not None else L
    ps = [gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, lin.weight, lin.bias, h]
    gs = torch.autograd.grad(L, ps, allow_unused=True)          # dy None: the head is not in the graph
    return [(torch.zeros_like(p) if g is None else g).double() for g, p in zip(gs, ps)]


CASES = [(1, 1, "ckpt", 1.0, True), (7, 5, "ckpt", 1.0, True), (32, 1024, "ckpt", 1.0, True), (32, 1024, "ckpt", 1.0, False),
         (300, 1500, "ckpt", 1.0, True), (1100, 256, "ckpt", 1.0, True), (32, 256, "rand", 1.0, True), (32, 256, "rand", 10.0, True),
         (32, 256, "rand", 3.0, True), (7, 1500, "rand", 1.0, False),
         (32, 256, "rand", 0.1, True), (32, 256, "rand", 0.01, True)]
# every tail length of the backward's groups of four steps, the start of its register ring (T < 4) and the forward's stage and
# tile edges, through the path users call (the raw kernels are held exactly at these lengths by tests/test_gpu_gru_train_edges.py)
CASES += [(3, T, "ckpt", 1.0, True) for T in T_EDGES] + [(2, T, "rand", 1.0, False) for T in (2, 3, 7, 33, 259)]
assert len(set(CASES)) == len(CASES)
# Random weights over three decades of scale, 0.01 to 10 times torch's init scale (beyond 10, the recurrence's gradients grow
# without bound in float64 too).  Below init scale the bar has a third term: the forward's tanh form 1 - 2/(1 + e^(2v)) (the
# low-latency kernel's, which the training forward reproduces bit for bit) has an ABSOLUTE error of ~1 ulp of 1 (6e-8), so with
# hidden states of ~1e-3 the gradients carry ~2e-5 relative error where torch's CPU fp32, with a relative-accuracy tanh, has
# ~1e-7; 1e-4 of the largest entry covers that with margin and still catches any wrong term of the adjoint (those are O(1)).
SMALL_SCALE_REL = 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,wk,scale,with_dy", CASES)
def test_bptt_gradients_against_float64_autograd(ntm, B, T, wk, scale, with_dy):
    sd = ntm.weights.load_state_dict(W_G) if wk == "ckpt" else _random_sd(B + T, scale)
    g = torch.Generator().manual_seed(31 * B + T)
    x = torch.rand(B, 1, T, generator=g) - 0.5
    h0 = 0.5 * (torch.rand(1, B, 64, generator=g) - 0.5)
    dy = torch.randn(B, T, generator=g) if with_dy else None
    dh = torch.randn(1, B, 64, generator=g)
    g64 = _torch_grads(sd, x, h0, dy, dh, torch.float64)
    g32 = _torch_grads(sd, x, h0, dy, dh, torch.float32)

    m = _model(ntm, sd)
    h = h0.cuda().requires_grad_(True)
    m.hidden = h
    y = m(x.cuda())
    outs, grads = [m.hidden], [dh.cuda()]
    if with_dy:
        outs.append(y[:, 0, :])
        grads.append(dy.cuda())
    got = torch.autograd.grad(outs, list(m.parameters()) + [h], grads)
    for name, a, r64, r32 in zip(KEYS + ["h0"], got, g64, g32):
        a = a.double().cpu().reshape(r64.shape)
        err = float((a - r64).abs().max())
        bar = max(4 * float((r32 - r64).abs().max()), (2e-6 if scale >= 1 else SMALL_SCALE_REL) * float(r64.abs().max()))
        assert err <= bar, (name, err, bar, float(r64.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["esr", "dcpre", "dcpre_off"])
def test_loss_adjoints_against_float64_autograd_and_values_unchanged(ntm, kind):
    g = torch.Generator().manual_seed(5)
    B, T = 5, 1000
    y = torch.rand(B, 1, T, generator=g) - 0.5
    t = (0.8 * y + 0.1 * torch.randn(B, 1, T, generator=g) + 0.05).float()
    R = float(np.float32(ntm.model.DC_PRE_R))
    fn = ntm.ESRLoss() if kind == "esr" else ntm.DCPreESR(dc_pre=(kind == "dcpre"))
    yc = y.cuda().requires_grad_(True)
    v = fn(yc, t.cuda())
    v0 = fn(y.cuda(), t.cuda())
    assert v.requires_grad and not v0.requires_grad and torch.equal(v.detach(), v0)
    (3.0 * v).backward()

    y64 = y.double().requires_grad_(True)
    a, b = y64, t.double()
    if kind == "dcpre":
        k = np.arange(T)
        h = np.where(k == 0, 1.0, R ** np.maximum(k - 1, 0) * (R - 1.0))
        d = k[:, None] - k[None, :]
        M = torch.from_numpy(np.where(d >= 0, h[np.maximum(d, 0)], 0.0))
        a, b = a @ M.T, b @ M.T
    n = y.numel()
    L64 = (((b - a) ** 2).sum() / n) / ((b ** 2).sum() / n + 1e-5)
    (3.0 * L64).backward()
    ref = y64.grad
    err = float((yc.grad.double().cpu() - ref).abs().max())
    assert err <= 1e-5 * float(ref.abs().max()), (err, float(ref.abs().max()))
    assert abs(float(v.detach()) / float(L64.detach()) - 1) < 1e-5


class RecordingAdam(torch.optim.Adam):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.grads = []

    def step(self, closure=None):
        self.grads.append([p.grad.detach().double().cpu().clone() for g in self.param_groups for p in g["params"]])
        return super().step(closure)


def _epoch(ntm, loss_name):
    inp = load("g23_train_inputs.npz")
    m = _model(ntm, ntm.weights.load_state_dict(W_G), grad=False)
    opt = RecordingAdam(m.parameters(), lr=float(inp["lr"]))
    fn = ntm.ESRLoss() if loss_name == "esr" else ntm.DCPreESR(dc_pre=True)
    losses = []

    def loss_fcn(p, t):
        v = fn(p, t)
        losses.append(float(v.detach()))
        return v

    loader = [(torch.from_numpy(x), torch.from_numpy(t), None) for x, t in zip(inp["x"], inp["t"])]
    epoch = m.train_epoch(loader, loss_fcn, opt)
    return m, opt, losses, epoch


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name", ["esr", "dcpreesr"])
def test_train_epoch_against_the_reference_g23(ntm, loss_name):
    ref = load(f"g23_train_{loss_name}.npz")
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
    lr = float(load("g23_train_inputs.npz")["lr"])
    sd = m.state_dict()
    for key in KEYS:
        a, r = sd[key].detach().cpu().numpy(), ref[f"final__{key}"]
        d = np.abs(a - r)
        assert float(d.max()) <= 2 * lr * steps, (key, float(d.max()))
        assert float((d <= 1e-5).mean()) >= 0.999, (key, float((d <= 1e-5).mean()))


@pytest.mark.gpu
def test_train_epoch_is_deterministic_and_the_loss_falls_over_epochs(ntm):
    m1, _, _, _ = _epoch(ntm, "dcpreesr")
    m2, _, _, _ = _epoch(ntm, "dcpreesr")
    for a, b in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    # a few epochs of the reference-style loop on the small synthetic set
    inp = load("g23_train_inputs.npz")
    m = _model(ntm, ntm.weights.load_state_dict(W_G), grad=False)
    opt = torch.optim.Adam(m.parameters(), 1e-3)
    loader = [(torch.from_numpy(x), torch.from_numpy(t), None) for x, t in zip(inp["x"], inp["t"])]
    curve = [m.train_epoch(loader, ntm.ESRLoss(), opt) for _ in range(4)]
    assert all(b < a for a, b in zip(curve, curve[1:])), curve


@pytest.mark.gpu
def test_inference_path_is_unchanged_with_default_parameters(ntm):
    sd = ntm.weights.load_state_dict(W_G)
    x = (torch.rand(3, 1, 700, generator=torch.Generator().manual_seed(1)) - 0.5).cuda()
    m = _model(ntm, sd, grad=False)
    with torch.enable_grad():
        y1 = m(x)
        l1 = ntm.ESRLoss()(y1, x)
    m.initialize_hidden()
    with torch.no_grad():
        y2 = m(x)
    assert not y1.requires_grad and not l1.requires_grad and torch.equal(y1, y2)
    # grad-requiring parameters under no_grad: the inference path (validate() after training, code/train.py:242)
    mt = _model(ntm, sd)
    with torch.no_grad():
        y3 = mt(x)
    assert not y3.requires_grad and torch.equal(y3, y2)


@pytest.mark.gpu
def test_training_refusals_on_the_device(ntm):
    sd = ntm.weights.load_state_dict(W_G)
    m = _model(ntm, sd)
    x = (torch.rand(2, 1, 64) - 0.5).cuda()
    with pytest.raises(RuntimeError, match="input requires grad"):
        m(x.clone().requires_grad_(True))
    # the optimizer updates a weight in place before backward: torch's version check refuses the stale graph
    m.initialize_hidden()
    y = m(x)
    with torch.no_grad():
        m.GRU.weight_hh_l0.add_(1e-3)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()
    m32 = ntm.RNN(1, 32, 1).cuda()
    with pytest.raises(RuntimeError, match="hidden_size=64"):
        m32.train_epoch([(x, x, None)], ntm.ESRLoss(), torch.optim.Adam(m32.parameters(), 1e-3))


# ---- the reduction and the loss adjoints through the raw ABI, against fp64 evaluated in the kernels' operation order.  The single
# entry points launch the `_replicas` kernels with one grid row (R = 1, bper = B); these are the anchors of that code that do not
# go through the replica path: equality, not a tolerance.
def _raw(ntm):
    return ntm._lib.lib(), ntm._lib.ptr, ntm._lib.current_stream()


@pytest.mark.gpu
def test_reduce_of_an_empty_batch_writes_zeros(ntm):
    L, ptr, s = _raw(ntm)
    grad = torch.full((ntm._lib.TRAIN_GRAD_FLOATS,), float("nan"), device="cuda")
    assert L.ntm_gru_train_reduce(None, 0, ptr(grad), s) == 0
    assert torch.equal(grad, torch.zeros_like(grad))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
def test_reduce_adds_the_partials_in_stream_order_in_fp64(ntm, B):
    L, ptr, s = _raw(ntm)
    n = ntm._lib.TRAIN_GRAD_FLOATS
    part = (torch.randn(B, n, generator=torch.Generator().manual_seed(B)) * 10.0 ** torch.randint(-3, 4, (B, n), generator=torch.Generator().manual_seed(7))).float().cuda()
    grad = torch.full((n,), float("nan"), device="cuda")
    assert L.ntm_gru_train_reduce(ptr(part), B, ptr(grad), s) == 0
    acc = torch.zeros(n, dtype=torch.float64, device="cuda")
    for b in range(B):
        acc = acc + part[b].double()
    assert torch.equal(grad, acc.float())


def _loss_inputs(B, T):
    g = torch.Generator().manual_seed(1000 * B + T)
    y = (torch.rand(B, T, generator=g) - 0.5).float()
    t = (0.8 * y + 0.1 * torch.randn(B, T, generator=g) + 0.05).float()
    sums = torch.tensor([float(((t.double() - y.double()) ** 2).sum()), float((t.double() ** 2).sum())], dtype=torch.float64)
    gout = torch.tensor([0.7], dtype=torch.float32)
    return y, t, sums, gout


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(1, 1), (1, 5), (3, 300)])
def test_esr_adjoint_equals_fp64_in_the_kernels_order(ntm, B, T):
    L, ptr, s = _raw(ntm)
    y, t, sums, gout = _loss_inputs(B, T)
    yc, tc, sc, gc = y.cuda(), t.cuda(), sums.cuda(), gout.cuda()
    dy = torch.full((B, T), float("nan"), device="cuda")
    assert L.ntm_esr_grad(ptr(yc), ptr(tc), B, T, ptr(sc), ptr(gc), 1e-5, ptr(dy), s) == 0
    n = float(B * T)
    c = gout.double()[0] * 2.0 / (n * (sums[1] / n + 1e-5))
    want = (c * (y.double() - t.double())).float()
    assert torch.equal(dy.cpu(), want)


def _fma(a, b, c):
    """a * b + c rounded once (float() of a Fraction rounds to nearest even), as v_fma_f64 does."""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _dcpre_adjoint_f64(y, t, pole, sums, gout, eps):
    """esr_dcpre_grad_kernel in Python floats (IEEE fp64), one stream after the other, in the kernel's operation order: the
    causal pass e_f = (w - w_prev) + pole e_f parked as fp32, then q = c e_f + pole q1, dy = q - q1 downwards.  The compiler
    contracts `+ pole * e_f` and `+ pole * q1` into fused multiply-adds (the file is built with hipcc's default contraction and
    this kernel does not switch it off), so these two are rounded once here too."""
    import struct
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]      # noqa: E731
    B, T = y.shape
    Rd = float(np.float32(pole))
    n = float(B * T)
    c = float(gout[0]) * 2.0 / (n * (float(sums[1]) / n + eps))
    out = torch.empty(B, T, dtype=torch.float32)
    for b in range(B):
        prev, ef, park = 0.0, 0.0, []
        for i in range(T):
            wv = float(y[b, i]) - float(t[b, i])
            ef = _fma(Rd, ef, wv - prev)
            prev = wv
            park.append(f32(ef))
        q1 = 0.0
        for i in range(T - 1, -1, -1):
            q = _fma(Rd, q1, c * park[i])
            out[b, i] = f32(q - q1)
            q1 = q
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(1, 1), (3, 5), (65, 7)])
def test_dcpre_adjoint_equals_fp64_in_the_kernels_order(ntm, B, T):
    L, ptr, s = _raw(ntm)
    y, t, sums, gout = _loss_inputs(B, T)
    pole = float(np.float32(ntm.model.DC_PRE_R))
    yc, tc, sc, gc = y.cuda(), t.cuda(), sums.cuda(), gout.cuda()
    dy = torch.full((B, T), float("nan"), device="cuda")
    assert L.ntm_esr_dcpre_grad(ptr(yc), ptr(tc), B, T, pole, ptr(sc), ptr(gc), 1e-5, ptr(dy), s) == 0
    want = _dcpre_adjoint_f64(y, t, pole, sums, gout, 1e-5)
    got = dy.cpu()
    print(f"dcpre adjoint ({B}, {T}): {int((got != want).sum())} of {B * T} elements differ from the fp64 evaluation")
    assert torch.equal(got, want)
