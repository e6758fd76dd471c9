"""GPU: the dilated conv stack of the time-domain critic (ntm_convstack_forward / ntm_convstack_backward,
csrc/convstack_kernels.hip), training.ConvStackFn and ntm_amd.critics.DilatedConvDisc.

The reference everywhere is a torch twin written here -- F.conv1d(..., dilation=d) with g * v / v.flatten(1).norm(dim=1) and
F.leaky_relu(., slope) -- on the CPU with autograd, in float64 (ref64) and again in float32 (ref32).  The bar of every
comparison, elementwise per tensor, is that of tests/test_gpu_critic.py:

    bar = 4 * max(|ref32 - ref64|, E32(kind) * max|ref64|)

E32(kind) is the worst max|ref32 - ref64| / max|ref64| of that tensor kind (output, input gradient, dg, dv, dbias) over this
file's own case table, computed here from the two torch references and never from the device.  The references are computed
once and shared.

In the table's last case (the default twelve-layer stack, 5 million activations) torch's own float32 lands on the other side of
LeakyReLU than float64 at two pre-activations of size 1e-7, which moves its gradients by 1 to 3 % of their largest element: the
E32 of the four gradient kinds over the whole table is that, 1e-2 to 3e-2, and a bar of four times it says little.  So wherever
the two references agree on every LeakyReLU side (the stacks a to d and the small module) a second bar is asserted as well, the
same formula with E32 taken over the cases of a to d alone (4e-7 .. 7e-6): `tight` below.

Measured on an MI355X, worst |got - ref64| / bar per tensor kind:
    the first bar, 25 raw cases     output 0.29   gx, dg, dv, dbias below 0.001
    tight bar, 24 raw cases         output 0.29   gx 0.19   dg 0.17   dv 0.12   dbias 0.25
    module vs golden, tight bar     output 0.020  gx 0.097  dg 0.008  dv 0.042  dbias 0.16;  the four losses 0.17
    LeakyReLU at 0, tight bar: gx 0.15; train_gen's gradient at the generator's output: 0.25"""
import contextlib
import functools
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

KINDS = ("out", "gx", "dg", "dv", "dbias")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_dilated_disc.npz")


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


# ---- the stacks: ((c_in, c_out, k, groups, dilation), ...), slope -------------------------------------------------------------
STACKS = {
    # the reference's shape in small
    "a": (((1, 8, 5, 1, 1), (8, 8, 5, 1, 2), (8, 8, 5, 1, 4), (8, 1, 5, 1, 1)), 0.2),
    # dilation across the frame tile: below it, just beyond a 16-frame MFMA column, far beyond any tile
    "b": (((1, 64, 5, 1, 1), (64, 64, 5, 1, 33), (64, 64, 5, 1, 1089), (64, 1, 5, 1, 1)), 0.2),
    # off-plan edges: channel counts off every tile, groups, three kernel sizes, another slope
    "c": (((3, 24, 3, 1, 7), (24, 40, 4, 8, 130), (40, 5, 2, 1, 3)), 0.05),
    # more than 8 layers
    "d": (tuple((4, 4, 2, 1, 65 if l % 2 else 1) for l in range(13)), 0.2),
    # the default critic
    "e": (((1, 64, 5, 1, 1),) + tuple((64, 64, 5, 1, 2 ** i) for i in range(1, 11)) + ((64, 1, 5, 1, 1),), 0.2),
}


def receptive_field(spec):
    return 1 + sum((k - 1) * d for _, _, k, _, d in spec)


def twin_forward(h, params, spec, slope):
    """h (B, C0, F0) torch, params [(g, v, bias)] torch in h's dtype -> the stack's output."""
    for l, ((_, _, _, groups, d), (g, v, b)) in enumerate(zip(spec, params)):
        w = g.view(-1, 1, 1) * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
        h = F.conv1d(h, w, b, groups=groups, dilation=d)
        if l + 1 < len(spec):
            h = F.leaky_relu(h, slope)
    return h


def twin(x, params, spec, slope, gout, dtype):
    """-> dict(out, gx, dg [n], dv [n], dbias [n]) as float64 numpy, by autograd in `dtype` on the CPU."""
    xx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    ps = [tuple(torch.from_numpy(a).to(dtype).requires_grad_(True) for a in p) for p in params]
    out = twin_forward(xx, ps, spec, slope)
    (out * torch.from_numpy(gout).to(dtype)).sum().backward()
    f = lambda t: t.detach().double().numpy()
    return dict(out=f(out), gx=f(xx.grad), dg=[f(p[0].grad) for p in ps], dv=[f(p[1].grad) for p in ps], dbias=[f(p[2].grad) for p in ps])


def make_case(seed, B, F0, spec):
    """Standard normal x and gout, v ~ N(0, 1 / fan_in), g = (1 .. 1.3) |v|, bias ~ 0.1 N."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, spec[0][0], F0)).astype(np.float32)
    params = []
    for ci, co, k, g, _ in spec:
        v = (rng.standard_normal((co, ci // g, k)) / np.sqrt(ci // g * k)).astype(np.float32)
        norm = np.sqrt((v.astype(np.float64) ** 2).sum(axis=(1, 2)))
        params.append(((norm * rng.uniform(1.0, 1.3, co)).astype(np.float32), v, (0.1 * rng.standard_normal(co)).astype(np.float32)))
    gout = rng.standard_normal((B, spec[-1][1], F0 - receptive_field(spec) + 1)).astype(np.float32)
    return x, params, gout


def tensors(r):
    """[(kind, name, array)] of a twin / device result."""
    rows = [("out", "out", r["out"])] + ([("gx", "gx", r["gx"])] if r.get("gx") is not None else [])
    for kind in ("dg", "dv", "dbias"):
        rows += [(kind, f"{kind}[{l}]", a) for l, a in enumerate(r.get(kind) or [])]
    return rows


def e32_of(pairs):
    """{kind: worst max|ref32 - ref64| / max|ref64|} over [(ref64 result, ref32 result)]."""
    e = {}
    for r64, r32 in pairs:
        for (kind, _, a64), (_, _, a32) in zip(tensors(r64), tensors(r32)):
            e[kind] = max(e.get(kind, 0.0), float(np.abs(a32 - a64).max()) / float(np.abs(a64).max()))
    return e


def check(got, r64, r32, e32, what):
    """Elementwise |got - ref64| <= 4 max(|ref32 - ref64|, E32 max|ref64|) -> the worst error / bar."""
    got = np.asarray(got, np.float64).reshape(np.shape(r64))
    r64, r32 = np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    bar = 4.0 * np.maximum(np.abs(r32 - r64), e32 * float(np.abs(r64).max()))
    ratio = float((np.abs(got - r64) / bar).max())
    print(f"{what}: worst err / bar {ratio:.3f}   max err {float(np.abs(got - r64).max()):.3e}   max|ref64| {float(np.abs(r64).max()):.3e}")
    assert np.isfinite(got).all() and ratio <= 1.0, (what, ratio)
    return ratio


def check_result(got, r64, r32, e32, what):
    """Every tensor of a device result against the twin's -> {kind: worst err / bar}."""
    worst = {}
    g = {name: a for _, name, a in tensors(got)}
    for (kind, name, a64), (_, _, a32) in zip(tensors(r64), tensors(r32)):
        if name in g:
            worst[kind] = max(worst.get(kind, 0.0), check(g[name], a64, a32, e32[kind], f"{what} {name}"))
    return worst


# ---- the raw entry points -------------------------------------------------------------------------------------------
def run_raw(ntm, x, params, spec, slope, gout, want_gx=True, want_pg=True):
    """ntm_convstack_forward + ntm_convstack_backward on numpy inputs -> dict of float32 numpy (every buffer starts as NaN)."""
    L, p = ntm._lib.lib(), ntm._lib.ptr
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    B, C0, F0 = x.shape
    n, lay = len(spec), ntm._lib.conv_layers_d(spec)
    xd, gd = dev(x), dev(gout)
    ps = [tuple(dev(a) for a in q) for q in params]
    arr = lambda i, src: ntm._lib.ptr_array([q[i] for q in src])
    n_saved, n_ws = int(L.ntm_convstack_saved_floats(B, C0, F0, n, lay)), int(L.ntm_convstack_workspace_floats(B, C0, F0, n, lay))
    assert n_saved > 0 and n_ws > 0, L.ntm_last_error()
    saved = nan(n_saved)
    out = nan(*gout.shape)
    rc = L.ntm_convstack_forward(p(xd), B, C0, F0, slope, n, lay, arr(0, ps), arr(1, ps), arr(2, ps), p(saved), p(out), ntm._lib.current_stream())
    assert rc == 0, L.ntm_last_error()
    ws = nan(n_ws)
    gx = nan(*x.shape) if want_gx else None
    gs = [tuple(nan(*a.shape) for a in q) for q in ps]
    none = lambda a: a if want_pg else None
    rc = L.ntm_convstack_backward(p(xd), B, C0, F0, slope, n, lay, arr(0, ps), arr(1, ps), p(saved), p(gd), p(gx), none(arr(0, gs)),
                                  none(arr(1, gs)), none(arr(2, gs)), p(ws), ntm._lib.current_stream())
    assert rc == 0, L.ntm_last_error()
    torch.cuda.synchronize()
    r = dict(out=out.cpu().numpy(), gx=None if gx is None else gx.cpu().numpy())
    if want_pg:
        r.update(dg=[q[0].cpu().numpy() for q in gs], dv=[q[1].cpu().numpy() for q in gs], dbias=[q[2].cpu().numpy() for q in gs])
    return r


def raw_cases():
    """[(stack, B, extra frames)]: F0 = the receptive field (one output frame), + 1, + 37; the default stack once, at + 70."""
    return [(s, B, extra) for s in "abcd" for B in (1, 3) for extra in (0, 1, 37)] + [("e", 1, 70)]


@functools.lru_cache(maxsize=None)
def raw_table():
    """({case: (inputs, ref64, ref32)}, E32 per kind, E32 per kind over the stacks a to d) -- computed once, never written to."""
    rows = {}
    for j, case in enumerate(raw_cases()):
        name, B, extra = case
        spec, slope = STACKS[name]
        inp = make_case(300 + j, B, receptive_field(spec) + extra, spec)
        rows[case] = (inp, twin(inp[0], inp[1], spec, slope, inp[2], torch.float64), twin(inp[0], inp[1], spec, slope, inp[2], torch.float32))
    tight = e32_of([(r[1], r[2]) for case, r in rows.items() if case[0] != "e"])
    return rows, e32_of([(r[1], r[2]) for r in rows.values()]), tight


def test_the_case_table_is_what_its_comments_say():
    assert [receptive_field(STACKS[s][0]) for s in "abcde"] == [33, 4497, 408, 398, 8193]
    assert len(STACKS["d"][0]) == 13 and len(STACKS["e"][0]) == 12 and len(raw_cases()) == 25


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STACKS))
def test_raw_stack_forward_and_backward_against_float64(ntm, name):
    """Output, gx and dg / dv / dbias of every layer at one, two and 38 output frames, B in {1, 3} (the default stack: B = 1, 71
    output frames)."""
    rows, e32, tight = raw_table()
    print("E32:", {k: f"{v:.2e}" for k, v in e32.items()}, "over a to d:", {k: f"{v:.2e}" for k, v in tight.items()})
    spec, slope = STACKS[name]
    worst, worst_t, ran = {}, {}, 0
    for case in raw_cases():
        if case[0] != name:
            continue
        (x, params, gout), r64, r32 = rows[case]
        assert r64["out"].shape == (case[1], spec[-1][1], case[2] + 1)
        got = run_raw(ntm, x, params, spec, slope, gout)
        for k, v in check_result(got, r64, r32, e32, f"{case}").items():
            worst[k] = max(worst.get(k, 0.0), v)
        if name != "e":
            for k, v in check_result(got, r64, r32, tight, f"tight {case}").items():
                worst_t[k] = max(worst_t.get(k, 0.0), v)
        ran += 1
    assert ran == (1 if name == "e" else 6) and set(worst) == set(KINDS)
    print(f"WORST raw {name}:", {k: f"{v:.3f}" for k, v in worst.items()}, "tight:", {k: f"{v:.3f}" for k, v in worst_t.items()})


@pytest.mark.gpu
def test_leaky_relu_takes_the_slope_at_zero(ntm):
    """One output channel of the second layer with g = 0 and bias = 0: its pre-activation is exactly 0, the stored output is 0, and
    the gradient through it takes the slope (torch's subgradient at 0) -- every gradient within the bar."""
    _, e32, tight = raw_table()
    spec, slope = STACKS["a"]
    x, params, gout = make_case(6, 3, receptive_field(spec) + 20, spec)
    params[1][0][5] = 0.0
    params[1][2][5] = 0.0
    r64, r32 = (twin(x, params, spec, slope, gout, dt) for dt in (torch.float64, torch.float32))
    assert float(np.abs(r64["dg"][1][5]).max()) > 0.0                     # the slope is taken: with 0 this would vanish
    got = run_raw(ntm, x, params, spec, slope, gout)
    check_result(got, r64, r32, e32, "LeakyReLU at 0")
    print("WORST LeakyReLU at 0, tight:", {k: f"{v:.3f}" for k, v in check_result(got, r64, r32, tight, "tight LeakyReLU at 0").items()})


def same(a, b):
    return all(np.array_equal(u, v, equal_nan=False) for (_, _, u), (_, _, v) in zip(tensors(a), tensors(b))) and len(tensors(a)) == len(tensors(b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["b", "e"])
def test_equal_calls_equal_bits_and_a_stream_does_not_depend_on_its_batch(ntm, name):
    spec, slope = STACKS[name]
    x, params, gout = raw_table()[0][(name, 3, 37)][0] if name == "b" else make_case(77, 3, receptive_field(spec) + 70, spec)
    a, b = (run_raw(ntm, x, params, spec, slope, gout) for _ in range(2))
    assert same(a, b) and all(np.isfinite(t).all() for _, _, t in tensors(a))
    one = run_raw(ntm, x[:1], params, spec, slope, gout[:1], want_pg=False)
    assert np.array_equal(one["out"], a["out"][:1]) and np.array_equal(one["gx"], a["gx"][:1])
    no_gx = run_raw(ntm, x, params, spec, slope, gout, want_gx=False)
    assert no_gx["gx"] is None and same(no_gx, dict(a, gx=None))
    no_pg = run_raw(ntm, x, params, spec, slope, gout, want_pg=False)
    assert np.array_equal(no_pg["out"], a["out"]) and np.array_equal(no_pg["gx"], a["gx"])


# ---- the module -----------------------------------------------------------------------------------------------------
LR = 1e-3
NAMES = ("weight_g", "weight_v", "bias")


def golden_critic(ntm, golden):
    with contextlib.redirect_stdout(io.StringIO()):
        m = ntm.critics.DilatedConvDisc(layers=4, conv_channels=8, test_in_len=100)
    m.load_state_dict({k[3:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("sd_")})
    return m


class DiscTwin:
    """The same stack in `dtype` on the CPU, on copies of a DilatedConvDisc's parameters."""

    def __init__(self, crit, dtype):
        self.dtype, self.spec, self.slope = dtype, crit.spec(), crit.slope
        self.ps = [tuple(getattr(c, a).detach().cpu().to(dtype).clone().requires_grad_(True) for a in NAMES) for c in crit.convs()]

    def parameters(self):
        return [t for p in self.ps for t in p]

    def __call__(self, x):
        return twin_forward(x.to(self.dtype), self.ps, self.spec, self.slope)

    def train_crit(self, fake, real, opt):
        loss = F.relu(1 + self(fake)).mean() + F.relu(1 - self(real)).mean()
        loss.backward()
        opt.step()
        return loss.item()

    def train_gen(self, y, opt):
        loss = -self(y).mean()
        loss.backward()
        opt.step()
        return loss.item()


def two_calls(crit, fake, real, y0):
    """train_crit twice with Adam(betas 0.5, 0.9) on the critic, then train_gen twice with Adam on the input, no zero_grad in
    between (gradients accumulate; every second call runs at stepped values) -> the four losses."""
    optC = torch.optim.Adam(crit.parameters(), lr=LR, betas=(0.5, 0.9))
    losses = [crit.train_crit(fake, real, optC) for _ in range(2)]
    y = y0.clone().requires_grad_(True)
    optG = torch.optim.Adam([y], lr=LR)
    return np.array(losses + [crit.train_gen(y, optG) for _ in range(2)], np.float64)


@pytest.mark.gpu
def test_dilated_conv_disc_against_the_reference_s_own_numbers(ntm):
    """DilatedConvDisc(layers=4, conv_channels=8, test_in_len=100) with the reference's seed-0 weights on the reference's input:
    the output and every gradient of -D(x).mean() against the float64 twin, the reference's own float32 numbers (golden g26)
    standing as ref32; then the losses train_crit and train_gen return, two calls each with Adam, against the twin's."""
    _, e32, tight = raw_table()
    golden = np.load(GOLDEN)
    crit = golden_critic(ntm, golden)
    t64 = DiscTwin(crit, torch.float64)
    x64 = torch.from_numpy(golden["x"]).double().requires_grad_(True)
    (-t64(x64).mean()).backward()
    conv_keys = [f"layers.{2 * i}" for i in range(4)]
    r32 = dict(out=golden["out"], gx=golden["gx"], dg=[golden[f"g_{k}.weight_g"] for k in conv_keys],
               dv=[golden[f"g_{k}.weight_v"] for k in conv_keys], dbias=[golden[f"g_{k}.bias"] for k in conv_keys])
    with torch.no_grad():
        out64 = t64(x64).numpy()
    r64 = dict(out=out64, gx=x64.grad.numpy(), dg=[p[0].grad.numpy() for p in t64.ps], dv=[p[1].grad.numpy() for p in t64.ps],
               dbias=[p[2].grad.numpy() for p in t64.ps])
    crit = crit.cuda()
    x = torch.from_numpy(golden["x"]).cuda().requires_grad_(True)
    out = crit(x)
    assert out.shape == (3, 1, 68) and crit(x[0]).shape == (1, 68)
    (-out.mean()).backward()
    f = lambda t: t.detach().cpu().numpy()
    got = dict(out=f(out), gx=f(x.grad), dg=[f(c.weight_g.grad) for c in crit.convs()], dv=[f(c.weight_v.grad) for c in crit.convs()],
               dbias=[f(c.bias.grad) for c in crit.convs()])
    worst = check_result(got, r64, r32, e32, "module")
    assert set(worst) == set(KINDS)
    print("WORST module:", {k: f"{v:.3f}" for k, v in worst.items()},
          "tight:", {k: f"{v:.3f}" for k, v in check_result(got, r64, r32, tight, "tight module").items()})

    rng = np.random.default_rng(27)
    fake, real, y0 = (torch.from_numpy(rng.uniform(-1.0, 1.0, (3, 1, 100)).astype(np.float32)) for _ in range(3))
    l64, l32 = (two_calls(DiscTwin(golden_critic(ntm, golden), dt), fake.to(dt), real.to(dt), y0.to(dt)) for dt in (torch.float64, torch.float32))
    crit = golden_critic(ntm, golden).cuda()
    lgot = two_calls(crit, fake.cuda(), real.cuda(), y0.cuda())
    print("losses: device", lgot, "ref64", l64, "ref32", l32)
    check(lgot, l64, l32, float(np.abs(l32 - l64).max()) / float(np.abs(l64).max()), "train_crit x 2, train_gen x 2: loss")


W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"
STEP_B, STEP_T0, STEP_T1 = 2, 256, 8193 + 256


def default_critic(ntm):
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        return ntm.critics.DilatedConvDisc(test_in_len=STEP_T1)


@functools.lru_cache(maxsize=None)
def generator_step(ntm):
    """DiffDelRNN(1, 64, 1, max_delay=64) with the shipped generator weights, B = 2: a warm-up of 256 samples, then one window of
    8193 + 256 whose output goes into the default DilatedConvDisc's train_gen.  Run twice -> [(y, dL/dy, generator parameter
    gradients, critic parameter gradients, loss)]."""
    B, T0, T1 = STEP_B, STEP_T0, STEP_T1
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 1, T0 + T1, generator=g) - 0.5
    n = torch.arange(T0 + T1, dtype=torch.float64)
    d = (32.0 + 30.0 * torch.sin(2 * np.pi * n / 700 + torch.rand(B, 1, generator=g, dtype=torch.float64) * 6)).float().unsqueeze(1)
    sd = {k: torch.as_tensor(v) for k, v in ntm.weights.load_state_dict(W_D).items()}
    runs = []
    for _ in range(2):
        crit = default_critic(ntm).cuda()
        m = ntm.DiffDelRNN(1, 64, 1, max_delay=64).cuda()
        m.load_state_dict(sd)
        for p in m.parameters():
            p.requires_grad_(True)
        m.initialize_hidden(B, m.max_delay)
        m(x[:, :, :T0].cuda(), d[:, :, :T0].cuda(), warmup=True)
        y, _ = m(x[:, :, T0:].cuda(), d[:, :, T0:].cuda())
        y.retain_grad()
        loss = crit.train_gen(y, torch.optim.SGD(m.parameters(), lr=0.0))
        runs.append((y.detach().cpu(), y.grad.cpu(), [p.grad.clone() for p in m.parameters()], [p.grad.clone() for p in crit.parameters()], loss))
    return runs


@pytest.mark.gpu
def test_train_gen_gradient_at_the_generator_output_against_float64(ntm):
    """The gradient train_gen leaves at the generator's output, against the float64 chain at the device's own y (E32 from this
    case's own two references)."""
    y, gy, _, _, loss = generator_step(ntm)[0]
    assert y.shape == (STEP_B, 1, STEP_T1) and gy.shape == y.shape and float(y.abs().max()) > 0.1
    refs = []
    for dt in (torch.float64, torch.float32):
        yy = y.to(dt).clone().requires_grad_(True)
        l = -DiscTwin(default_critic(ntm), dt)(yy).mean()
        l.backward()
        refs.append((yy.grad.double().numpy(), float(l.detach())))
    (g64, l64), (g32, l32) = refs
    e32 = float(np.abs(g32 - g64).max()) / float(np.abs(g64).max())
    print(f"train_gen: loss {loss:.6f} ref64 {l64:.6f} ref32 {l32:.6f}; E32 {e32:.2e}")
    check(gy.numpy(), g64, g32, e32, "train_gen: d/dy")


@pytest.mark.gpu
def test_train_gen_parameter_gradients_are_finite_nonzero_and_reproducible(ntm):
    """Every generator parameter gradient finite and non-zero (five tensors), the critic's 36 parameters are left with gradients
    as torch leaves them, and a second identical run gives the same bits."""
    (_, gy1, g1, c1, l1), (_, gy2, g2, c2, l2) = generator_step(ntm)
    assert len(g1) == 5 and len(c1) == 36
    for a in g1 + c1:
        assert bool(torch.isfinite(a).all()) and bool(a.any())
    assert torch.equal(gy1, gy2) and all(torch.equal(a, c) for a, c in zip(g1 + c1, g2 + c2)) and l1 == l2
