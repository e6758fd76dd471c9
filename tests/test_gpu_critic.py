"""GPU: the conv stack of the spectral critics (ntm_speccrit_forward / ntm_speccrit_backward, csrc/critic_kernels.hip),
training.SpecCritFn and ntm_amd.critics.

The reference everywhere is a torch twin written here -- F.conv1d with g * v / v.flatten(1).norm(dim=1), F.leaky_relu(., 0.2) and
the log head log10(clamp(x, min=float32(1e-5))) -- on the CPU with autograd, in float64 (ref64) and again in float32 (ref32).
The bar of every comparison, elementwise per tensor:

    bar = 4 * max(|ref32 - ref64|, E32(kind) * max|ref64|)

E32(kind) is the worst max|ref32 - ref64| / max|ref64| of that tensor kind (output, input gradient, dg, dv, dbias; for the
module also the loss) over the test's own case table, computed here from the two torch references: the project's rule, factor 4
over torch's own float32.  The references are computed once and shared.

Measured on an MI355X, worst |got - ref64| / bar per tensor kind:
    raw stack, 144 cases    output 0.14   gx 0.36   dg 0.90   dv 0.19   dbias 0.25
    modules, three cases    output 0.18   loss 0.43   dg 0.087   dv 0.11   dbias 0.19
    head edges: gx 0.055; LeakyReLU at 0: gx 0.098; train_gen's gradient at the generator's output: 0.008
The 0.90 is one scalar -- dg of the last layer at C0 = 1025, B = 1, two output frames, which cancels to 1.5 % of its terms and on
which torch's own float32 happens to be four times nearer float64 than its output errors predict; every other dg of the raw table
is at or below 0.07.  The first form of the conv kernel (one fmaf chain through all input channels instead of a sum per slab of 16)
was at 2.1 on that scalar."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import noise_pair

FLOOR = float(np.float32(1e-5))
KINDS = ("out", "gx", "dg", "dv", "dbias")


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


# ---- the twin -------------------------------------------------------------------------------------------------------
def stack(C0, ks, layers=4, chan_in=16, chan_fac=4, g_fac=16):
    """((c_in, c_out, k, groups), ...) as SpecCrit's constructor lays the convs out behind C0 bins."""
    spec = [(C0, chan_in, 10, 1)]
    for _ in range(layers - 2):
        out = min(chan_in * chan_fac, 1024)
        spec.append((chan_in, out, ks, out // g_fac))
        chan_in = out
    return tuple(spec + [(chan_in, chan_in, 5, 1), (chan_in, 1, 3, 1)])


def receptive_field(spec):
    return 1 + sum(k - 1 for _, _, k, _ in spec)


def twin_forward(h, params, spec, floor):
    """h (B, C0, F0) torch, params [(g, v, bias)] torch in h's dtype -> the stack's output."""
    if floor > 0:
        h = torch.log10(torch.clamp(h, min=floor))
    for l, ((_, _, _, groups), (g, v, b)) in enumerate(zip(spec, params)):
        w = g.view(-1, 1, 1) * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
        h = F.conv1d(h, w, b, groups=groups)
        if l + 1 < len(spec):
            h = F.leaky_relu(h, 0.2)
    return h


def twin(x, params, spec, floor, gout, dtype):
    """-> dict(out, gx, dg [n], dv [n], dbias [n]) as float64 numpy, by autograd in `dtype` on the CPU."""
    xx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    ps = [tuple(torch.from_numpy(a).to(dtype).requires_grad_(True) for a in p) for p in params]
    out = twin_forward(xx, ps, spec, floor)
    (out * torch.from_numpy(gout).to(dtype)).sum().backward()
    f = lambda t: t.detach().double().numpy()
    return dict(out=f(out), gx=f(xx.grad), dg=[f(p[0].grad) for p in ps], dv=[f(p[1].grad) for p in ps], dbias=[f(p[2].grad) for p in ps])


def make_case(seed, B, C0, F0, spec, floor):
    """x (the power of unit-variance complex noise, lifted by 1e-3 so that every cell is far above the floor, where the head
    is on; standard normal where it is off), standard normal gout, v ~ N(0, 1 / fan_in), g = (1 .. 1.3) |v|, bias ~ 0.1 N."""
    rng = np.random.default_rng(seed)
    if floor > 0:
        x = (rng.standard_normal((B, C0, F0)) ** 2 + rng.standard_normal((B, C0, F0)) ** 2 + 1e-3).astype(np.float32)
    else:
        x = rng.standard_normal((B, C0, F0)).astype(np.float32)
    params = []
    for ci, co, k, g in spec:
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


def check(got, r64, r32, e32, what, scale=None):
    """Elementwise |got - ref64| <= 4 max(|ref32 - ref64|, E32 max|ref64|) -> the worst error / bar.  `scale` stands in for
    max|ref64| where the caller knows the tensor to be a difference of larger terms that cancels exactly."""
    got = np.asarray(got, np.float64).reshape(np.shape(r64))
    r64, r32 = np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    bar = 4.0 * np.maximum(np.abs(r32 - r64), e32 * (float(np.abs(r64).max()) if scale is None else scale))
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
def run_raw(ntm, x, params, spec, floor, gout, want_gx=True, want_pg=True):
    """ntm_speccrit_forward + ntm_speccrit_backward on numpy inputs -> dict of float32 numpy (every buffer starts as NaN)."""
    L, p = ntm._lib.lib(), ntm._lib.ptr
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    B, C0, F0 = x.shape
    n, lay = len(spec), ntm._lib.conv_layers(spec)
    xd, gd = dev(x), dev(gout)
    ps = [tuple(dev(a) for a in q) for q in params]
    arr = lambda i, src: ntm._lib.ptr_array([q[i] for q in src])
    saved = nan(int(L.ntm_speccrit_saved_floats(B, C0, F0, n, lay)))
    out = nan(*gout.shape)
    rc = L.ntm_speccrit_forward(p(xd), B, C0, F0, floor, n, lay, arr(0, ps), arr(1, ps), arr(2, ps), p(saved), p(out), ntm._lib.current_stream())
    assert rc == 0, L.ntm_last_error()
    ws = nan(int(L.ntm_speccrit_workspace_floats(B, C0, F0, n, lay)))
    gx = nan(*x.shape) if want_gx else None
    gs = [tuple(nan(*a.shape) for a in q) for q in ps]
    none = lambda a: a if want_pg else None
    rc = L.ntm_speccrit_backward(p(xd), B, C0, F0, floor, n, lay, arr(0, ps), arr(1, ps), p(saved), p(gd), p(gx), none(arr(0, gs)),
                                 none(arr(1, gs)), none(arr(2, gs)), p(ws), ntm._lib.current_stream())
    assert rc == 0, L.ntm_last_error()
    torch.cuda.synchronize()
    r = dict(out=out.cpu().numpy(), gx=None if gx is None else gx.cpu().numpy())
    if want_pg:
        r.update(dg=[q[0].cpu().numpy() for q in gs], dv=[q[1].cpu().numpy() for q in gs], dbias=[q[2].cpu().numpy() for q in gs])
    return r


HEADS = [(33, 21), (65, 17), (160, 7), (1025, 7)]
PLANS = {"reference": dict(), "small": dict(layers=3, chan_in=8, chan_fac=2, g_fac=4), "deep": dict(layers=5, chan_in=16, chan_fac=2, g_fac=16)}


def raw_cases():
    """[(C0, ks, plan, B, extra frames, floor)]: F0 = the receptive field (one output frame), + 1, + 37."""
    return [(C0, ks, plan, B, extra, floor) for C0, ks in HEADS for plan in PLANS for B in (1, 3) for extra in (0, 1, 37)
            for floor in (FLOOR, 0.0)]


@functools.lru_cache(maxsize=None)
def raw_table():
    """({case: (inputs, ref64, ref32)}, E32 per kind) -- computed once, never written to."""
    rows = {}
    for j, case in enumerate(raw_cases()):
        C0, ks, plan, B, extra, floor = case
        spec = stack(C0, ks, **PLANS[plan])
        inp = make_case(100 + j, B, C0, receptive_field(spec) + extra, spec, floor)
        rows[case] = (spec, inp, twin(inp[0], inp[1], spec, floor, inp[2], torch.float64), twin(inp[0], inp[1], spec, floor, inp[2], torch.float32))
    return rows, e32_of([(r[2], r[3]) for r in rows.values()])


@pytest.mark.gpu
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("C0,ks", HEADS)
def test_raw_stack_forward_and_backward_against_float64(ntm, C0, ks, plan):
    """Output, gx and dg / dv / dbias of every layer at one, two and 38 output frames, B in {1, 3}, with and without the log head:
    the reference's channel plan (16, 64 in 4 groups, 256 in 16 groups, 256, 1) and two plans off it."""
    rows, e32 = raw_table()
    print("E32:", {k: f"{v:.2e}" for k, v in e32.items()})
    worst = {}
    for case in raw_cases():
        if case[:3] != (C0, ks, plan):
            continue
        spec, (x, params, gout), r64, r32 = rows[case]
        assert r64["out"].shape[2] == case[4] + 1
        got = run_raw(ntm, x, params, spec, case[5], gout)
        for k, v in check_result(got, r64, r32, e32, f"{case}").items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"WORST raw C0={C0} ks={ks} {plan}:", {k: f"{v:.3f}" for k, v in worst.items()})


@pytest.mark.gpu
def test_head_edges_zero_the_floor_and_the_float_below_it(ntm):
    """Cells of x exactly 0, exactly float32(1e-5) and the float just below it: gx is exactly 0 at the first and the third (the
    clamp's gradient), within the bar at the second (it passes at equality) and everywhere else."""
    _, e32 = raw_table()
    spec = stack(33, 7)
    x, params, gout = make_case(5, 2, 33, receptive_field(spec) + 9, spec, FLOOR)
    below = np.nextafter(np.float32(FLOOR), np.float32(0))
    cells = {0.0: [(0, 0, 0), (1, 32, 5), (0, 17, 36)], FLOOR: [(0, 1, 0), (1, 31, 36), (1, 5, 11)], float(below): [(0, 2, 0), (1, 30, 36), (0, 9, 20)]}
    for val, where in cells.items():
        for c in where:
            x[c] = val
    r64, r32 = (twin(x, params, spec, FLOOR, gout, dt) for dt in (torch.float64, torch.float32))
    got = run_raw(ntm, x, params, spec, FLOOR, gout)
    for val, where in cells.items():
        for c in where:
            assert (got["gx"][c] == 0.0) == (val != FLOOR) and (r64["gx"][c] == 0.0) == (val != FLOOR), (val, c, got["gx"][c], r64["gx"][c])
    check_result(got, r64, r32, e32, "head edges")


@pytest.mark.gpu
def test_leaky_relu_takes_the_slope_at_zero(ntm):
    """One output channel of the second layer with g = 0 and bias = 0: its pre-activation is exactly 0, the stored output is 0, and
    the gradient through it takes the slope 0.2 (torch's subgradient at 0) -- every gradient within the bar."""
    _, e32 = raw_table()
    spec = stack(33, 7)
    x, params, gout = make_case(6, 3, 33, receptive_field(spec) + 20, spec, FLOOR)
    params[1][0][5] = 0.0
    params[1][2][5] = 0.0
    r64, r32 = (twin(x, params, spec, FLOOR, gout, dt) for dt in (torch.float64, torch.float32))
    assert float(np.abs(r64["dg"][1][5]).max()) > 0.0                     # the slope is taken: with 0 this would vanish
    check_result(run_raw(ntm, x, params, spec, FLOOR, gout), r64, r32, e32, "LeakyReLU at 0")


def same(a, b):
    return all(np.array_equal(u, v, equal_nan=False) for (_, _, u), (_, _, v) in zip(tensors(a), tensors(b))) and len(tensors(a)) == len(tensors(b))


@pytest.mark.gpu
@pytest.mark.parametrize("C0,ks,plan,floor", [(33, 21, "reference", FLOOR), (160, 7, "deep", 0.0), (65, 17, "small", FLOOR)])
def test_equal_calls_equal_bits_and_a_stream_does_not_depend_on_its_batch(ntm, C0, ks, plan, floor):
    spec, (x, params, gout), _, _ = raw_table()[0][(C0, ks, plan, 3, 37, floor)]
    a, b = (run_raw(ntm, x, params, spec, floor, gout) for _ in range(2))
    assert same(a, b) and all(np.isfinite(t).all() for _, _, t in tensors(a))
    for s in range(3):
        one = run_raw(ntm, x[s:s + 1], params, spec, floor, gout[s:s + 1], want_pg=False)
        assert np.array_equal(one["out"], a["out"][s:s + 1]) and np.array_equal(one["gx"], a["gx"][s:s + 1]), s
    no_gx = run_raw(ntm, x, params, spec, floor, gout, want_gx=False)
    assert no_gx["gx"] is None and same(no_gx, dict(a, gx=None))
    no_pg = run_raw(ntm, x, params, spec, floor, gout, want_pg=False)
    assert np.array_equal(no_pg["out"], a["out"]) and np.array_equal(no_pg["gx"], a["gx"])


# ---- the modules ----------------------------------------------------------------------------------------------------
def model_like_pair(seed, B, T):
    """A saturating model against a slightly different one, small noise on both (the family of tests/test_gpu_stft_grad.py)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (B, T))
    y = 0.5 * np.tanh(1.7 * x) + 1e-3 * rng.standard_normal((B, T))
    t = 0.6 * np.tanh(2.0 * x) + 1e-3 * rng.standard_normal((B, T))
    return y.astype(np.float32), t.astype(np.float32)


COMMON = dict(layers=4, chan_in=16, chan_fac=4, stride=1, g_fac=16, test_in_len=2048, log=True)
SPEC_PARS = dict(scales=[64, 128], kernel_sizes=[21, 7], hop_sizes=[16, 32], **COMMON)
MEL_PARS = dict(scales=[256], kernel_sizes=[7], hop_sizes=[64], tf_rep="mel", **COMMON)
MODULE_CASES = {"noise": (SPEC_PARS, noise_pair), "model": (SPEC_PARS, model_like_pair), "mel": (MEL_PARS, noise_pair)}
MOD_B, MOD_T, LR = 3, 2048, 0.05


def make_critic(ntm, pars):
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        return ntm.critics.MultiSpecCrit(**pars)


def _power_t(s, n_fft):
    X = torch.stft(s, n_fft, n_fft // 4, n_fft, torch.hann_window(n_fft, dtype=s.dtype), return_complex=True)
    return X.real ** 2 + X.imag ** 2


class CriticTwin:
    """The same architecture from torch.stft on, in `dtype` on the CPU, on copies of a MultiSpecCrit's parameters."""

    def __init__(self, crit, dtype):
        self.dtype, self.models = dtype, []
        for m in crit.models:
            ps = [tuple(getattr(c, a).detach().cpu().to(dtype).clone().requires_grad_(True) for a in ("weight_g", "weight_v", "bias"))
                  for c in m.convs()]
            basis = m.layers[0].mel_basis.detach().cpu().to(dtype) if m.tf_rep == "mel" else None
            self.models.append((m.scale, m.spec(), ps, basis, FLOOR if m.log else 0.0))

    def parameters(self):
        return [t for _, _, ps, _, _ in self.models for p in ps for t in p]

    def __call__(self, audio):
        outs = []
        for n_fft, spec, ps, basis, floor in self.models:
            P = _power_t(audio.to(self.dtype), n_fft)
            outs.append(twin_forward(P if basis is None else torch.matmul(basis, P), ps, spec, floor))
        return outs

    def train_crit(self, fake, real, opt):
        loss = sum(F.relu(1 + s).mean() for s in self(fake)) + sum(F.relu(1 - s).mean() for s in self(real))
        loss.backward()
        opt.step()
        return loss.item()

    def train_gen_loss(self, y):
        return sum(-s.mean() for s in self(y))


def module_result(crit, fake, real, is_twin):
    """forward's list at the starting weights, then train_crit twice with SGD and no zero_grad -> dict(out, loss, dg, dv, dbias)."""
    with torch.no_grad():
        outs = [o.detach().double().cpu().numpy() for o in crit(fake)]
    # (weight_g, weight_v, bias) per conv, scale by scale: the twin's order (nn.Module.parameters() lists the bias first)
    params = crit.parameters() if is_twin else [getattr(c, n) for m in crit.models for c in m.convs() for n in ("weight_g", "weight_v", "bias")]
    opt = torch.optim.SGD(params, lr=LR)
    losses = [crit.train_crit(fake, real, opt) for _ in range(2)]
    grads = [p.grad.detach().double().cpu().numpy() for p in params]
    return dict(out=outs, loss=np.array(losses, np.float64), dg=grads[0::3], dv=grads[1::3], dbias=grads[2::3])


def module_tensors(r):
    return ([("out", f"out[{i}]", a) for i, a in enumerate(r["out"])] + [("loss", "loss", r["loss"])]
            + [(k, f"{k}[{i}]", a) for k in ("dg", "dv", "dbias") for i, a in enumerate(r[k])])


@functools.lru_cache(maxsize=None)
def module_table(ntm):
    """({case: (fake, real, ref64, ref32)}, E32 per kind)."""
    rows, e = {}, {}
    for j, (name, (pars, family)) in enumerate(MODULE_CASES.items()):
        fake, real = (torch.from_numpy(a) for a in family(40 + j, MOD_B, MOD_T))
        refs = [module_result(CriticTwin(make_critic(ntm, pars), dt), fake, real, True) for dt in (torch.float64, torch.float32)]
        rows[name] = (fake, real, refs[0], refs[1])
        for (kind, _, a64), (_, _, a32) in zip(module_tensors(refs[0]), module_tensors(refs[1])):
            if np.abs(a64).max() > 0:                   # (the last layer's dbias is exactly 0: see the test)
                e[kind] = max(e.get(kind, 0.0), float(np.abs(a32 - a64).max()) / float(np.abs(a64).max()))
    return rows, e


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(MODULE_CASES))
def test_multi_spec_crit_forward_and_train_crit_against_the_float64_chain(ntm, case):
    """MultiSpecCrit(scales [64, 128], kernel sizes [21, 7], log) and one tf_rep='mel' critic (n_fft 256, ks 7), B = 3, T = 2048:
    forward's list, train_crit's returned loss and the parameter gradients it leaves, called twice with SGD and no zero_grad (they
    accumulate, and the second call runs at the stepped weights), against the float64 chain from torch.stft.

    The last layer's dbias is the one tensor without a scale of its own: d/db of mean(1 + D(fake)) + mean(1 - D(real)) is
    sum(1/N) - sum(1/N) = 0 exactly in float64, while each of the two terms, which arrive in separate backward calls and are
    rounded before autograd adds them, is 1.  Its bar is therefore taken at the scale 1 of those terms instead of max|ref64| = 0."""
    rows, e32 = module_table(ntm)
    print("E32:", {k: f"{v:.2e}" for k, v in e32.items()})
    fake, real, r64, r32 = rows[case]
    crit = make_critic(ntm, MODULE_CASES[case][0]).cuda()
    outs = crit(fake.cuda().unsqueeze(1))
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(MOD_B,) + a.shape[1:] for a in r64["out"]]
    got = module_result(crit, fake.cuda().unsqueeze(1), real.cuda().unsqueeze(1), False)
    worst = {}
    for (kind, name, a), (_, _, a64), (_, _, a32) in zip(module_tensors(got), module_tensors(r64), module_tensors(r32)):
        scale = 1.0 if kind == "dbias" and not np.abs(a64).max() > 0 else None
        worst[kind] = max(worst.get(kind, 0.0), check(a, a64, a32, e32[kind], f"{case} {name}", scale))
    print(f"WORST module {case}:", {k: f"{v:.3f}" for k, v in worst.items()})
    # the reference's .squeeze(): a batch of one gives (bins, frames) behind the transform and an output (1, F_out)
    one = crit(fake[:1].cuda().unsqueeze(1))
    assert [tuple(o.shape) for o in one] == [(1, a.shape[2]) for a in r64["out"]]


W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"
STEP_B, STEP_T0, STEP_T1 = 2, 256, 2048


@functools.lru_cache(maxsize=None)
def generator_step(ntm):
    """DiffDelRNN(1, 64, 1, max_delay=64) with the shipped generator weights, B = 2: a warm-up of 256 samples, then one window of
    2048 whose output goes into MultiSpecCrit.train_gen (the critic of the module test).  Run twice -> [(y, dL/dy, generator
    parameter gradients, critic parameter gradients, loss)]."""
    B, T0, T1 = STEP_B, STEP_T0, STEP_T1
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 1, T0 + T1, generator=g) - 0.5
    n = torch.arange(T0 + T1, dtype=torch.float64)
    d = (32.0 + 30.0 * torch.sin(2 * np.pi * n / 700 + torch.rand(B, 1, generator=g, dtype=torch.float64) * 6)).float().unsqueeze(1)
    sd = {k: torch.as_tensor(v) for k, v in ntm.weights.load_state_dict(W_D).items()}
    runs = []
    for _ in range(2):
        crit = make_critic(ntm, SPEC_PARS).cuda()
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
    """The gradient train_gen leaves at the generator's output, against the float64 chain from torch.stft at the device's own y
    (E32 from this case's own two references)."""
    y, gy, _, _, loss = generator_step(ntm)[0]
    assert y.shape == (STEP_B, 1, STEP_T1) and float(y.abs().max()) > 0.1
    refs = []
    for dt in (torch.float64, torch.float32):
        yy = y[:, 0].to(dt).clone().requires_grad_(True)
        l = CriticTwin(make_critic(ntm, SPEC_PARS), dt).train_gen_loss(yy)
        l.backward()
        refs.append((yy.grad.double().numpy(), float(l.detach())))
    (g64, l64), (g32, l32) = refs
    e32 = float(np.abs(g32 - g64).max()) / float(np.abs(g64).max())
    print(f"train_gen: loss {loss:.6f} ref64 {l64:.6f} ref32 {l32:.6f}; E32 {e32:.2e}")
    check(gy[:, 0].numpy(), g64, g32, e32, "train_gen: d/dy")


@pytest.mark.gpu
def test_train_gen_parameter_gradients_are_finite_nonzero_and_reproducible(ntm):
    """Every generator parameter gradient finite and non-zero (five tensors), the critic's parameters are left with gradients as
    torch leaves them, and a second identical run gives the same bits."""
    (_, gy1, g1, c1, l1), (_, gy2, g2, c2, l2) = generator_step(ntm)
    assert len(g1) == 5 and len(c1) == 30
    for a in g1 + c1:
        assert bool(torch.isfinite(a).all()) and bool(a.any())
    assert torch.equal(gy1, gy2) and all(torch.equal(a, c) for a, c in zip(g1 + c1, g2 + c2)) and l1 == l2
