"""GPU: the strided conv stack of the MelGAN critic (ntm_sconvstack_forward / ntm_sconvstack_backward, csrc/sconv_kernels.hip),
training.StridedConvStackFn and ntm_amd.critics.MelGCrit / NLayerDiscriminator.

The reference everywhere is the torch twin of tests/melgan_cases.py on the CPU, in float64 (ref64) and again in float32 (ref32);
the bar, elementwise per tensor, is that of tests/test_gpu_convstack.py, bar = 4 max(|ref32 - ref64|, E32(kind) max|ref64|), with
E32 over this file's own case table and never from the device.  A second, `tight` bar (E32 over the small stacks a to c alone) is
asserted on every case of a to c and on the small module: tests/test_melgan_cpu.py asserts that the two references agree on every
LeakyReLU side in all of them.  Only the configuration-size cases (stack e, the num_D = 1 module, the generator step) are left to
the first bar.  Every test prints its worst error / bar per tensor kind.

Measured on an MI355X, worst |got - ref64| / bar per tensor kind:
    the first bar, 31 raw cases     output 0.10   gx 0.21   dg 0.22   dv 0.12   dbias 0.11
    tight bar, 28 raw cases         output 0.26   gx 0.30   dg 0.22   dv 0.22   dbias 0.11
    module vs golden, tight bar     output 0.058  gx 0.28   dg 0.042  dv 0.12   dbias 0.006;  the four losses 0.25
    feature matching, tight bar     output 0.060  gx 0.11   dg 0.13   dv 0.13   dbias 0.003
    the one-element output small by cancellation: outputs 0.027 of the bar scaled by the terms, gradients gx 0.12
    LeakyReLU at 0, tight bar: gx 0.16; one configuration-size discriminator: gx 0.37; train_gen's gradient at the generator's
    output: 0.40"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from melgan_cases import (CANCELLATION_CASE, KINDS, STACKS, MelTwin, term_magnitudes, check, check_result, e32_of, frames, make_case, raw_cases, raw_table, sides_agree,
                          tensors, twin)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g27_melgan_crit.npz")


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


# ---- the raw entry points -------------------------------------------------------------------------------------------
def run_raw(ntm, x, params, spec, slope, gouts, want_gx=True, want_pg=True):
    """ntm_sconvstack_forward + ntm_sconvstack_backward on numpy inputs -> dict of float32 numpy (every buffer starts as NaN)."""
    L, p = ntm._lib.lib(), ntm._lib.ptr
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    B, C0, F0 = x.shape
    n, lay = len(spec), ntm._lib.conv_layers_s(spec)
    Fr = frames(F0, spec)
    xd, gd = dev(x), [dev(g) for g in gouts]
    ps = [tuple(dev(a) for a in q) for q in params]
    arr = lambda i, src: ntm._lib.ptr_array([q[i] for q in src])
    n_saved, n_ws = int(L.ntm_sconvstack_saved_floats(B, C0, F0, n, lay)), int(L.ntm_sconvstack_workspace_floats(B, C0, F0, n, lay))
    assert n_saved > 0 and n_ws > 0, L.ntm_last_error()
    saved = nan(n_saved)
    outs = [nan(B, spec[l][1], Fr[l + 1]) for l in range(n)]
    rc = L.ntm_sconvstack_forward(p(xd), B, C0, F0, slope, n, lay, arr(0, ps), arr(1, ps), arr(2, ps), p(saved), ntm._lib.ptr_array(outs),
                                  ntm._lib.current_stream())
    assert rc == 0, L.ntm_last_error()
    ws = nan(n_ws)
    gx = nan(*x.shape) if want_gx else None
    gs = [tuple(nan(*a.shape) for a in q) for q in ps]
    none = lambda a: a if want_pg else None
    rc = L.ntm_sconvstack_backward(p(xd), B, C0, F0, slope, n, lay, arr(0, ps), arr(1, ps), p(saved), ntm._lib.ptr_array(outs),
                                   ntm._lib.ptr_array(gd), p(gx), none(arr(0, gs)), none(arr(1, gs)), none(arr(2, gs)), p(ws),
                                   ntm._lib.current_stream())
    assert rc == 0, L.ntm_last_error()
    torch.cuda.synchronize()
    r = dict(out=[o.cpu().numpy() for o in outs], gx=None if gx is None else gx.cpu().numpy())
    if want_pg:
        r.update(dg=[q[0].cpu().numpy() for q in gs], dv=[q[1].cpu().numpy() for q in gs], dbias=[q[2].cpu().numpy() for q in gs])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STACKS))
def test_raw_stack_forward_and_backward_against_float64(ntm, name):
    """Every layer's output, gx and dg / dv / dbias of every layer: a, b at T in {8, 9, 39, 2101}, c at {4, 24, 1205}, B in {1, 3},
    gradients at all outputs; one case per stack again with only the last gradient and with a NULL in the middle; e (configuration
    0) at B = 1, T = 300."""
    rows, e32, tight = raw_table()
    print("E32:", {k: f"{v:.2e}" for k, v in e32.items()}, "over a to c:", {k: f"{v:.2e}" for k, v in tight.items()})
    spec, slope = STACKS[name]
    worst, worst_t, ran = {}, {}, 0
    for case in raw_cases():
        if case[0] != name:
            continue
        (x, params, gouts), r64, r32 = rows[case]
        got = run_raw(ntm, x, params, spec, slope, gouts)
        assert [o.shape[2] for o in got["out"]] == frames(case[2], spec)[1:]
        for k, v in check_result(got, r64, r32, e32, f"{case}").items():
            worst[k] = max(worst.get(k, 0.0), v)
        if name != "e":
            for k, v in check_result(got, r64, r32, tight, f"tight {case}").items():
                worst_t[k] = max(worst_t.get(k, 0.0), v)
        ran += 1
    assert ran == {"a": 10, "b": 10, "c": 8, "e": 3}[name] and set(worst) == set(KINDS)
    print(f"WORST raw {name}:", {k: f"{v:.3f}" for k, v in worst.items()}, "tight:", {k: f"{v:.3f}" for k, v in worst_t.items()})


@pytest.mark.gpu
def test_a_one_element_output_small_by_cancellation(ntm):
    """Stack a at B = 1, T = 9 with the seed the case table leaves out: the last output is ONE element of 7e-4 summed from terms
    of 0.2, so max|ref64| of that tensor is no scale for the rounding of its sum.  Every layer's output is held to the bar's
    formula with the terms of its sums as the scale (max sum |w| |in| + |bias|, float64, from the CPU) and the tight E32; gx and
    the parameter gradients, which are not small by cancellation, to the bar as it is."""
    _, e32, tight = raw_table()
    name, B, T, seed = CANCELLATION_CASE
    spec, slope = STACKS[name]
    x, params, gouts = make_case(seed, B, T, spec)
    r64, r32 = (twin(x, params, spec, slope, gouts, dt) for dt in (torch.float64, torch.float32))
    mags, _ = term_magnitudes(x, params, spec, slope)
    got = run_raw(ntm, x, params, spec, slope, gouts)
    worst = max(check(got["out"][l], r64["out"][l], r32["out"][l], tight["out"], f"cancellation out[{l}]", scale=mags[l]) for l in range(len(spec)))
    print(f"WORST cancellation case, outputs against the terms' scale: {worst:.3f}; last output {r64['out'][-1].ravel()}, terms {mags[-1]:.3f}")
    grads = {k: v for k, v in got.items() if k != "out"}
    print("WORST cancellation case, gradients:", {k: f"{v:.3f}" for k, v in check_result(dict(grads, out=[]), r64, r32, e32, "cancellation").items()})


@pytest.mark.gpu
def test_input_frames_no_tap_reads_get_an_exactly_zero_gradient(ntm):
    """A one-layer stack with k = 2 at stride 3 and pad 1: input frames 1 mod 3 are read by no tap, and their gx is exactly 0 (the
    data gradient's phase with no tap stores the epilogue of 0), the others' is not."""
    spec = ((2, 6, 2, 1, 3, 1, 0),)
    x, params, gouts = make_case(5, 2, 20, spec)
    got = run_raw(ntm, x, params, spec, 0.2, gouts)
    r64 = twin(x, params, spec, 0.2, gouts, torch.float64)
    unread = r64["gx"] == 0.0
    assert unread[:, :, 1::3].all() and not unread[:, :, 0::3].any()
    assert (got["gx"][unread] == 0.0).all() and np.isfinite(got["gx"]).all()


@pytest.mark.gpu
def test_leaky_relu_takes_the_slope_at_zero(ntm):
    """One output channel of the second layer with g = 0 and bias = 0: its pre-activation is exactly 0, the stored output is 0, and
    the gradient through it takes the slope (torch's subgradient at 0) -- every gradient within the bar."""
    _, e32, tight = raw_table()
    spec, slope = STACKS["a"]
    x, params, gouts = make_case(6, 3, 60, spec)
    params[1][0][5] = 0.0
    params[1][2][5] = 0.0
    r64, r32 = (twin(x, params, spec, slope, gouts, dt) for dt in (torch.float64, torch.float32))
    assert sides_agree(r64, r32) and float(np.abs(r64["dg"][1][5]).max()) > 0.0     # the slope is taken: with 0 this would vanish
    got = run_raw(ntm, x, params, spec, slope, gouts)
    assert (got["out"][1][:, 5] == 0.0).all()
    check_result(got, r64, r32, e32, "LeakyReLU at 0")
    print("WORST LeakyReLU at 0, tight:", {k: f"{v:.3f}" for k, v in check_result(got, r64, r32, tight, "tight LeakyReLU at 0").items()})


def same(a, b):
    return all(np.array_equal(u, v, equal_nan=False) for (_, _, u), (_, _, v) in zip(tensors(a), tensors(b))) and len(tensors(a)) == len(tensors(b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_equal_calls_equal_bits_and_a_stream_does_not_depend_on_its_batch(ntm, name):
    spec, slope = STACKS[name]
    T = {"a": 2101, "b": 39, "c": 1205}[name]
    x, params, gouts = raw_table()[0][(name, 3, T, "all")][0]
    a, b = (run_raw(ntm, x, params, spec, slope, gouts) for _ in range(2))
    assert same(a, b) and all(np.isfinite(t).all() for _, _, t in tensors(a))
    one = run_raw(ntm, x[:1], params, spec, slope, [g[:1] for g in gouts], want_pg=False)
    assert all(np.array_equal(o, q[:1]) for o, q in zip(one["out"], a["out"])) and np.array_equal(one["gx"], a["gx"][:1])
    no_gx = run_raw(ntm, x, params, spec, slope, gouts, want_gx=False)
    assert no_gx["gx"] is None and same(no_gx, dict(a, gx=None))
    no_pg = run_raw(ntm, x, params, spec, slope, gouts, want_pg=False)
    assert all(np.array_equal(o, q) for o, q in zip(no_pg["out"], a["out"])) and np.array_equal(no_pg["gx"], a["gx"])


@pytest.mark.gpu
def test_layers_above_the_highest_gradient_get_exact_zeros(ntm):
    """gouts non-NULL only at layer 1: layers 2 .. n-1 return exactly 0 in dg, dv and dbias (their buffers start as NaN), the
    layers below are within the tight bar."""
    _, _, tight = raw_table()
    spec, slope = STACKS["a"]
    x, params, gouts = make_case(8, 3, 39, spec)
    gouts = [None, gouts[1], None, None, None]
    r64, r32 = (twin(x, params, spec, slope, gouts, dt) for dt in (torch.float64, torch.float32))
    got = run_raw(ntm, x, params, spec, slope, gouts)
    for l in range(2, 5):
        assert all((got[k][l] == 0.0).all() for k in ("dg", "dv", "dbias"))
    assert all(float(np.abs(got[k][l]).max()) > 0.0 for k in ("dg", "dv", "dbias") for l in (0, 1))
    check_result(got, r64, r32, tight, "gradient at layer 1 only")


# ---- the module -----------------------------------------------------------------------------------------------------
LR = 1e-3


def golden_critic(ntm, golden):
    m = ntm.critics.MelGCrit(num_D=2, ndf=8, n_layers=2, downsampling_factor=1)
    m.load_state_dict({k[3:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("sd_")})
    return m


def module_result(crit, outs, x):
    f = lambda t: t.detach().cpu().numpy()
    convs = [c for d in crit.model.values() for c in d.convs()]
    return dict(out=[f(o) for s in outs for o in s], gx=f(x.grad), dg=[f(c.weight_g.grad) for c in convs],
                dv=[f(c.weight_v.grad) for c in convs], dbias=[f(c.bias.grad) for c in convs])


def two_calls(crit, fake, real, y0):
    """train_crit twice with Adam(betas 0.5, 0.9) on the critic, then train_gen twice with Adam on the input, no zero_grad in
    between (gradients accumulate; every second call runs at stepped values) -> the four losses."""
    optC = torch.optim.Adam(crit.parameters(), lr=LR, betas=(0.5, 0.9))
    losses = [crit.train_crit(fake, real, optC) for _ in range(2)]
    y = y0.clone().requires_grad_(True)
    optG = torch.optim.Adam([y], lr=LR)
    return np.array(losses + [crit.train_gen(y, optG) for _ in range(2)], np.float64)


def golden_keys(golden):
    conv_keys = [k[:-len(".bias")] for k in str(golden["skeys"]).split(";") if k.endswith(".bias")]
    return conv_keys


@pytest.mark.gpu
def test_melgcrit_against_the_reference_s_own_numbers(ntm):
    """MelGCrit(num_D=2, ndf=8, n_layers=2, downsampling_factor=1) with the reference's seed-0 weights on the reference's input:
    all 2 x 5 outputs and every gradient of sum_disc -scale[-1].mean() against the float64 twin, the reference's own float32
    numbers (golden g27) standing as ref32; then the losses train_crit and train_gen return, two calls each with Adam."""
    _, e32, tight = raw_table()
    golden = np.load(GOLDEN)
    crit = golden_critic(ntm, golden)
    t64 = MelTwin(crit, torch.float64)
    x64 = torch.from_numpy(golden["x"]).double().requires_grad_(True)
    o64 = t64(x64)
    sum(-s[-1].mean() for s in o64).backward()
    r64 = t64.result(o64, x64)
    ck = golden_keys(golden)
    assert len(ck) == 10
    r32 = dict(out=[golden[f"out_{d}_{l}"] for d in range(2) for l in range(5)], gx=golden["gx"], dg=[golden[f"g_{k}.weight_g"] for k in ck],
               dv=[golden[f"g_{k}.weight_v"] for k in ck], dbias=[golden[f"g_{k}.bias"] for k in ck])
    assert sides_agree(dict(out=r64["out"][:5]), dict(out=r32["out"][:5])) and sides_agree(dict(out=r64["out"][5:]), dict(out=r32["out"][5:]))
    crit = crit.cuda()
    x = torch.from_numpy(golden["x"]).cuda().requires_grad_(True)
    outs = crit(x)
    assert len(outs) == 2 and all(len(s) == 5 for s in outs) and outs[0][-1].shape == (3, 1, 40)
    single = crit(x[0])
    assert single[1][-1].shape == (1, 40) and torch.equal(single[1][2], outs[1][2][0])
    sum(-s[-1].mean() for s in outs).backward()
    got = module_result(crit, outs, x)
    worst = check_result(got, r64, r32, e32, "module")
    assert set(worst) == set(KINDS)
    print("WORST module:", {k: f"{v:.3f}" for k, v in worst.items()},
          "tight:", {k: f"{v:.3f}" for k, v in check_result(got, r64, r32, tight, "tight module").items()})

    rng = np.random.default_rng(27)
    fake, real, y0 = (torch.from_numpy(rng.uniform(-1.0, 1.0, (3, 1, 40)).astype(np.float32)) for _ in range(3))
    l64, l32 = (two_calls(MelTwin(golden_critic(ntm, golden), dt), fake.to(dt), real.to(dt), y0.to(dt)) for dt in (torch.float64, torch.float32))
    crit = golden_critic(ntm, golden).cuda()
    lgot = two_calls(crit, fake.cuda(), real.cuda(), y0.cuda())
    print("losses: device", lgot, "ref64", l64, "ref32", l32)
    check(lgot, l64, l32, float(np.abs(l32 - l64).max()) / float(np.abs(l64).max()), "train_crit x 2, train_gen x 2: loss")


def feature_matching(fake, real):
    """mean |feat_fake - feat_real.detach()| over EVERY layer of every discriminator."""
    return sum(F.l1_loss(a, b.detach()) for sf, sr in zip(fake, real) for a, b in zip(sf, sr))


def fm_inputs():
    rng = np.random.default_rng(28)
    return tuple(torch.from_numpy(rng.uniform(-1.0, 1.0, (3, 1, 40)).astype(np.float32)) for _ in range(2))


@pytest.mark.gpu
def test_feature_matching_loss_differentiates_through_every_layer(ntm):
    """A MelGAN feature-matching loss over all 2 x 5 features of the small golden instance: gx (at the fake input) and the parameter
    gradients against float64, tight bar."""
    _, _, tight = raw_table()
    golden = np.load(GOLDEN)
    fake, real = fm_inputs()
    refs = []
    for dt in (torch.float64, torch.float32):
        t = MelTwin(golden_critic(ntm, golden), dt)
        xf = fake.clone().to(dt).requires_grad_(True)
        of = t(xf)
        feature_matching(of, t(real.to(dt))).backward()
        refs.append(t.result(of, xf))
    crit = golden_critic(ntm, golden).cuda()
    xf = fake.cuda().requires_grad_(True)
    of = crit(xf)
    loss = feature_matching(of, crit(real.cuda()))
    loss.backward()
    got = module_result(crit, of, xf)
    worst = check_result(got, refs[0], refs[1], tight, "feature matching")
    assert set(worst) == set(KINDS) and float(np.abs(got["dv"][0]).max()) > 0.0
    print("WORST feature matching, tight:", {k: f"{v:.3f}" for k, v in worst.items()})


@pytest.mark.gpu
def test_one_configuration_size_discriminator_against_float64(ntm):
    """MelGCrit(num_D=1, ndf=16, n_layers=4, downsampling_factor=4), the reference's seven layers (16.9 M / 3 parameters), at
    B = 2, T = 300: the outputs and every gradient of -scale[-1].mean() + a feature term, against float64; E32 from this case's own
    two references."""
    torch.manual_seed(5)
    crit = ntm.critics.MelGCrit(num_D=1, ndf=16, n_layers=4, downsampling_factor=4)
    assert sum(p.numel() for p in crit.parameters()) * 3 == 16924086
    x0 = torch.rand(2, 1, 300, generator=torch.Generator().manual_seed(6)) - 0.5
    refs = []
    for dt in (torch.float64, torch.float32):
        t = MelTwin(crit, dt)
        xx = x0.clone().to(dt).requires_grad_(True)
        o = t(xx)
        (-o[0][-1].mean() + sum(f.abs().mean() for f in o[0][:-1])).backward()
        refs.append(t.result(o, xx))
    assert [o.shape[2] for o in refs[0]["out"]] == [300, 75, 19, 5, 2, 2, 2]
    crit = crit.cuda()
    x = x0.cuda().requires_grad_(True)
    o = crit(x)
    (-o[0][-1].mean() + sum(f.abs().mean() for f in o[0][:-1])).backward()
    got = module_result(crit, o, x)
    worst = check_result(got, refs[0], refs[1], e32_of([tuple(refs)]), "configuration-size discriminator")
    assert set(worst) == set(KINDS)
    print("WORST configuration-size discriminator:", {k: f"{v:.3f}" for k, v in worst.items()})


@pytest.mark.gpu
def test_an_output_without_a_gradient_reaches_the_abi_as_null(ntm, monkeypatch):
    """train_gen uses scale[-1] only: the node hands ntm_sconvstack_backward a gouts array whose other entries are NULL (torch
    materialises no zero tensors for them).  With a loss on layer 1's feature alone the array is (NULL, g, NULL, NULL, NULL), and
    the layers above it come back with parameter gradients of exactly 0."""
    golden = np.load(GOLDEN)
    crit = golden_critic(ntm, golden).cuda()
    seen = []
    real = ntm._lib.ptr_array

    def spy(tensors):
        seen.append([t is None for t in tensors])
        return real(tensors)
    monkeypatch.setattr(ntm._lib, "ptr_array", spy)
    y = torch.from_numpy(golden["x"]).cuda().requires_grad_(True)
    crit.train_gen(y, torch.optim.SGD([y], lr=0.0))
    assert seen.count([True, True, True, True, False]) == 2 and bool(y.grad.any())          # one gouts array per discriminator
    assert all(bool(p.grad.any()) for p in crit.parameters())
    seen.clear()
    crit.zero_grad(set_to_none=True)
    feats = crit(torch.from_numpy(golden["x"]).cuda())
    (feats[0][1] ** 2).sum().backward()
    assert seen.count([True, False, True, True, True]) == 1 and seen.count([True, True, True, True, False]) == 0
    convs = crit.model["disc_0"].convs()
    for l, c in enumerate(convs):
        for t in (c.weight_g, c.weight_v, c.bias):
            assert bool(t.grad.any()) == (l <= 1) and bool(torch.isfinite(t.grad).all()), l
    assert all(p.grad is None for p in crit.model["disc_1"].parameters())


@pytest.mark.gpu
def test_an_in_place_edit_of_a_returned_feature_raises_torch_s_version_error(ntm):
    golden = np.load(GOLDEN)
    crit = golden_critic(ntm, golden).cuda()
    outs = crit(torch.from_numpy(golden["x"]).cuda())
    outs[0][1].mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        outs[0][-1].mean().backward()


W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"
STEP_B, STEP_T0, STEP_T1 = 2, 256, 1024


def config0_critic(ntm):
    torch.manual_seed(11)
    return ntm.critics.MelGCrit(num_D=3, ndf=16, n_layers=4, downsampling_factor=4)


@functools.lru_cache(maxsize=None)
def generator_step(ntm):
    """DiffDelRNN(1, 64, 1, max_delay=64) with the shipped generator weights, B = 2: a warm-up of 256 samples, then one window of
    1024 whose output goes into the configuration-0 MelGCrit's train_gen.  Run twice -> [(y, dL/dy, generator parameter gradients,
    critic parameter gradients, loss)]."""
    B, T0, T1 = STEP_B, STEP_T0, STEP_T1
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 1, T0 + T1, generator=g) - 0.5
    n = torch.arange(T0 + T1, dtype=torch.float64)
    d = (32.0 + 30.0 * torch.sin(2 * np.pi * n / 700 + torch.rand(B, 1, generator=g, dtype=torch.float64) * 6)).float().unsqueeze(1)
    sd = {k: torch.as_tensor(v) for k, v in ntm.weights.load_state_dict(W_D).items()}
    runs = []
    for _ in range(2):
        crit = config0_critic(ntm).cuda()
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
        l = sum(-s[-1].mean() for s in MelTwin(config0_critic(ntm), dt)(yy))
        l.backward()
        refs.append((yy.grad.double().numpy(), float(l.detach())))
    (g64, l64), (g32, l32) = refs
    e32 = float(np.abs(g32 - g64).max()) / float(np.abs(g64).max())
    print(f"train_gen: loss {loss:.6f} ref64 {l64:.6f} ref32 {l32:.6f}; E32 {e32:.2e}")
    check(gy.numpy(), g64, g32, e32, "train_gen: d/dy")


@pytest.mark.gpu
def test_train_gen_parameter_gradients_are_finite_nonzero_and_reproducible(ntm):
    """Every generator parameter gradient finite and non-zero (five tensors), the critic's 63 parameters are left with gradients
    as torch leaves them, and a second identical run gives the same bits."""
    (_, gy1, g1, c1, l1), (_, gy2, g2, c2, l2) = generator_step(ntm)
    assert len(g1) == 5 and len(c1) == 63
    for a in g1 + c1:
        assert bool(torch.isfinite(a).all()) and bool(a.any())
    assert torch.equal(gy1, gy2) and all(torch.equal(a, c) for a, c in zip(g1 + c1, g2 + c2)) and l1 == l2
