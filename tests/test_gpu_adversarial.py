"""GPU: the adversarial run on the device -- training.AdvHeadFn (ntm_adv_head_forward / ntm_adv_head_backward,
csrc/advhead_kernels.hip) and ntm_amd.adversarial.Trainer.

The head.  Loss: |got - ref64| <= (2 K + 1) 2^-24 sum|means| with ref64 the formula in float64 on the same float32 outputs (one
rounding per mean and per add).  Gradients: torch.equal to torch's autograd on the reference's expression on the same device
tensors.

The loop.  Golden g28 (tools/make_goldens_adversarial.py) is the reference's own loop on the CPU, as it runs (ref32) and in double
(ref64), with E32 per kind of tensor -- the worst max|ref32 - ref64| / max|ref64| over the tensors of that kind -- stored beside
the results.  The bar of every comparison is the project's,

    |got - ref64| <= 4 max(|ref32 - ref64|, E32(kind) max|ref64|)  =  4 E32(kind) max|ref64|

(no element of a tensor differs between the references by more than the worst ratio of its kind times its largest element, so
the second term is the maximum everywhere).  Where a float64 twin stands in for the reference (the three critic families, the
spectral run) both references are torch on the CPU, built as tests/test_gpu_critic.py, test_gpu_convstack.py and melgan_cases.py
build theirs, and E32 comes from that case's own pair.

One tensor has no scale of its own, as in tests/test_gpu_critic.py: the last layer's dbias of a critic whose hinge terms are all
active is sum(1/N) - sum(1/N) = 0 exactly in float64 while each of the two sums is 1; its bar is taken at that scale 1."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_convstack as conv_tests
import test_gpu_critic as spec_tests
from melgan_cases import MelTwin, check

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g28_adversarial.npz")
W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"
U = 2.0 ** -24
NAMES = ("weight_g", "weight_v", "bias")


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


# ---- the head ---------------------------------------------------------------------------------------------------------------
ELEMS = (1, 63, 64, 65, 257, 4097)
ONE = np.float32(1.0)
SPECIALS = np.array([-1.0, 1.0, np.nextafter(-ONE, np.float32(0)), np.nextafter(-ONE, np.float32(-2)), np.nextafter(ONE, np.float32(0)),
                     np.nextafter(ONE, np.float32(2)), 50.0, -50.0], np.float32)


def head_outputs(seed, K, rows, n_fake, elems):
    """K float32 outputs [rows, ...] around the hinges: N(0, 2) with -1, +1, their neighbours by one ulp and +-50 planted in both
    halves; the row lengths rotate through ELEMS from `elems` on, one output is 3-D, and with K > 1 the last one is all inactive
    (fake rows at -3, real rows at +3: every term is 0)."""
    rng = np.random.default_rng(seed)
    outs = []
    for k in range(K):
        e = elems if k == 0 or elems not in ELEMS else ELEMS[(ELEMS.index(elems) + k) % len(ELEMS)]
        o = (2.0 * rng.standard_normal((rows, e))).astype(np.float32)
        for half in (o[:n_fake].reshape(-1), o[n_fake:].reshape(-1)):
            sp = np.roll(SPECIALS, seed + k)[:half.size]
            half[rng.permutation(half.size)[:sp.size]] = sp
        if K > 1 and k == K - 1:
            o[:n_fake], o[n_fake:] = -3.0, 3.0
        outs.append(o.reshape(rows, 1, e) if k == 1 else o)
    return outs


def head_ref64(mode, n_fake, outs):
    """The formula in float64 on the float32 outputs -> (loss, sum of |means|)."""
    o = [a.astype(np.float64) for a in outs]
    if mode == "gen":
        means = [-a.mean() for a in o]
    else:
        means = [np.maximum(1 + a[:n_fake], 0).mean() for a in o] + [np.maximum(1 - a[n_fake:], 0).mean() for a in o]
    return float(sum(means)), float(sum(abs(m) for m in means))


def head_torch(mode, n_fake, leaves):
    """The reference's expression in torch on the device tensors."""
    loss = 0
    if mode == "gen":
        for scale in leaves:
            loss += -scale.mean()
    else:
        for scale in leaves:
            loss += F.relu(1 + scale[:n_fake]).mean()
        for scale in leaves:
            loss += F.relu(1 - scale[n_fake:]).mean()
    return loss


def run_head(ntm, mode, n_fake, outs, gout):
    """-> (loss tensor, [grad]) of AdvHeadFn and of torch's autograd, each on leaves of its own."""
    both = []
    for fn in (lambda l: ntm.training.AdvHeadFn.apply(mode, n_fake, *l), lambda l: head_torch(mode, n_fake, l)):
        leaves = [torch.from_numpy(o).cuda().requires_grad_(True) for o in outs]
        loss = fn(leaves)
        loss.backward(None if gout is None else torch.tensor(gout, device="cuda"))
        both.append((loss.detach(), [l.grad for l in leaves]))
    return both


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["crit", "gen"])
@pytest.mark.parametrize("rows,n_fake", [(2, 1), (4, 3)])
@pytest.mark.parametrize("K", [1, 4])
def test_head_loss_within_its_rounding_bar_and_gradients_equal_to_autograd(ntm, K, rows, n_fake, mode):
    worst = 0.0
    for j, elems in enumerate(ELEMS):
        outs = head_outputs(100 * K + 10 * rows + j, K, rows, n_fake, elems)
        ref, scale = head_ref64(mode, n_fake, outs)
        for gout in (None, 0.37):
            (loss, grads), (tloss, tgrads) = run_head(ntm, mode, n_fake, outs, gout)
            assert loss.dtype == torch.float32 and loss.dim() == 0
            err, bar = abs(float(loss) - ref), (2 * K + 1) * U * scale
            print(f"K {K} rows {rows} elems {elems} {mode} gout {gout}: loss {float(loss):.8f} ref64 {ref:.8f} err/bar {err / bar:.3f} "
                  f"(torch's own: {abs(float(tloss) - ref) / bar:.3f})")
            assert err <= bar, (elems, err, bar)
            worst = max(worst, err / bar)
            for k, (g, t) in enumerate(zip(grads, tgrads)):
                assert g.shape == t.shape and g.dtype == torch.float32 and torch.equal(g, t), (elems, gout, k, float((g - t).abs().max()))
            if K > 1:
                assert not bool(grads[-1].any()) or mode == "gen"           # the all-inactive output: exact zeros
    print(f"WORST head loss err / bar: {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["crit", "gen"])
def test_head_over_several_chunks_per_half(ntm, mode):
    """131 072 floats per row, three fake rows and one real: 96 chunks of 4096 in the fake half, 32 in the real one."""
    outs = head_outputs(7, 1, 4, 3, 131072)
    ref, scale = head_ref64(mode, 3, outs)
    (loss, grads), (_, tgrads) = run_head(ntm, mode, 3, outs, 0.37)
    err, bar = abs(float(loss) - ref), 3 * U * scale
    print(f"{mode}: loss {float(loss):.8f} ref64 {ref:.8f} err/bar {err / bar:.3f}")
    assert err <= bar and torch.equal(grads[0], tgrads[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["crit", "gen"])
def test_head_equal_calls_equal_bits_and_other_layouts(ntm, mode):
    outs = head_outputs(3, 4, 4, 3, 4097)
    a, b = (run_head(ntm, mode, 3, outs, 0.37)[0] for _ in range(2))
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    # a non-contiguous output and one at an odd offset inside its storage: the same values, so the same bits
    leaves = [torch.from_numpy(o).cuda() for o in outs]
    wide = torch.zeros(4, 2 * leaves[0].shape[1], device="cuda")
    wide[:, ::2] = leaves[0]
    odd = torch.zeros(leaves[2].numel() + 3, device="cuda")
    odd[3:] = leaves[2].reshape(-1)
    other = [wide[:, ::2].requires_grad_(True), leaves[1].requires_grad_(True), odd[3:].view(leaves[2].shape).requires_grad_(True),
             leaves[3].requires_grad_(True)]
    assert not other[0].is_contiguous() and other[2].data_ptr() % 16 != 0
    loss = ntm.training.AdvHeadFn.apply(mode, 3, *other)
    gw, go = torch.autograd.grad(loss, [other[0], other[2]], torch.tensor(0.37, device="cuda"))
    assert torch.equal(loss.detach(), a[0]) and torch.equal(gw, a[1][0]) and torch.equal(go, a[1][2])
    # an output that needs no gradient gets none
    only = ntm.training.AdvHeadFn.apply(mode, 3, leaves[0].clone().requires_grad_(True), leaves[3])
    assert only.requires_grad and torch.equal(only.detach(), ntm.training.AdvHeadFn.apply(mode, 3, leaves[0], leaves[3]))
    with pytest.raises(ntm.NtmError, match="n_fake"):
        ntm.training.AdvHeadFn.apply("crit", 4, *leaves)
    with pytest.raises(RuntimeError, match="first dimension"):
        ntm.training.AdvHeadFn.apply("gen", 0, leaves[0], leaves[1][:2])


# ---- the generator: fakes under no_grad ------------------------------------------------------------------------------------------
def golden():
    return np.load(GOLDEN)


def trajectories(g, knots, T):
    """The maker's knots_to_traj: piecewise linear between knots every `knot` samples, float64 seconds."""
    knot = int(g["meta"][7])
    flat = knots.reshape(-1, knots.shape[-1])
    n, kn = np.arange(T, dtype=np.float64), np.arange(knots.shape[-1], dtype=np.float64) * knot
    return np.stack([np.interp(n, kn, row) for row in flat]).reshape(knots.shape[:-1] + (T,))


def make_generator(ntm):
    m = ntm.DiffDelRNN(hidden_size=64, skip=False).cuda()
    m.load_state_dict({k: torch.as_tensor(v) for k, v in ntm.weights.load_state_dict(W_D).items()})
    return m


def golden_batches(g):
    """(inp_gen, inp_crit, tgt_crit): lists of the reference's (input, target, meta) batches, the trajectories in float64 seconds."""
    T = g["x_gen"].shape[-1]
    traj = trajectories(g, g["traj_knots"], T)
    none = torch.zeros(0)
    mk = lambda x, which: [(torch.from_numpy(x[i]), none, {"delay_trajectory": torch.from_numpy(traj[i, which])}) for i in range(len(x))]   # noqa: E731
    return mk(g["x_gen"], 0), mk(g["x_crit"], 1), [(none, torch.from_numpy(t), {}) for t in g["t_real"]]


@pytest.mark.gpu
def test_fakes_under_no_grad_are_the_bits_of_the_grad_mode_forward(ntm):
    """B = 2: warm-up and two windows, once under no_grad (the inference kernels) and once in grad mode (the training nodes):
    outputs, pre-delay outputs, hidden state and delay buffer are equal bit for bit -- what lets difference 1 cost nothing."""
    g = golden()
    _, crit_batches, _ = golden_batches(g)
    x = crit_batches[0][0].cuda()
    d = (crit_batches[0][2]["delay_trajectory"].unsqueeze(1) * 44100 - 398).cuda()
    runs = []
    for grad in (False, True):
        m = make_generator(ntm)
        for p in m.parameters():
            p.requires_grad_(True)
        with torch.enable_grad() if grad else torch.no_grad():
            m.initialize_hidden(2, 1024)
            m(x[:, :, :1024], d[:, :, :1024], warmup=True)
            outs = [m(x[:, :, 1024 + 1024 * k:2048 + 1024 * k], d[:, :, 1024 + 1024 * k:2048 + 1024 * k]) for k in range(2)]
        assert all(o[0].requires_grad == grad for o in outs)
        runs.append([t.detach() for o in outs for t in o] + [m.hidden.detach(), m.diffdel.buffer.detach()])
    assert float(runs[0][0].abs().max()) > 0.01
    for a, b in zip(*runs):
        assert a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a, b)


# ---- stacked against two-call, the three critic families ------------------------------------------------------------------------
def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn()


def spec_family(ntm):
    crit = spec_tests.make_critic(ntm, spec_tests.SPEC_PARS)
    return (crit, 2048, lambda c: [getattr(v, n) for m in c.models for v in m.convs() for n in NAMES],
            lambda c, dt: (lambda t: (t.parameters(), lambda x: t(x[:, 0])))(spec_tests.CriticTwin(c, dt)))


def dilated_family(ntm):
    torch.manual_seed(12)
    crit = quiet(lambda: ntm.critics.DilatedConvDisc(layers=6, conv_channels=16, test_in_len=1024))

    def twin(c, dt):
        ps = [tuple(getattr(v, n).detach().cpu().to(dt).clone().requires_grad_(True) for n in NAMES) for v in c.convs()]
        return [t for p in ps for t in p], lambda x: [conv_tests.twin_forward(x.to(dt), ps, c.spec(), c.slope)]
    return crit, 1024, lambda c: [getattr(v, n) for v in c.convs() for n in NAMES], twin


def melgan_family(ntm):
    torch.manual_seed(11)
    crit = ntm.critics.MelGCrit(num_D=3, ndf=16, n_layers=4, downsampling_factor=4)
    return (crit, 1024, lambda c: [getattr(v, n) for d in c.model.values() for v in d.convs() for n in NAMES],
            lambda c, dt: (lambda t: (t.parameters(), lambda x: [s[-1] for s in t(x)]))(MelTwin(c, dt)))


FAMILIES = {"MultiSpecCrit": spec_family, "DilatedConvDisc": dilated_family, "MelGCrit": melgan_family}


def twin_step(twin, fake, real, dt):
    """train_crit's loss and the parameter gradients it leaves, by the twin in `dt` -> (loss, [grad float64 numpy])."""
    params, fn = twin
    loss = sum(F.relu(1 + s).mean() for s in fn(fake.to(dt))) + sum(F.relu(1 - s).mean() for s in fn(real.to(dt)))
    loss.backward()
    return float(loss.detach()), [p.grad.double().numpy() for p in params]


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_critic_step_stacked_against_two_call_and_the_float64_twin(ntm, family):
    crit0, window, dev_params, make_twin = FAMILIES[family](ntm)
    clone = lambda: FAMILIES[family](ntm)[0]          # noqa: E731  seeded: the same weights (a weight_norm module has no deepcopy)
    B = 2
    fake, real = (torch.from_numpy(a).unsqueeze(1) for a in spec_tests.model_like_pair(61, B, window))
    (l64, g64), (l32, g32) = (twin_step(make_twin(crit0, dt), fake, real, dt) for dt in (torch.float64, torch.float32))
    kinds = ("dg", "dv", "dbias")
    e32 = {}
    for j, (a64, a32) in enumerate(zip(g64, g32)):
        if np.abs(a64).max() > 0:
            e32[kinds[j % 3]] = max(e32.get(kinds[j % 3], 0.0), float(np.abs(a32 - a64).max() / np.abs(a64).max()))
    print(f"{family}: loss ref64 {l64:.8f} ref32 {l32:.8f}; E32 {e32}")
    gen = make_generator(ntm)
    fake, real = fake.cuda(), real.cuda()
    got = {}
    for stacked in (True, False):
        crit = clone()
        assert all(torch.equal(v, w) for v, w in zip(crit.state_dict().values(), crit0.state_dict().values()))
        crit = crit.cuda()
        with torch.no_grad():
            sep = [ntm.adversarial.critic_heads(crit, crit(x)) for x in (fake, real)]
            both = ntm.adversarial.critic_heads(crit, crit(torch.cat([fake, real])))
        # a stream's output does not depend on its batch: the rows of the stacked pass are the two separate passes' bits
        for o, f, r in zip(both, *sep):
            assert torch.equal(o[:B], f) and torch.equal(o[B:], r)
        opt = torch.optim.SGD(crit.parameters(), lr=0.0)
        tr = ntm.adversarial.Trainer(gen, crit, torch.optim.SGD(gen.parameters(), lr=0.0), opt, window, 44100, 400.25 / 44100,
                                     700.75 / 44100, stacked=stacked)
        loss = tr.critic_step(fake, real)
        K = len(both)
        o64 = [torch.cat([f, r]).double().cpu().numpy() for f, r in zip(*sep)]
        ref, scale = head_ref64("crit", B, o64)
        assert abs(loss - ref) <= (2 * K + 1) * U * scale, (loss, ref)
        got[stacked] = (loss, [p.grad.double().cpu().numpy() for p in dev_params(crit)])
        worst = {}
        for j, (a, a64, a32) in enumerate(zip(got[stacked][1], g64, g32)):
            kind = kinds[j % 3]
            zero = kind == "dbias" and not np.abs(a64).max() > 0            # the last layer's dbias: module docstring
            worst[kind] = max(worst.get(kind, 0.0), check(a, a64, a32, e32[kind], f"{family} stacked={stacked} {kind}[{j // 3}]",
                                                          1.0 if zero else None))
        print(f"WORST {family} stacked={stacked}:", {k: f"{v:.3f}" for k, v in worst.items()}, f"loss {loss:.8f}")
    # the same output bits go into the same head: the two forms' losses are within the head's bar of each other
    assert abs(got[True][0] - got[False][0]) <= (2 * K + 1) * U * scale


# ---- the loop against the reference (golden g28) -----------------------------------------------------------------------------
class RecordingAdam(torch.optim.Adam):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.grads = []

    def step(self, closure=None):
        self.grads.append([None if p.grad is None else p.grad.detach().clone() for g in self.param_groups for p in g["params"]])
        return super().step(closure)


def golden_critic(ntm, g):
    crit = quiet(lambda: ntm.critics.DilatedConvDisc(layers=int(g["crit_layers"]), conv_channels=int(g["crit_channels"]), test_in_len=1024))
    crit.load_state_dict({k[len("crit_init__"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("crit_init__")})
    return crit.cuda()


def golden_trainer(ntm, g, stacked, **kw):
    gen, crit = make_generator(ntm), golden_critic(ntm, g)
    lr = float(g["lr"])
    optG = RecordingAdam(gen.parameters(), lr=lr, betas=(0.5, 0.9))
    optC = RecordingAdam(crit.parameters(), lr=lr, betas=(0.5, 0.9))
    return ntm.adversarial.Trainer(gen, crit, optG, optC, 1024, 44100, float(g["d_min_s"]), float(g["d_max_s"]), stacked=stacked, **kw)


@functools.lru_cache(maxsize=None)
def golden_epoch(ntm, stacked, repeat=0):
    g = golden()
    tr = golden_trainer(ntm, g, stacked)
    assert (tr.train_init, tr.d_traj_offset) == (1024, 398)
    losses = tr.train_epoch(*golden_batches(g))
    return tr, losses


def bar_check(got, ref64, e32, what, scale=None):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    bar = 4.0 * e32 * (float(np.abs(ref64).max()) if scale is None else scale)
    ratio = float(np.abs(got - ref64).max()) / bar
    print(f"{what}: worst err / bar {ratio:.3f}   max err {float(np.abs(got - ref64).max()):.3e}   max|ref64| {float(np.abs(ref64).max()):.3e}")
    assert np.isfinite(got).all() and ratio <= 1.0, (what, ratio)
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("stacked", [False, True])
def test_train_epoch_against_the_reference_s_own_loop(ntm, stacked):
    """Every window's loss and every gradient at every optimizer step of both networks against the reference in double.  The
    critic's recorded gradients are its .grad at each step: the second window of an iteration holds the sum over both windows,
    the first window of the next iteration starts from zero -- a loop that zeroed at another place would miss these bars by
    orders of magnitude."""
    g = golden()
    tr, (crit_losses, gen_losses) = golden_epoch(ntm, stacked)
    e = {k: float(g[f"e32__{k}"]) for k in ("crit_loss", "gen_loss", "crit_grad", "gen_grad")}
    assert len(crit_losses) == len(gen_losses) == 4 == len(tr.optC.grads) == len(tr.optG.grads) == tr.crit_step == tr.gen_step
    assert all(isinstance(v, float) for v in crit_losses + gen_losses)
    worst = {"crit_loss": bar_check(crit_losses, g["ref64__crit_losses"], e["crit_loss"], "critic losses"),
             "gen_loss": bar_check(gen_losses, g["ref64__gen_losses"], e["gen_loss"], "generator losses")}
    for tag, module, opt in (("gen", tr.generator, tr.optG), ("crit", tr.critic, tr.optC)):
        keys = [k for k, _ in module.named_parameters()]
        assert keys == [str(k) for k in g[f"{tag}_keys"]]
        for j, k in enumerate(keys):
            ref = g[f"ref64__{tag}_grad__{k}"]
            for step in range(4):
                zero = not np.abs(ref[step]).max() > 0            # the critic's last bias: module docstring
                r = bar_check(opt.grads[step][j].cpu().numpy(), ref[step], e[f"{tag}_grad"], f"{tag} step {step} d/d {k}", 1.0 if zero else None)
                worst[f"{tag}_grad"] = max(worst.get(f"{tag}_grad", 0.0), r)
    print(f"WORST g28 stacked={stacked}:", {k: f"{v:.3f}" for k, v in worst.items()})
    # final weights, as golden g24's are held: every entry within 2 lr steps, and almost all of them within 1e-5
    lr, steps = float(g["lr"]), 4
    for k, v in tr.generator.state_dict().items():
        d = np.abs(v.double().cpu().numpy() - g[f"ref64__gen_final__{k}"].astype(np.float64))
        assert d.max() <= 2 * lr * steps, (k, d.max())
    dg = np.concatenate([np.abs(v.double().cpu().numpy() - g[f"ref64__gen_final__{k}"].astype(np.float64)).reshape(-1)
                         for k, v in tr.generator.state_dict().items()])
    print(f"generator final weights: {100 * (dg <= 1e-5).mean():.3f} % within 1e-5, max {dg.max():.2e}")
    assert (dg <= 1e-5).mean() >= 0.999
    sd = tr.critic.state_dict()
    dc = np.concatenate([np.abs(v.double().cpu().numpy() - g[f"ref64__crit_final__{k}"].astype(np.float64)).reshape(-1) for k, v in sd.items()])
    d32 = np.concatenate([np.abs(g[f"ref32__crit_final__{k}"].astype(np.float64) - g[f"ref64__crit_final__{k}"].astype(np.float64)).reshape(-1)
                          for k in sd])
    share32 = float((d32 <= 1e-5).mean())
    print(f"critic final weights: {100 * (dc <= 1e-5).mean():.3f} % within 1e-5 (the reference's own float32: {100 * share32:.3f} %), max {dc.max():.2e}")
    assert dc.max() <= 2 * lr * steps and (dc <= 1e-5).mean() >= min(0.999, share32)
    # difference 3: the generator phase left the critic's .grad as the critic phase's last step recorded it
    for p, rec in zip(tr.critic.parameters(), tr.optC.grads[-1]):
        assert torch.equal(p.grad, rec)
    assert all(p.grad is None or not bool(p.grad.any()) for p in tr.generator.parameters())


@pytest.mark.gpu
def test_two_identical_epochs_give_the_same_bits(ntm):
    (a, la), (b, lb) = golden_epoch(ntm, True), golden_epoch(ntm, True, repeat=1)
    assert a is not b and la == lb
    for m, n in ((a.generator, b.generator), (a.critic, b.critic)):
        for (k, v), w in zip(m.state_dict().items(), n.state_dict().values()):
            assert torch.equal(v, w), k
    first = make_generator(ntm).state_dict()
    assert not all(torch.equal(v, first[k]) for k, v in a.generator.state_dict().items())          # and they did move


def validation_batch(g):
    T = g["val_x"].shape[-1]
    return (torch.from_numpy(g["val_x"]), torch.from_numpy(g["val_t"]), {"delay_trajectory": torch.from_numpy(trajectories(g, g["val_knots"], T))})


@functools.lru_cache(maxsize=None)
def validation_run(ntm):
    g = golden()
    seen = []

    class Evaluator:
        def add_loss(self, output, target):
            seen.append((output, target))

    tr = golden_trainer(ntm, g, True)
    pred, pre_d = tr.validate([validation_batch(g)], Evaluator(), float(g["d_max_s"]))
    return tr, pred, pre_d, seen


@pytest.mark.gpu
def test_validate_prediction_against_the_reference(ntm):
    """(pred, pre_d) of golden g28's validation batch within the bar of the golden's own pair, 4 E32(val) max|ref64|.

    The reference's validation set is VADataset(double=True), so its delay line forms the interpolation weights from float64
    delays.  Trainer.validate hands a float64 trajectory on in float64 (DiffDelRNN.forward_f64_delays, ntm_delay_forward_f64): a
    float32 delay of 400 to 700 samples is 3e-5 to 6e-5 samples wide, and on this white-noise batch, where neighbouring samples
    differ by 0.3, that rounding alone moves the output by 9.3e-6 -- 1.9 times this bar, which is what the float32 path measures
    and what the last assert below holds it to from the other side."""
    g = golden()
    _, pred, pre_d, _ = validation_run(ntm)
    e = float(g["e32__val"])
    bar_check(pre_d.cpu().numpy(), g["ref64__val_pre_d"], e, "validation pre_d")
    bar_check(pred.cpu().numpy(), g["ref64__val_pred"], e, "validation pred")
    # the same batch with a float32 trajectory takes forward(): pre_d is the same bits, the delayed output is not
    x, t, meta = validation_batch(g)
    tr32 = golden_trainer(ntm, g, True)
    pred32, pre32 = tr32.validate([(x, t, {"delay_trajectory": meta["delay_trajectory"].float()})], type("E", (), {"add_loss": lambda *a: None})(),
                                  float(g["d_max_s"]))
    assert torch.equal(pre32, pre_d) and not torch.equal(pred32, pred) and float((pred32 - pred).abs().max()) < 1e-4


@pytest.mark.gpu
def test_validate_protocol_and_checkpoints(ntm, tmp_path):
    g = golden()
    batch = validation_batch(g)
    T = batch[0].shape[-1]
    tr, pred, pre_d, seen = validation_run(ntm)
    assert pred.shape == pre_d.shape == (2, 1, T) and tr.generator.diffdel.buffer.shape[-1] == int(float(g["d_max_s"]) * 44100 + 1) + 1
    (o, t), = seen
    assert o.shape == t.shape == (2, T) and o.dtype == t.dtype == torch.float32 and torch.equal(o, pred[:, 0]) and torch.equal(t.cpu(), batch[1][:, 0])
    # the bookkeeping of an epoch: running{epoch}.pth before the pass, {key}best.pt for every key whose best epoch this is
    logs = []
    ev = ntm.evaluation.val_loss_supervised(device="cuda")
    dry = golden_trainer(ntm, g, True, model_path=str(tmp_path / "dry"), dry_run=True, log=lambda values, step=None: logs.append(values))
    dry.validate([batch], ev, float(g["d_max_s"]), epoch=0)
    assert not (tmp_path / "dry").exists() and ev.iter_count == 0 and all(b[0] == 0 and b[1] < 1e9 for b in ev.bst_losses.values())
    assert [k for v in logs for k in v if k != "epoch"] == [p + "loss/" + k for k in ev.bst_losses for p in ("", "best_")]
    wet = golden_trainer(ntm, g, True, model_path=str(tmp_path / "wet"))
    wet.validate([batch], ev, float(g["d_max_s"]), epoch=0)
    assert sorted(os.listdir(tmp_path / "wet")) == sorted(["running0.pth"] + [k + "best.pt" for k in ev.bst_losses])
    sd = torch.load(tmp_path / "wet" / "ESRbest.pt")
    assert all(torch.equal(v.cpu(), sd[k].cpu()) for k, v in wet.generator.state_dict().items())
    # an epoch that is nowhere the best writes its running checkpoint alone
    ev.bst_losses = {k: [0, 0.0] for k in ev.bst_losses}
    wet.validate([batch], ev, float(g["d_max_s"]), epoch=1)
    assert sorted(os.listdir(tmp_path / "wet")) == sorted(["running0.pth", "running1.pth"] + [k + "best.pt" for k in ev.bst_losses])


# ---- the delay line with float64 delays ------------------------------------------------------------------------------------------
def delay_f64_formula(pre, buf, d):
    """y[n] = w_b z[n - k - 1] + w_a z[n - k] with k = floor(d), w = 1 - |m - d| in float64, the m = k + 1 term first, rounded to
    float32 once; z = [buffer, pre].  Every operation is one IEEE double operation, so the kernel can be held to the bits."""
    B, T = pre.shape
    D = buf.shape[1]
    z = torch.cat([buf, pre], dim=1).double()
    k = torch.floor(d)
    at = D + torch.arange(T, device=pre.device)[None, :] - k.long()
    wb, wa = 1.0 - ((k + 1.0) - d).abs(), 1.0 - (k - d).abs()
    zb = torch.where(k + 1.0 <= D, z.gather(1, (at - 1).clamp(min=0)), torch.zeros_like(d))
    acc = torch.where(wb > 0, wb * zb, torch.zeros_like(d))
    return (acc + wa * z.gather(1, at)).float()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 255, 257, 1000])
def test_delay_line_with_float64_delays_against_its_formula(ntm, T):
    """ntm_delay_forward_f64 through DiffDelRNN.forward_f64_delays, B = 3, D = 38: history taps, whole delays (a weight of exactly
    0), d = 0 and d = D, delays that float32 cannot hold -- equal to the float64 formula bit for bit; pre_d and the hidden state
    are forward()'s bits; the carried buffer is the last D samples; a split call equals the whole one; d > D raises as forward()
    does and leaves the buffer as it was."""
    B, D = 3, 38
    rng = np.random.default_rng(T)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 1, T)).astype(np.float32)).cuda()
    d = rng.uniform(0.0, D, (B, 1, T))
    d[0, 0, ::7] = np.round(d[0, 0, ::7])
    d[1, 0, 0], d[2, 0, -1] = 0.0, float(D)
    d[1, 0, T // 2] = 17.0 + 2.0 ** -40
    d = torch.from_numpy(d).cuda()
    runs = []
    for f64 in (True, False):
        m = make_generator(ntm)
        m.initialize_hidden(B, D - 1)
        assert m.diffdel.buffer.shape[-1] == D
        m.diffdel.buffer = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 1, D)).astype(np.float32)).cuda() if f64 else runs[0][3].clone()
        buf0 = m.diffdel.buffer.clone()
        y, pre = m.forward_f64_delays(x, d) if f64 else m(x, d.float())
        runs.append((y, pre, m.hidden.clone(), buf0, m.diffdel.buffer.clone()))
    (y, pre, h, buf0, buf1), (y32, pre32, h32, _, buf32) = runs
    assert torch.equal(pre, pre32) and torch.equal(h, h32) and torch.equal(buf1, buf32) and y.dtype == torch.float32
    assert torch.equal(y[:, 0], delay_f64_formula(pre[:, 0], buf0[:, 0], d[:, 0]))
    assert torch.equal(buf1[:, 0], torch.cat([buf0[:, 0], pre[:, 0]], dim=1)[:, -D:])
    assert float((y - y32).abs().max()) < 1e-5
    if T > 1:
        m = make_generator(ntm)
        m.initialize_hidden(B, D - 1)
        m.diffdel.buffer = buf0.clone()
        cut = T // 3 + 1
        parts = [m.forward_f64_delays(x[:, :, :cut], d[:, :, :cut])[0], m.forward_f64_delays(x[:, :, cut:], d[:, :, cut:])[0]]
        assert torch.equal(torch.cat(parts, dim=2), y) and torch.equal(m.diffdel.buffer, buf1)
        bad = d.clone()
        bad[2, 0, 1] = D + 1e-9
        kept = m.diffdel.buffer.clone()
        with pytest.raises(AssertionError):
            m.forward_f64_delays(x, bad)
        assert torch.equal(m.diffdel.buffer, kept)
    with pytest.raises(RuntimeError, match="float64"):
        make_generator(ntm).forward_f64_delays(x, d.float())


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_trajectory_outside_the_warm_up_is_refused_with_the_weights_untouched(ntm):
    g = golden()
    tr = golden_trainer(ntm, g, True)
    before = [p.detach().clone() for m in (tr.generator, tr.critic) for p in m.parameters()]
    inp_gen, inp_crit, tgt = golden_batches(g)
    for bad in ((1024 + 398 + 0.5) / 44100, 397.0 / 44100):          # a delay above train_init, a delay below zero samples
        crit_bad = [(x, t, {"delay_trajectory": m["delay_trajectory"].clone()}) for x, t, m in inp_crit]
        crit_bad[0][2]["delay_trajectory"][1, 2000] = bad
        with pytest.raises(AssertionError):
            tr.train_epoch(inp_gen, crit_bad, tgt)
    assert tr.crit_step == tr.gen_step == 0 and not tr.optC.grads and not tr.optG.grads
    for p, q in zip((p for m in (tr.generator, tr.critic) for p in m.parameters()), before):
        assert torch.equal(p, q)
    # a segment with no whole window: empty loss lists, no optimizer step
    short = lambda bs: [tuple(a[..., :2047] if torch.is_tensor(a) and a.numel() else a for a in b[:2])      # noqa: E731
                        + ({k: v[..., :2047] for k, v in b[2].items()},) for b in bs]
    assert tr.train_epoch(short(inp_gen), short(inp_crit), short(tgt)) == ([], [])
    assert not tr.optC.grads and not tr.optG.grads
    for p, q in zip((p for m in (tr.generator, tr.critic) for p in m.parameters()), before):
        assert torch.equal(p, q)


# ---- a spectral run against a float64 twin of the whole chain -------------------------------------------------------------------
class GeneratorTwin:
    """DiffDelRNN(1, 64, 1, skip=False) in `dtype` on the CPU: torch.nn.GRU, the bias-free head, and the delay line in closed
    form -- y[n] = (1 - f) z[D + n - k] + f z[D + n - k - 1] with z = [buffer, pre], k = floor(d[n]), f = d[n] - k."""

    def __init__(self, sd, dtype):
        self.gru = torch.nn.GRU(1, 64, batch_first=True).to(dtype)
        self.gru.load_state_dict({k[len("GRU."):]: v.to(dtype) for k, v in sd.items() if k.startswith("GRU.")})
        self.w_o = sd["output.weight"].to(dtype).clone().requires_grad_(True)
        self.dtype = dtype

    def parameters(self):
        return list(self.gru.parameters()) + [self.w_o]

    def initialize_hidden(self, B, D):
        self.hidden, self.buffer = None, torch.zeros(B, int(D) + 1, dtype=self.dtype)

    def __call__(self, x, d, warmup=False):
        h, self.hidden = self.gru(x.to(self.dtype).transpose(1, 2), self.hidden)
        pre = (h @ self.w_o.t())[:, :, 0]
        D, T = self.buffer.shape[1], pre.shape[1]
        z = torch.cat([self.buffer, pre], dim=1)
        self.buffer = z[:, -D:]
        if warmup:
            return pre.unsqueeze(1)
        d = d[:, 0].to(self.dtype)
        k = torch.floor(d)
        f = d - k
        at = D + torch.arange(T)[None, :] - k.long()
        return ((1 - f) * z.gather(1, at) + f * z.gather(1, at - 1)).unsqueeze(1)


def spectral_batches(g, it=0):
    """Golden g28's batches of iteration `it` with the trajectories in float32 seconds, as SegmentFeeder hands them over: the
    reference then forms the delays in float32 (`traj * fs - offset` on a float32 tensor), and they are the engine's delays bit for bit."""
    return [[(x, t, {k: v.float() for k, v in m.items()})] for (x, t, m) in (b[it] for b in golden_batches(g))]


def spectral_chain(sd, crit, g, dt, it=0):
    """One iteration of the loop by the twins in `dt` -> (critic loss, generator loss, generator gradients, the scales of the two
    losses: the sum of the means of |term|, which for the generator's loss, small by cancellation, is not the loss itself)."""
    (b_gen,), (b_crit,), (b_tgt,) = spectral_batches(g, it)
    d = lambda b: b[2]["delay_trajectory"].unsqueeze(1) * 44100 - 398       # noqa: E731  float32, as Trainer forms them
    G, C = GeneratorTwin(sd, dt), spec_tests.CriticTwin(crit, dt)
    x, dd = b_crit[0], d(b_crit)
    with torch.no_grad():
        G.initialize_hidden(2, 1024)
        G(x[:, :, :1024], dd[:, :, :1024], warmup=True)
        fake = G(x[:, :, 1024:], dd[:, :, 1024:])
    real = b_tgt[1][:, :, 1024:].to(dt)
    loss_c = sum(F.relu(1 + s).mean() for s in C(fake[:, 0])) + sum(F.relu(1 - s).mean() for s in C(real[:, 0]))
    x, dd = b_gen[0], d(b_gen)
    G.initialize_hidden(2, 1024)
    G(x[:, :, :1024], dd[:, :, :1024], warmup=True)
    outs = C(G(x[:, :, 1024:], dd[:, :, 1024:])[:, 0])
    loss_g = sum(-s.mean() for s in outs)
    loss_g.backward()
    scales = (float(loss_c.detach()), float(sum(s.detach().abs().mean() for s in outs)))
    return float(loss_c.detach()), float(loss_g.detach()), [p.grad.double().numpy() for p in G.parameters()], scales


@pytest.mark.gpu
def test_one_spectral_iteration_against_a_float64_twin_of_the_whole_chain(ntm):
    """MultiSpecCrit (the parameters of tests/test_gpu_critic.py), one window of 2048 behind the warm-up of 1024 on golden g28's
    first batches, optimizers with a zero step: the critic's loss, the generator's loss and the generator's five gradients
    against the chain GRU -> head -> delay line -> torch.stft -> conv stacks in float64; E32 from the chain's own float32 run.

    The trajectories are float32 here (spectral_batches), so the twin and the engine read the same delays.  This chain is
    ill-conditioned: the log-spectrogram critic at its initial weights (d log10 P / dP = 1 / (P ln 10) at the spectral nulls of a
    noise-driven signal) turns a relative 1e-7 on the generator's weights into 3e-4 on these gradients (measured with the float64
    twin), and torch's own float32 run of the chain stands 4e-2 of the largest element off the float64 one.  That E32 is the
    references' own and makes the gradients' bar a coarse one (0.17 of the largest element: it tells a wrong sign or a missing
    term, not a rounding; the device itself lands 3e-4 of the largest element from the float64 twin, 0.002 of that bar, and its
    losses at 0.001 and 0.09 of theirs).  The fine figures are piece by piece, measured on an MI355X with this case's inputs: dL/dy at the
    device's own y against the float64 twin 6e-7 of its largest element, the generator's five gradients from a fixed dL/dy 1e-6 to
    7e-6, and Trainer's step equal bit for bit to generator -> the module's own train_gen."""
    g = golden()
    sd = {k: torch.as_tensor(v) for k, v in ntm.weights.load_state_dict(W_D).items()}
    crit = spec_tests.make_critic(ntm, spec_tests.SPEC_PARS)
    (c64, g64, p64, (sc, sg)), (c32, g32, p32, _) = (spectral_chain(sd, crit, g, dt) for dt in (torch.float64, torch.float32))
    e_grad = max(float(np.abs(a32 - a64).max() / np.abs(a64).max()) for a64, a32 in zip(p64, p32))
    # the losses' E32 over both iterations of the golden's batches (four numbers), each against the scale of its terms
    (c64b, g64b, _, (scb, sgb)), (c32b, g32b, _, _) = (spectral_chain(sd, crit, g, dt, 1) for dt in (torch.float64, torch.float32))
    e_loss = max(abs(c32 - c64) / sc, abs(g32 - g64) / sg, abs(c32b - c64b) / scb, abs(g32b - g64b) / sgb)
    print(f"critic loss ref64 {c64:.8f} ref32 {c32:.8f}; generator loss ref64 {g64:.8f} ref32 {g32:.8f}; E32 of the losses {e_loss:.2e}, "
          f"of the gradients {e_grad:.2e}")
    assert 0 < 4 * e_loss < 0.05 and 4 * e_grad < 0.5          # a zero tensor is still twice the bar away
    gen = make_generator(ntm)
    optG = RecordingAdam(gen.parameters(), lr=0.0)
    tr = ntm.adversarial.Trainer(gen, crit.cuda(), optG, torch.optim.SGD(crit.parameters(), lr=0.0), 2048, 44100, float(g["d_min_s"]),
                                 float(g["d_max_s"]))
    crit_losses, gen_losses = tr.train_epoch(*spectral_batches(g))
    assert len(crit_losses) == len(gen_losses) == 1 == len(optG.grads)
    bar_check(crit_losses, [c64], e_loss, "critic loss", sc)
    bar_check(gen_losses, [g64], e_loss, "generator loss", sg)
    order = ["GRU.weight_ih_l0", "GRU.weight_hh_l0", "GRU.bias_ih_l0", "GRU.bias_hh_l0", "output.weight"]
    assert [k for k, _ in gen.named_parameters()] == order
    for k, got, a64 in zip(order, optG.grads[0], p64):
        bar_check(got.cpu().numpy(), a64, e_grad, f"d/d {k}")
