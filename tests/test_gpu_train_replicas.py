"""GPU: R replicas trained in one launch per window (ntm_amd.Replicas, training.GRUTrainStep with R, the *_replicas kernels of
csrc/gru_train.hip).  The oracle throughout is the single-model path in the same process -- GRUTrainStep, ESRLoss / DCPreESR and
the models' own train_epoch on the replica's slice with the replica's weights -- compared bit for bit (torch.equal): that path is
pinned to float64 autograd and to the reference by tests/test_gpu_train.py and tests/test_gpu_train_diffdel.py (goldens g23, g24),
and replica 0 of the epoch tests is held to g23's bars directly as well.
For the gradient reduction and the loss adjoints there is one kernel each: the single-model entry points launch it with one grid
row, so "single versus replica" compares R = 1 against R > 1 of the same code there.  Their independent anchors are the fp64
tests of the raw entry points in tests/test_gpu_train.py and the goldens g23 / g24."""
import numpy as np
import pytest
import torch

from helpers import load

W_G = "GRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE]_BEST"
W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"
KEYS = ["GRU.weight_ih_l0", "GRU.weight_hh_l0", "GRU.bias_ih_l0", "GRU.bias_hh_l0", "output.weight", "output.bias"]
SCALES = (0.1, 1.0, 3.0)


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def _random_sd(seed, scale, bias=True):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / 8.0
    shapes = {"GRU.weight_ih_l0": (192, 1), "GRU.weight_hh_l0": (192, 64), "GRU.bias_ih_l0": (192,), "GRU.bias_hh_l0": (192,),
              "output.weight": (1, 64), "output.bias": (1,)}
    sd = {n: ((torch.rand(*s, generator=g) * 2 - 1) * k * scale).float() for n, s in shapes.items()}
    return sd if bias else {n: v for n, v in sd.items() if n != "output.bias"}


def _model(ntm, sd, grad=True):
    m = ntm.RNN(1, 64, 1).cuda()
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    for p in m.parameters():
        p.requires_grad_(grad)
    return m


def _sds(ntm, R):
    """Replica r carries _random_sd(seed=r, scale cycling over 0.1, 1, 3); the middle one carries the shipped checkpoint, so a wrong
    replica index (s % R, an off-by-one at a boundary) cannot pass."""
    return [ntm.weights.load_state_dict(W_G) if r == R // 2 else _random_sd(r, SCALES[r % 3]) for r in range(R)]


GRID = [(1, 7), (2, 1), (3, 5), (8, 32), (9, 32)]       # (9, 32): 288 streams, more workgroups than CUs


def _inputs(R, Bper, T):
    g = torch.Generator().manual_seed(R * 7919 + Bper * 31 + T)
    B = R * Bper
    x = (torch.rand(B, 1, T, generator=g) - 0.5).cuda()
    h0 = (0.5 * (torch.rand(1, B, 64, generator=g) - 0.5)).cuda()
    dy = torch.randn(B, T, generator=g).cuda()
    dh = torch.randn(1, B, 64, generator=g).cuda()
    return x, h0, dy, dh


@pytest.mark.gpu
@pytest.mark.parametrize("R,Bper", GRID)
@pytest.mark.parametrize("T", [1, 5, 33, 300])          # either side of the 32-step save stage and of the 128 / 256 x-tile points
def test_forward_is_bit_identical_to_every_replica_alone(ntm, R, Bper, T):
    sds = _sds(ntm, R)
    x, h0, _, _ = _inputs(R, Bper, T)
    reps = ntm.Replicas([_model(ntm, sd) for sd in sds])
    reps.hidden = h0.clone()
    y = reps(x)
    assert y.requires_grad and reps.hidden.requires_grad and y.shape == x.shape
    for r, sd in enumerate(sds):
        sl = slice(r * Bper, (r + 1) * Bper)
        m = _model(ntm, sd)
        m.hidden = h0[:, sl].clone()
        ya = m(x[sl])
        assert torch.equal(y[sl].detach(), ya.detach()), r
        assert torch.equal(reps.hidden[:, sl].detach(), m.hidden.detach()), r
        assert torch.equal(reps.models[r].hidden.detach(), m.hidden.detach()), r      # each model sees its slice of the state


GRAD_CASES = [(R, Bper, T, True, True) for R, Bper in GRID for T in (5, 300)] + [(3, 5, 300, False, True), (3, 5, 300, True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("R,Bper,T,with_dy,with_dh", GRAD_CASES)
def test_gradients_are_bit_identical_to_every_replica_alone(ntm, R, Bper, T, with_dy, with_dh):
    """All six parameter gradients and dh0.  Accuracy against float64 is established for the single path
    (test_bptt_gradients_against_float64_autograd) and inherited through equality."""
    sds = _sds(ntm, R)
    x, h0, dy, dh = _inputs(R, Bper, T)

    def grads(run, params, h0_, dy_, dh_):
        h = h0_.clone().requires_grad_(True)
        y, hT = run(h)
        outs = ([hT] if with_dh else []) + ([y[:, 0, :]] if with_dy else [])
        gs = ([dh_] if with_dh else []) + ([dy_] if with_dy else [])
        return torch.autograd.grad(outs, params + [h], gs, allow_unused=True)

    reps = ntm.Replicas([_model(ntm, sd) for sd in sds])

    def run_group(h):
        reps.hidden = h
        y = reps(x)
        return y, reps.hidden
    got = grads(run_group, [p for m in reps.models for p in m.parameters()], h0, dy, dh)
    for r, sd in enumerate(sds):
        sl = slice(r * Bper, (r + 1) * Bper)
        m = _model(ntm, sd)

        def run_alone(h):
            m.hidden = h
            y = m(x[sl])
            return y, m.hidden
        want = grads(run_alone, list(m.parameters()), h0[:, sl], dy[sl], dh[:, sl])
        for key, a, b in zip(KEYS, got[6 * r:6 * r + 6], want[:6]):
            if b is None:                    # dy None: the head's bias is not reached -- in neither path
                assert key == "output.bias" and not with_dy and (a is None or not a.any())
                continue
            assert a is not None and torch.equal(a, b), (r, key)
        assert torch.equal(got[-1][:, sl], want[-1]), r


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["esr", "dcpre", "dcpre_off"])
def test_grouped_losses_are_the_single_losses_value_and_adjoint(ntm, kind):
    R, Bper, T = 3, 5, 300
    g = torch.Generator().manual_seed(11)
    y = torch.rand(R * Bper, 1, T, generator=g) - 0.5
    energy = torch.tensor([0.05, 1.0, 7.0]).repeat_interleave(Bper).view(-1, 1, 1)      # swapped sums would show
    t = (energy * (0.8 * y + 0.1 * torch.randn(R * Bper, 1, T, generator=g) + 0.05)).float()
    w = torch.tensor([3.0, 0.5, -2.0]).cuda()
    fn = ntm.ESRLoss() if kind == "esr" else ntm.DCPreESR(dc_pre=(kind == "dcpre"))
    yc, tc = y.cuda().requires_grad_(True), t.cuda()
    v = fn.replicas(yc, tc, R)
    v0 = fn.replicas(y.cuda(), tc, R)
    assert v.shape == (R,) and v.requires_grad and not v0.requires_grad and torch.equal(v.detach(), v0)
    (v * w).sum().backward()
    for r in range(R):
        sl = slice(r * Bper, (r + 1) * Bper)
        ya = y[sl].cuda().requires_grad_(True)
        va = fn(ya, tc[sl])
        (va * w[r]).backward()
        assert torch.equal(v[r].detach(), va.detach()), (r, float(v[r]), float(va))
        assert torch.equal(yc.grad[sl], ya.grad), r
    assert len({float(a) for a in v.detach()}) == R
    # R = 1: the grouped loss of one replica is the plain loss (the two share their kernels: an offset bug would show here)
    y1 = y[Bper:].cuda().requires_grad_(True)           # 2 * Bper streams as ONE replica
    y2 = y[Bper:].cuda().requires_grad_(True)
    v1, v2 = fn.replicas(y1, tc[Bper:], 1), fn(y2, tc[Bper:])
    (v1 * w[:1]).sum().backward()
    (v2 * w[0]).backward()
    assert v1.shape == (1,) and torch.equal(v1[0].detach(), v2.detach()) and torch.equal(y1.grad, y2.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("Bper", [1, 4, 5, 32, 100, 256, 300])
@pytest.mark.parametrize("splits", [1, 3, 9])
def test_the_loss_sums_are_added_in_the_order_of_the_single_losses(ntm, Bper, splits):
    """ntm_loss_sums_replicas against the two torch sums of the single-model path (esr_sums: partial rows, ESRLoss: streams) on
    rows of widely different magnitude, where any other order of adding shows in the last bits."""
    R = 3
    g = torch.Generator().manual_seed(Bper * 10 + splits)
    rows = (torch.randn(R * Bper, splits, 2, generator=g, dtype=torch.float64)
            * torch.exp(3 * torch.randn(R * Bper, splits, 2, generator=g, dtype=torch.float64))).abs().cuda()
    got = ntm.model._replica_sums(rows, R, Bper, splits)
    for r in range(R):
        part = rows[r * Bper:(r + 1) * Bper].clone()
        per_stream = part[:, 0] if splits == 1 else part.sum(dim=1)
        assert torch.equal(got[r], per_stream.sum(dim=0)), r


class RecordingAdam(torch.optim.Adam):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.grads = []

    def step(self, closure=None):
        self.grads.append([p.grad.detach().double().cpu().clone() for g in self.param_groups for p in g["params"]])
        return super().step(closure)


def _g23_setup(ntm, loss_name, third=None):
    """Replica 0: the checkpoint, the g23 loader, g23's lr.  Replicas 1 and 2: random inits, the two batches in swapped order,
    Adam at 3e-4 / 1e-3.  -> (state dicts, loaders, learning rates, loss function)."""
    inp = load("g23_train_inputs.npz")
    loader = [(torch.from_numpy(x), torch.from_numpy(t), None) for x, t in zip(inp["x"], inp["t"])]
    sds = [ntm.weights.load_state_dict(W_G), _random_sd(1, 1.0), _random_sd(2, 3.0) if third is None else third]
    fn = ntm.ESRLoss() if loss_name == "esr" else ntm.DCPreESR(dc_pre=True)
    return sds, [loader, loader[::-1], loader[::-1]], [float(inp["lr"]), 3e-4, 1e-3], fn


_CACHE = {}


def _alone(ntm, loss_name):
    """Every replica trained by its own RNN.train_epoch: [(model, window losses, epoch loss)]; computed once, never modified."""
    if ("alone", loss_name) not in _CACHE:
        sds, loaders, lrs, fn = _g23_setup(ntm, loss_name)
        out = []
        for sd, loader, lr in zip(sds, loaders, lrs):
            m = _model(ntm, sd, grad=False)
            losses = []

            def loss_fcn(p, t):
                v = fn(p, t)
                losses.append(float(v.detach()))
                return v
            epoch = m.train_epoch(loader, loss_fcn, torch.optim.Adam(m.parameters(), lr=lr))
            out.append((m, losses, epoch))
        _CACHE["alone", loss_name] = out
    return _CACHE["alone", loss_name]


def _group(ntm, loss_name, lrs=None, one_optimizer=False, third=None):
    sds, loaders, lrs0, fn = _g23_setup(ntm, loss_name, third)
    lrs = lrs0 if lrs is None else lrs
    models = [_model(ntm, sd, grad=False) for sd in sds]
    if one_optimizer:
        opts = RecordingAdam([p for m in models for p in m.parameters()], lr=lrs[0])
    else:
        opts = [RecordingAdam(m.parameters(), lr=lr) for m, lr in zip(models, lrs)]
    windows = []
    epochs = ntm.Replicas(models).train_epoch(loaders, fn, opts, losses_hook=windows.append)
    return models, opts, windows, epochs


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name", ["esr", "dcpreesr"])
def test_train_epoch_gives_every_replica_the_bits_of_its_own_train_epoch_and_meets_g23(ntm, loss_name):
    models, opts, windows, epochs = _group(ntm, loss_name)
    assert len(windows) == 6 and all(len(w) == 3 for w in windows) and len(epochs) == 3
    for r, (m, (ma, losses, epoch)) in enumerate(zip(models, _alone(ntm, loss_name))):
        for (name, a), b in zip(m.named_parameters(), ma.parameters()):
            assert torch.equal(a, b), (r, name)
        assert [w[r] for w in windows] == losses and epochs[r] == epoch, r
        assert torch.equal(m.hidden, ma.hidden), r
    # replica 0 against the reference's own epoch, with the bars of test_train_epoch_against_the_reference_g23
    ref = load(f"g23_train_{loss_name}.npz")
    assert len(opts[0].grads) == len(ref["losses"]) == 6
    for w, gw in enumerate(opts[0].grads):
        for key, a in zip(KEYS, gw):
            r = ref[f"grad__{key}"][w].astype(np.float64)
            err = float(np.abs(a.numpy().reshape(r.shape) - r).max())
            assert err <= 1e-4 * float(np.abs(r).max()), (w, key, err, float(np.abs(r).max()))
    np.testing.assert_allclose([w[0] for w in windows], ref["losses"], rtol=1e-5, atol=0)
    assert abs(epochs[0] / float(ref["epoch_loss"]) - 1) < 1e-5
    steps, lr = len(ref["losses"]), float(load("g23_train_inputs.npz")["lr"])
    sd = models[0].state_dict()
    for key in KEYS:
        a, r = sd[key].detach().cpu().numpy(), ref[f"final__{key}"]
        d = np.abs(a - r)
        assert float(d.max()) <= 2 * lr * steps, (key, float(d.max()))
        assert float((d <= 1e-5).mean()) >= 0.999, (key, float((d <= 1e-5).mean()))


@pytest.mark.gpu
def test_one_optimizer_over_all_replicas_equals_one_optimizer_each(ntm):
    lrs = [1e-3] * 3
    each, _, w_each, e_each = _group(ntm, "esr", lrs)
    one, opt, w_one, e_one = _group(ntm, "esr", lrs, one_optimizer=True)
    assert sum(len(g["params"]) for g in opt.param_groups) == 18
    assert w_each == w_one and e_each == e_one
    for ma, mb in zip(each, one):
        for a, b in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_epochs_are_deterministic_and_replicas_do_not_leak_into_each_other(ntm):
    a, _, wa, ea = _group(ntm, "dcpreesr")
    b, _, wb, eb = _group(ntm, "dcpreesr")
    assert wa == wb and ea == eb
    for ma, mb in zip(a, b):
        for p, q in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(p, q)
    c, _, wc, ec = _group(ntm, "dcpreesr", third=_random_sd(77, 1.0))       # only replica 2's weights change
    for r in (0, 1):
        assert [w[r] for w in wc] == [w[r] for w in wa] and ec[r] == ea[r]
        for p, q in zip(a[r].parameters(), c[r].parameters()):
            assert torch.equal(p, q)
    assert [w[2] for w in wc] != [w[2] for w in wa]


class _Loader(list):
    """The reference's DataLoader as train_epoch sees it: (x, t, meta) batches and .dataset.fs / .dataset.delay_analyzer."""

    def __init__(self, batches, fs, max_delay_s):
        super().__init__(batches)
        self.dataset = type("DS", (), {"fs": fs, "delay_analyzer": type("DA", (), {"max_delay": max_delay_s})})


def _dd_model(ntm, sd, max_delay, grad=False):
    m = ntm.DiffDelRNN(1, 64, 1, max_delay=max_delay).cuda()
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    for p in m.parameters():
        p.requires_grad_(grad)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name", ["esr", "dcpreesr"])
def test_diffdel_train_epoch_gives_every_replica_the_bits_of_its_own_train_epoch(ntm, loss_name):
    inp = load("g24_train_diffdel_inputs.npz")
    fs, D = int(inp["meta"][7]), int(inp["meta"][6])

    def loader():
        return _Loader([(torch.from_numpy(x), torch.from_numpy(t), {"delay_trajectory": torch.from_numpy(tr)})
                        for x, t, tr in zip(inp["x"], inp["t"], inp["traj_s"])], fs, float(inp["analyser_max_delay_s"]))
    sds = [ntm.weights.load_state_dict(W_D), _random_sd(5, 1.0, bias=False)]
    lrs = [float(inp["lr"]), 3e-4]
    fn = ntm.ESRLoss() if loss_name == "esr" else ntm.DCPreESR(dc_pre=True)
    alone = []
    for sd, lr in zip(sds, lrs):
        m = _dd_model(ntm, sd, D)
        alone.append((m, m.train_epoch(loader(), fn, torch.optim.Adam(m.parameters(), lr=lr))))
    models = [_dd_model(ntm, sd, D) for sd in sds]
    epochs = ntm.Replicas(models).train_epoch([loader(), loader()], fn,
                                              [torch.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(models, lrs)])
    for r, (m, (ma, epoch)) in enumerate(zip(models, alone)):
        for (name, a), b in zip(m.named_parameters(), ma.parameters()):
            assert torch.equal(a, b), (r, name)
        assert epochs[r] == epoch, r
        assert torch.equal(m.hidden, ma.hidden) and torch.equal(m.diffdel.buffer, ma.diffdel.buffer), r


@pytest.mark.gpu
def test_a_delay_above_the_buffer_in_one_replica_raises_and_leaves_every_replica(ntm):
    Bper, D = 2, 300
    models = [_dd_model(ntm, sd, D - 1, grad=True) for sd in (ntm.weights.load_state_dict(W_D), _random_sd(5, 1.0, bias=False))]
    reps = ntm.Replicas(models)
    reps.initialize_hidden(Bper)
    x = (torch.rand(2 * Bper, 1, 512) - 0.5).cuda()
    d = torch.full((2 * Bper, 1, 512), 100.0, device="cuda")
    reps(x, d, warmup=True)
    bufs = [m.diffdel.buffer.detach().clone() for m in models]
    params = [p.detach().clone() for m in models for p in m.parameters()]
    bad = d.clone()
    bad[3, 0, 77] = D + 0.5                  # replica 1
    with pytest.raises(AssertionError):
        reps(x, bad)
    assert all(torch.equal(m.diffdel.buffer.detach(), b) for m, b in zip(models, bufs))
    assert all(torch.equal(p, q) for p, q in zip([p for m in models for p in m.parameters()], params))
    y, _ = reps(x, d)                        # the flag is cleared: the next good window runs
    assert y.requires_grad


@pytest.mark.gpu
def test_replica_refusals_on_the_device(ntm):
    sd = ntm.weights.load_state_dict(W_G)
    a, b = _model(ntm, sd), _model(ntm, _random_sd(1, 1.0))
    with pytest.raises(ValueError, match="same module appears twice"):
        ntm.Replicas([a, b, a])
    with pytest.raises(RuntimeError, match="hidden_size=64"):
        ntm.Replicas([a, ntm.RNN(1, 32, 1).cuda()])
    with pytest.raises(TypeError):
        ntm.Replicas([a, ntm.DiffDelRNN(1, 64, 1).cuda()])
    reps = ntm.Replicas([a, b])
    before = [p.detach().clone() for p in list(a.parameters()) + list(b.parameters())]
    x4, x3 = torch.zeros(4, 1, 2048), torch.zeros(3, 1, 2048)
    opt = torch.optim.Adam(list(a.parameters()) + list(b.parameters()), 1e-3)
    with pytest.raises(ValueError, match=r"\(3, 1, 2048\).*\(4, 1, 2048\)"):
        reps.train_epoch([[(x4, x4, None)], [(x3, x3, None)]], ntm.ESRLoss(), opt)
    with pytest.raises(ValueError, match="3 loaders for 2 replicas"):
        reps.train_epoch([[(x4, x4, None)]] * 3, ntm.ESRLoss(), opt)
    assert all(torch.equal(p, q) for p, q in zip(list(a.parameters()) + list(b.parameters()), before))
