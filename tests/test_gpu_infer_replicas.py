"""GPU: R replicas validated and predicted in one launch (ntm_gru_forward_replicas = gru_lat_kernel<HEADW, REP>, Replicas.infer /
validate / predict).  The oracle throughout is the single-model path in the same process -- ntm_gru_forward_ex with NTM_GRU_LAT,
and the models' own validate() / predict() on the replica's slice with the replica's weights -- compared bit for bit (torch.equal,
== on floats): that path is pinned to the reference by tests/test_gpu_parity.py and tests/test_gpu_round3.py (golden g18)."""
import pytest
import torch

from helpers import validate_batches

W_G = "GRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE]_BEST"
W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"
KEYS = ["GRU.weight_ih_l0", "GRU.weight_hh_l0", "GRU.bias_ih_l0", "GRU.bias_hh_l0", "output.weight", "output.bias"]


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def _sds(ntm, R, name=W_G):
    """Replica 0 carries the shipped checkpoint, replica r > 0 a copy perturbed by its own noise (3 % of each tensor's largest
    entry, seed r): a wrong slice of any of the six stacks cannot pass."""
    base = {k: torch.as_tensor(v).float() for k, v in ntm.weights.load_state_dict(name).items()}
    out = [base]
    for r in range(1, R):
        g = torch.Generator().manual_seed(r)
        out.append({k: v + 0.03 * float(v.abs().max()) * torch.randn(v.shape, generator=g) for k, v in base.items()})
    return out


def _stack(sds, bias=True):
    return [torch.stack([sd[k] for sd in sds]).cuda().contiguous() if (bias or k != "output.bias") else None for k in KEYS]


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw_group(ntm, stacks, x, y, R, Bper, T, h):
    L = ntm._lib.lib()
    rc = L.ntm_gru_forward_replicas(*[_p(s) for s in stacks], _p(x), _p(y), R, Bper, T, x.stride(0), y.stride(0), _p(h), _stream())
    assert rc == 0, L.ntm_last_error()


def _raw_single(ntm, stacks, r, x, y, B, T, h):
    L = ntm._lib.lib()
    rc = L.ntm_gru_forward_ex(*[_p(None if s is None else s[r]) for s in stacks], 64, _p(x), _p(y), B, T, x.stride(0), y.stride(0),
                              _p(h), ntm._lib.NTM_GRU_LAT, _stream())
    assert rc == 0, L.ntm_last_error()


def _check_raw(ntm, sds, R, Bper, T, with_state, pad=(0, 0), bias=True):
    """The grouped launch against R single launches on the slices: y (and its padding, untouched) and h_state."""
    B = R * Bper
    g = torch.Generator().manual_seed(1000 * R + 10 * Bper + T)
    stacks = _stack(sds, bias)
    x = torch.zeros(B, T + pad[0])
    x[:, :T] = torch.rand(B, T, generator=g) - 0.5
    x = x.cuda()
    h0 = (0.8 * (torch.rand(B, 64, generator=g) - 0.5)).cuda() if with_state else None
    y = torch.full((B, T + pad[1]), 7.0, device="cuda")
    h = None if h0 is None else h0.clone()
    _raw_group(ntm, stacks, x, y, R, Bper, T, h)
    for r in range(R):
        sl = slice(r * Bper, (r + 1) * Bper)
        xa = x[sl, :T].contiguous()
        ya = torch.full((Bper, T), 7.0, device="cuda")
        ha = None if h0 is None else h0[sl].clone()
        _raw_single(ntm, stacks, r, xa, ya, Bper, T, ha)
        assert torch.equal(y[sl, :T], ya), r
        if with_state:
            assert torch.equal(h[sl], ha), r
    assert bool((y[:, T:] == 7.0).all())
    if T > 2 and R > 1:       # the replicas do differ: equality above is not that of a constant
        assert not torch.equal(y[:Bper, :T], y[Bper:2 * Bper, :T])
    return y


# the sub-tile branches of the tile loop (1, 2, 3, 129), one full 256-sample tile, the first sample of a second tile, and a tile
# with the x prefetch and the delayed y flush
@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 3, 129, 256, 257, 600])
@pytest.mark.parametrize("with_state", [False, True])
def test_the_grouped_kernel_is_bit_identical_to_lat_on_every_slice(ntm, T, with_state):
    sds = _sds(ntm, 3)
    _check_raw(ntm, sds, 3, 2, T, with_state)
    _check_raw(ntm, sds, 3, 2, T, with_state, pad=(5, 3))          # row strides above T


@pytest.mark.gpu
def test_a_null_head_bias_and_R_1(ntm):
    sds = _sds(ntm, 3)
    _check_raw(ntm, sds, 3, 2, 257, True, bias=False)
    # R = 1 IS ntm_gru_forward with the lat variant
    for T in (3, 300):
        _check_raw(ntm, sds[1:2], 1, 5, T, True)


@pytest.mark.gpu
def test_both_head_forms_of_the_grouped_kernel(ntm):
    """More streams than CUs in the group (no head wave) while each replica alone has fewer (head wave), and a group below the
    CU count: each equals its replicas run alone."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    R = 5
    Bper = cus // R + 9
    assert R * Bper > cus >= Bper
    _check_raw(ntm, _sds(ntm, R), R, Bper, 300, True)
    assert 3 * 2 <= cus
    _check_raw(ntm, _sds(ntm, 3), 3, 2, 300, True)


def _model(ntm, sd, kind="gru", max_delay=None):
    m = (ntm.RNN(1, 64, 1) if kind == "gru" else ntm.DiffDelRNN(1, 64, 1, max_delay=max_delay)).cuda()
    m.load_state_dict({k: torch.as_tensor(v).clone() for k, v in sd.items()})
    return m


@pytest.mark.gpu
def test_infer_in_pieces_equals_one_call_and_carries_the_state(ntm):
    R, Bper, T = 3, 2, 700
    sds = _sds(ntm, R)
    x = (torch.rand(R * Bper, 1, T, generator=torch.Generator().manual_seed(3)) - 0.5).cuda()
    one = ntm.Replicas([_model(ntm, sd) for sd in sds])
    y1 = one.infer(x)
    assert y1.shape == x.shape and not y1.requires_grad
    reps = ntm.Replicas([_model(ntm, sd) for sd in sds])
    ys = []
    for a, b in ((0, 256), (256, 257), (257, 700)):
        ys.append(reps.infer(x[:, :, a:b]))
        for r, m in enumerate(reps.models):                 # each model's hidden is its slice of the group's
            assert torch.equal(m.hidden, reps.hidden[:, r * Bper:(r + 1) * Bper])
    assert torch.equal(torch.cat(ys, dim=2), y1)
    assert torch.equal(reps.hidden, one.hidden) and tuple(reps.hidden.shape) == (1, R * Bper, 64)
    for r, sd in enumerate(sds):                            # and the single model's own forward, state included
        m = _model(ntm, sd)
        m.kernel_variant = "lat"
        ya = m(x[r * Bper:(r + 1) * Bper])
        assert torch.equal(y1[r * Bper:(r + 1) * Bper], ya) and torch.equal(one.models[r].hidden, m.hidden), r
    with pytest.raises(ValueError, match="7 streams do not divide into 3 replicas"):
        reps.infer(torch.zeros(7, 1, 8, device="cuda"))
    with pytest.raises(RuntimeError, match=r"Expected hidden size \(1, 3, 64\), got \[1, 6, 64\]"):
        reps.infer(torch.zeros(3, 1, 8, device="cuda"))


# ---- validate, RNN: straight after a grouped train_epoch
VAL_T = 1024 + 700
_CACHE = {}


def _val_loaders(R, shared):
    def loader(seed):
        g = torch.Generator().manual_seed(seed)
        out = []
        for _ in range(2):
            x = torch.rand(2, 1, VAL_T, generator=g) - 0.5
            out.append((x, (0.7 * torch.tanh(1.5 * x) + 0.01 * torch.randn(2, 1, VAL_T, generator=g)).float(), None))
        return out
    return loader(50) if shared else [loader(50 + r) for r in range(R)]


def _plain_loss(pred, target):
    return ((pred - target) ** 2).mean() / ((target ** 2).mean() + 1e-5)


def _loss(ntm, name):
    return {"esr": ntm.ESRLoss(), "dcpre": ntm.DCPreESR(dc_pre=True), "plain": _plain_loss}[name]


def _trained_group(ntm):
    """R = 3 models after ONE grouped train_epoch of one short batch (requires_grad is on from there on); built once."""
    if "trained" not in _CACHE:
        R = 3
        models = [_model(ntm, sd) for sd in _sds(ntm, R)]
        reps = ntm.Replicas(models)
        g = torch.Generator().manual_seed(9)
        x = torch.rand(2, 1, 2048, generator=g) - 0.5
        reps.train_epoch([(x, 0.5 * x, None)], ntm.ESRLoss(), [torch.optim.Adam(m.parameters(), lr=1e-3) for m in models])
        assert all(p.requires_grad for m in models for p in m.parameters())
        _CACHE["trained"] = (reps, [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in models])
    return _CACHE["trained"]


def _alone_validate(ntm, loss_name, shared):
    """Every replica's own validate() on its own loader, from the trained weights; computed once, never modified."""
    key = ("alone", loss_name, shared)
    if key not in _CACHE:
        _, sds = _trained_group(ntm)
        loaders = _val_loaders(len(sds), shared)
        _CACHE[key] = [_model(ntm, sd).validate(loaders if shared else loaders[r], _loss(ntm, loss_name))
                       for r, sd in enumerate(sds)]
    return _CACHE[key]


def _same_results(got, want):
    assert len(got) == len(want)
    for r, ((v, ex), (va, exa)) in enumerate(zip(got, want)):
        assert v == va, (r, v, va)
        assert len(ex) == len(exa)
        for e, ea in zip(ex, exa):
            assert list(e) == list(ea)
            for k in e:
                assert not e[k].requires_grad and torch.equal(e[k], ea[k]), (r, k)


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name", ["esr", "dcpre", "plain"])
@pytest.mark.parametrize("shared", [True, False])
def test_validate_gives_every_replica_the_bits_of_its_own_validate(ntm, loss_name, shared):
    reps, sds = _trained_group(ntm)
    got = reps.validate(_val_loaders(len(sds), shared), _loss(ntm, loss_name))
    _same_results(got, _alone_validate(ntm, loss_name, shared))
    assert len({v for v, _ in got}) == len(sds)                                    # three different models
    assert all(len(ex) == 2 and ex[0]["prediction"].shape == (700,) for _, ex in got)
    assert not reps.hidden.requires_grad and all(not m.hidden.requires_grad for m in reps.models)       # no graph left behind
    assert all(p.requires_grad and p.grad_fn is None for m in reps.models for p in m.parameters())
    v2, ex2 = reps.validate(_val_loaders(len(sds), shared), _loss(ntm, loss_name), store_examples=False)[1]
    assert v2 == got[1][0] and ex2 == []


@pytest.mark.gpu
def test_two_identical_grouped_validations_are_identical_and_the_refusals(ntm):
    reps, sds = _trained_group(ntm)
    a = reps.validate(_val_loaders(3, False), ntm.DCPreESR(dc_pre=True))
    b = reps.validate(_val_loaders(3, False), ntm.DCPreESR(dc_pre=True))
    _same_results(a, b)
    with pytest.raises(ValueError, match="2 loaders for 3 replicas"):
        reps.validate(_val_loaders(2, False), ntm.ESRLoss())
    x4, x3 = torch.zeros(4, 1, 1100), torch.zeros(3, 1, 1100)
    with pytest.raises(ValueError, match=r"\(3, 1, 1100\).*\(4, 1, 1100\)"):
        reps.validate([[(x4, x4, None)], [(x3, x3, None)], [(x4, x4, None)]], ntm.ESRLoss())
    with pytest.raises(ValueError, match="different lengths"):
        reps.validate([[(x4, x4, None)], [(x4, x4, None)] * 2, [(x4, x4, None)]], ntm.ESRLoss())


# ---- validate, DiffDelRNN
FS = 44100
INIT = 512                       # nextpow2(int(300 / FS * FS)): the analyser's warm-up length of the stub dataset


class _Loader(list):
    """The reference's DataLoader as validate sees it: (x, t, meta) batches and .dataset.fs / .dataset.delay_analyzer."""

    def __init__(self, batches, fs=FS, max_delay_s=300.5 / FS):
        super().__init__(batches)
        self.dataset = type("DS", (), {"fs": fs, "delay_analyzer": type("DA", (), {"max_delay": max_delay_s})})


def _dd_loader(seed, T, n_batches=2):
    return _Loader([(torch.from_numpy(x), torch.from_numpy(t), {"delay_trajectory": torch.from_numpy(d).float()})
                    for x, t, d in validate_batches(seed, n_batches, 2, T, FS)])


@pytest.mark.gpu
@pytest.mark.parametrize("D", [INIT - 1, INIT + 8])       # the delay buffer just below / just above the warm-up length
@pytest.mark.parametrize("loss_name", ["dcpre", "plain"])
def test_diffdel_validate_gives_every_replica_the_bits_of_its_own_validate(ntm, D, loss_name):
    from ntm_amd.utilities import nextpow2
    T = INIT + 2 * 2048                                    # two 2048-sample pieces after the warm-up
    sds = _sds(ntm, 2, W_D)
    assert nextpow2(int(_Loader([]).dataset.delay_analyzer.max_delay * FS)) == INIT
    models = [_model(ntm, sd, "diffdel", D - 1) for sd in sds]
    for m in models:
        for p in m.parameters():
            p.requires_grad_(True)                         # as train_epoch leaves them
    reps = ntm.Replicas(models)
    loss = _loss(ntm, loss_name)
    got = reps.validate([_dd_loader(70, T), _dd_loader(71, T)], loss)
    want = [_model(ntm, sd, "diffdel", D - 1).validate(_dd_loader(70 + r, T), loss) for r, sd in enumerate(sds)]
    _same_results(got, want)
    assert list(got[0][1][0]) == ["input", "target", "prediction", "prediction_pre_d"] and got[0][0] != got[1][0]
    assert got[0][1][0]["prediction_pre_d"].shape == (2 * 2048,)
    shared = reps.validate(_dd_loader(70, T), loss)        # one loader for both
    assert shared[0][0] == want[0][0] and torch.equal(shared[0][1][1]["prediction"], want[0][1][1]["prediction"])
    assert shared[1][0] != want[1][0]


@pytest.mark.gpu
def test_diffdel_validate_refusals(ntm):
    D = INIT + 8
    sds = _sds(ntm, 2, W_D)
    reps = ntm.Replicas([_model(ntm, sd, "diffdel", D - 1) for sd in sds])
    with pytest.raises(ZeroDivisionError):                 # T <= INIT_LEN: no piece follows the warm-up
        reps.validate(_dd_loader(5, INIT, 1), ntm.ESRLoss())
    with pytest.raises(ZeroDivisionError):
        _model(ntm, sds[0], "diffdel", D - 1).validate(_dd_loader(5, INIT, 1), ntm.ESRLoss())
    with pytest.raises(ValueError, match="different warm-up lengths"):
        reps.validate([_dd_loader(5, 4096, 1), _Loader(_dd_loader(5, 4096, 1), FS, 600.5 / FS)], ntm.ESRLoss())
    # a trajectory above the buffer in ONE replica: AssertionError, and no replica's buffer has moved
    Bper, T = 2, 600
    g = torch.Generator().manual_seed(4)
    x = (torch.rand(2 * Bper, 1, T, generator=g) - 0.5).cuda()
    d = torch.full((2 * Bper, 1, T), 100.0, device="cuda")
    reps.initialize_hidden(Bper)
    reps.infer(x, d, warmup=True)
    bufs = [m.diffdel.buffer.clone() for m in reps.models]
    assert bool(bufs[0].any()) and tuple(bufs[0].shape) == (Bper, 1, D)
    bad = d.clone()
    bad[3, 0, 77] = D + 0.5                                # replica 1
    with pytest.raises(AssertionError):
        reps.infer(x, bad)
    assert all(torch.equal(m.diffdel.buffer, b) for m, b in zip(reps.models, bufs))
    y, pre = reps.infer(x, d)                              # the flag is cleared: the next good call runs
    assert not torch.equal(reps.models[0].diffdel.buffer, bufs[0]) and not y.requires_grad and not pre.requires_grad
    good, worse = _dd_loader(6, INIT + 2048, 1), _dd_loader(6, INIT + 2048, 1)
    worse[0][2]["delay_trajectory"][1, INIT + 5] = (D + 3.0) / FS
    with pytest.raises(AssertionError):
        reps.validate([good, worse], ntm.ESRLoss())


# ---- predict
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gru", "diffdel"])
def test_predict_is_every_models_predict_and_follows_a_change_of_the_weights(ntm, kind):
    R, Bper, T, D = 2, 3, 600, 300
    sds = _sds(ntm, R, W_G if kind == "gru" else W_D)
    g = torch.Generator().manual_seed(12)
    x = (torch.rand(R * Bper, 1, T, generator=g) - 0.5).cuda()
    n = torch.arange(T, dtype=torch.float32)
    d = (120.0 + 80.0 * torch.sin(n / 37.0) + 10.0 * torch.rand(R * Bper, 1, 1, generator=g)).expand(R * Bper, 1, T).contiguous().cuda()
    extra = () if kind == "gru" else (d,)
    group = [_model(ntm, sd, kind, D - 1) for sd in sds]
    alone = [_model(ntm, sd, kind, D - 1) for sd in sds]
    for m in group + alone:
        m.warm_cache = True                                # the single models serve their warm state from the cache the second time
    reps = ntm.Replicas(group)

    def tup(v):
        return v if isinstance(v, tuple) else (v,)

    def check(seg):
        got = tup(reps.predict(x, *extra, segment_length=seg))
        assert len(got) == len(extra) + 1 and all(o.shape == x.shape and not o.requires_grad for o in got)
        for r, m in enumerate(alone):
            sl = slice(r * Bper, (r + 1) * Bper)
            want = tup(m.predict(x[sl], *(e[sl] for e in extra), segment_length=seg))
            for a, b in zip(got, want):
                assert torch.equal(a[sl], b), (r, seg)
            assert torch.equal(group[r].hidden, m.hidden), r
            if kind == "diffdel":
                assert torch.equal(group[r].diffdel.buffer, m.diffdel.buffer), r
        return got
    whole = check(None)
    pieces = check(256)
    assert all(torch.equal(a, b) for a, b in zip(whole, pieces))
    with torch.no_grad():                                  # in place: the parameter's version counter moves, its storage stays
        for m in (group[1], alone[1]):
            m.GRU.weight_hh_l0.mul_(0.9)
    again = check(None)
    assert torch.equal(again[0][:Bper], whole[0][:Bper]) and not torch.equal(again[0][Bper:], whole[0][Bper:])
    with pytest.raises(ValueError, match="5 streams do not divide into 2 replicas"):
        reps.predict(x[:5], *(e[:5] for e in extra))
