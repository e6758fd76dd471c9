"""CPU: the shared TBPTT epoch, validation and predict-segment loops (ntm_amd.epoch) driven by a stub group in plain torch.
The expected call sequences, window counts and piece lengths are literals transcribed from the reference's loops
(code/model.py:90-216 for RNN, :426-616 for DiffDelRNN), not read from the code under test."""
import pytest
import torch

import ntm_amd
from ntm_amd import epoch

W0, LR = 0.4, 1e-9


class _Model(torch.nn.Module):
    def __init__(self, w):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(float(w)))

    def _check_trainable(self, who):
        pass


class _Group:
    """R stub replicas: pred = w_r * x + carry, carry <- the last predicted sample; every call is logged.  The input is a ramp,
    so a slice shows its own offset: forwards are logged as ("forward", first sample, length, warmup)."""
    name, device = "Stub", torch.device("cpu")

    def __init__(self, R, schedule, ws=None):
        self.models = [_Model(W0 if ws is None else ws[r]) for r in range(R)]
        self.schedule, self.log, self.delays, self.carry = schedule, [], [], None

    def reset(self, Bper):
        self.carry = None
        self.log.append(("reset",))

    def stepper(self, train):
        def step(x, d_traj, warmup):
            R = len(self.models)
            n = x.shape[0] // R
            self.log.append(("forward", float(x[0, 0, 0]) if x.shape[-1] else None, x.shape[-1], bool(warmup)))
            assert (d_traj is not None) == self.schedule.delays
            if d_traj is not None:
                self.delays.append(d_traj.clone())
            carry = torch.zeros(x.shape[0], 1, 1) if self.carry is None else self.carry
            pred = torch.cat([m.w * x[r * n:(r + 1) * n] + carry[r * n:(r + 1) * n] for r, m in enumerate(self.models)])
            self.carry = pred[:, :, -1:]
            return pred, (2 * x if self.schedule.delays else None)
        return step

    def detach_hidden(self):
        self.carry = self.carry.detach()
        self.log.append(("detach",))

    def zero_grad(self):
        for m in self.models:
            m.zero_grad()
        self.log.append(("zero_grad",))

    def grouped_loss(self, loss_fcn):
        return None


class _SGD:
    def __init__(self, group, lr=LR):
        self.group, self.lr, self.seen = group, lr, []

    def step(self):
        with torch.no_grad():
            for m in self.group.models:
                m.w -= self.lr * m.w.grad
        self.seen.append([float(m.w.detach()) for m in self.group.models])
        self.group.log.append(("step",))


class _MSE:
    """A loss without a grouped form; logs each call and the (shape, stride) of both arguments."""

    def __init__(self, log=None):
        self.log, self.layouts = log, []

    def __call__(self, pred, target):
        if self.log is not None:
            self.log.append(("loss",))
        self.layouts.append((tuple(pred.shape), pred.stride(), tuple(target.shape), target.stride()))
        return ((pred - target) ** 2).mean()


class _DS:
    fs, max_delay = 100, 0.3                 # warm-up nextpow2(int(0.3 * 100)) = nextpow2(30) = 32


class _Loader(list):
    dataset = _DS


def _ramp(B, T, seed=0):
    x = torch.arange(T, dtype=torch.float32).expand(B, 1, T).contiguous()
    t = 0.5 * x + torch.rand(B, 1, T, generator=torch.Generator().manual_seed(seed))
    return x, t


def _dd_batch(B, T, seed=0, meta=True):
    x, t = _ramp(B, T, seed)
    d = 0.001 * torch.rand(B, T, generator=torch.Generator().manual_seed(seed + 100)).double()      # seconds
    return (x, t, {"delay_trajectory": d}) if meta else (x, t, d.unsqueeze(1), None)


def _windows(w0, x, t, init, window, count):
    """The mean window loss of one batch by the stub's formula: warm-up in the graph, SGD after every window."""
    w = torch.tensor(w0, requires_grad=True)
    carry = (w * x[:, :, :init])[:, :, -1:]
    losses = []
    for k in range(count):
        sl = slice(init + k * window, init + (k + 1) * window)
        pred = w * x[:, :, sl] + carry
        loss = ((pred - t[:, :, sl]) ** 2).mean()
        g, = torch.autograd.grad(loss, w)
        losses.append(loss.item())
        w = (w.detach() - LR * g).requires_grad_(True)
        carry = pred[:, :, -1:].detach()
    return sum(losses) / count


def test_the_two_schedules_are_the_references_numbers():
    r, d = epoch.RNN_SCHEDULE, epoch.DIFFDEL_SCHEDULE
    assert (r.warmup(None), r.window, r.delays, r.val_pieces) == (1024, 1024, False, None)
    assert (d.warmup(_DS), d.window, d.delays) == (32, 2048, True)
    assert [r.train_windows(n, 1024) for n in (-24, 1023, 1024, 2055)] == [-1, 0, 1, 2]
    assert [d.train_windows(n, 2048) for n in (2047, 2048, 4101)] == [0, 1, 2]
    assert [d.val_pieces(n, 2048) for n in (0, 1, 2048, 2053)] == [0, 1, 1, 2]
    assert ntm_amd.RNN.schedule is r and ntm_amd.DiffDelRNN.schedule is d


def test_rnn_training_call_log_windows_and_return_value():
    T = 3079                                                    # 1024 + 2 * 1024 + 7
    x, t = _ramp(2, T)
    x[:, :, -7:] = t[:, :, -7:] = float("nan")                  # never read
    g = _Group(1, epoch.RNN_SCHEDULE)
    loss, opt = _MSE(g.log), _SGD(g)
    out = epoch.train_epoch(g, [[(x, t)]], loss, opt)
    window = [("loss",), ("step",), ("detach",), ("zero_grad",)]
    assert g.log == ([("reset",), ("forward", 0.0, 1024, True), ("zero_grad",)]
                     + [("forward", 1024.0, 1024, False)] + window + [("forward", 2048.0, 1024, False)] + window)
    assert max(e[1] + e[2] for e in g.log if e[0] == "forward") == 3072
    assert len(out) == 1 and out[0] == pytest.approx(_windows(W0, x, t, 1024, 1024, 2), rel=1e-6)
    assert len(opt.seen) == 2 and W0 != opt.seen[0][0] != opt.seen[1][0]
    assert all(m.training and m.w.requires_grad for m in g.models)


@pytest.mark.parametrize("meta", [True, False])
def test_diffdel_training_warmup_windows_and_delays(meta):
    T = 32 + 2 * 2048 + 5
    batch = _dd_batch(2, T, meta=meta)
    g = _Group(1, epoch.DIFFDEL_SCHEDULE)
    out = epoch.train_epoch(g, _Loader([batch]), _MSE(), _SGD(g))
    assert [e for e in g.log if e[0] == "forward"] == [("forward", 0.0, 32, True), ("forward", 32.0, 2048, False),
                                                       ("forward", 2080.0, 2048, False)]
    seconds = batch[2]["delay_trajectory"].unsqueeze(1) if meta else batch[2]
    want = seconds.float() * 100
    got = torch.cat(g.delays, dim=2)
    assert got.dtype == torch.float32 and torch.equal(got, want[:, :, :32 + 2 * 2048])
    assert out[0] == pytest.approx(_windows(W0, batch[0], batch[1], 32, 2048, 2), rel=1e-6)
    # the dataset may be handed over instead of being the loader's
    g2 = _Group(1, epoch.DIFFDEL_SCHEDULE)
    assert epoch.train_epoch(g2, [batch], _MSE(), _SGD(g2), dataset=_DS) == out


def test_window_counts_at_the_edges_in_training():
    def run(schedule, T):
        g = _Group(1, schedule)
        batch = _ramp(2, T) if schedule is epoch.RNN_SCHEDULE else _dd_batch(2, T)
        return epoch.train_epoch(g, _Loader([batch]), _MSE(), _SGD(g)), g
    with pytest.raises(ZeroDivisionError):
        run(epoch.RNN_SCHEDULE, 2047)
    out, g = run(epoch.RNN_SCHEDULE, 1000)      # shorter than the warm-up: the count is -1, the loop empty, 0 / -1
    assert out == [0.0] and [e for e in g.log if e[0] in ("forward", "loss", "step")] == [("forward", 0.0, 1000, True)]
    with pytest.raises(ZeroDivisionError):
        run(epoch.DIFFDEL_SCHEDULE, 32 + 2047)


def test_validation_pieces_and_examples():
    # DiffDel: ceil(2053 / 2048) = 2 pieces of 2048 and 5 samples, the batch loss their mean
    x, t, meta = _dd_batch(2, 32 + 2048 + 5)
    g, loss = _Group(1, epoch.DIFFDEL_SCHEDULE), _MSE()
    (val, examples), = epoch.validate(g, _Loader([(x, t, meta)]), loss)
    assert [e for e in g.log if e[0] == "forward"] == [("forward", 0.0, 32, True), ("forward", 32.0, 2053, False)]
    assert [lay[0][-1] for lay in loss.layouts] == [2048, 5]
    pred = W0 * x[:, :, 32:] + W0 * 31.0
    pieces = [((pred[:, :, a:b] - t[:, :, 32 + a:32 + b]) ** 2).mean().item() for a, b in ((0, 2048), (2048, 2053))]
    assert val == pytest.approx(sum(pieces) / 2, rel=1e-6)
    assert sorted(examples[0]) == ["input", "prediction", "prediction_pre_d", "target"]
    assert all(v.shape == (2053,) for v in examples[0].values())
    assert torch.equal(examples[0]["input"], x[0, 0, 32:]) and torch.equal(examples[0]["prediction_pre_d"], 2 * x[0, 0, 32:])
    assert not any(m.training for m in g.models)
    with pytest.raises(ZeroDivisionError):
        epoch.validate(_Group(1, epoch.DIFFDEL_SCHEDULE), _Loader([_dd_batch(2, 32)]), _MSE())
    # RNN: everything after the warm-up as ONE piece, no division
    x, t = _ramp(2, 1030)
    g, loss = _Group(1, epoch.RNN_SCHEDULE), _MSE()
    (val, examples), = epoch.validate(g, [[(x, t, None)]], loss, store_examples=True)
    assert [e for e in g.log if e[0] == "forward"] == [("forward", 0.0, 1024, True), ("forward", 1024.0, 6, False)]
    assert [lay[0][-1] for lay in loss.layouts] == [6]
    assert val == pytest.approx(((W0 * x[:, :, 1024:] + W0 * 1023.0 - t[:, :, 1024:]) ** 2).mean().item(), rel=1e-6)
    assert sorted(examples[0]) == ["input", "prediction", "target"] and all(v.shape == (6,) for v in examples[0].values())
    assert epoch.validate(_Group(1, epoch.RNN_SCHEDULE), [[(x, t, None)]], _MSE(), store_examples=False)[0] == (val, [])


@pytest.mark.parametrize("kind", ["rnn", "diffdel"])
def test_every_replica_sees_the_single_models_layout_and_gives_its_numbers(kind):
    """Layout and R independence: one shared loader, replicas started equal."""
    if kind == "rnn":
        schedule, T_train, T_val = epoch.RNN_SCHEDULE, 1024 + 2 * 1024 + 7, 1024 + 300
        train = _Loader([_ramp(2, T_train, s) for s in (1, 2)])
        val = _Loader([_ramp(2, T_val, s) + (None,) for s in (3, 4)])
    else:
        schedule, T_train, T_val = epoch.DIFFDEL_SCHEDULE, 32 + 2 * 2048 + 5, 32 + 2048 + 5
        train = _Loader([_dd_batch(2, T_train, s) for s in (1, 2)])
        val = _Loader([_dd_batch(2, T_val, s) for s in (3, 4)])
    results = {}
    for R in (1, 2, 3):
        g, loss = _Group(R, schedule), _MSE()
        trained = epoch.train_epoch(g, train, _MSE(), _SGD(g))
        validated = epoch.validate(g, val, loss)
        results[R] = (trained, [v for v, _ in validated], loss.layouts, [float(m.w.detach()) for m in g.models])
    one = results[1]
    for R in (2, 3):
        trained, validated, layouts, ws = results[R]
        assert trained == one[0] * R and validated == one[1] * R and ws == one[3] * R
        calls = len(one[2]) // 2                                  # per batch: the loop visits replica by replica
        for b in range(2):
            for r in range(R):
                at = b * R * calls + r * calls
                assert layouts[at:at + calls] == one[2][b * calls:(b + 1) * calls], (R, b, r)
    B, T0 = 2, T_val - schedule.warmup(_DS)
    if kind == "rnn":           # a fresh contiguous prediction, the target a slice of the whole-length one
        assert one[2][0] == ((B, 1, T0), (T0, T0, 1), (B, 1, T0), (T_val, T_val, 1))
    else:                       # slices of whole-length buffers
        assert one[2][:2] == [((B, 1, 2048), (T_val, T_val, 1)) * 2, ((B, 1, 5), (T_val, T_val, 1)) * 2]


def test_loader_rules():
    sch = epoch.RNN_SCHEDULE
    a, b = [_ramp(2, 3072, 1), _ramp(2, 3072, 2)], [_ramp(2, 3072, 3), _ramp(2, 3072, 4)]
    alone = []
    for loader in (a, b):
        g = _Group(1, sch)
        alone.append(epoch.train_epoch(g, [loader], _MSE(), _SGD(g))[0])
    g = _Group(2, sch)
    assert epoch.train_epoch(g, [a, b], _MSE(), _SGD(g)) == alone                   # a list of R loaders is zipped
    g = _Group(2, sch)
    assert epoch.train_epoch(g, a, _MSE(), _SGD(g)) == [alone[0]] * 2               # one loader is shared
    g = _Group(2, sch)
    assert epoch.train_epoch(g, (batch for batch in a), _MSE(), _SGD(g)) == [alone[0]] * 2       # a generator serves
    g = _Group(2, sch)
    with pytest.raises(ValueError, match="3 loaders for 2 replicas"):
        epoch.train_epoch(g, [a, b, a], _MSE(), _SGD(g))
    va, vb = [_ramp(2, 1100, 1) + (None,)], [_ramp(2, 1100, 2) + (None,)] * 2
    with pytest.raises(ValueError, match=r"different lengths \[1, 2\]"):
        epoch.validate(_Group(2, sch), [va, vb], _MSE())
    # shapes that differ across replicas: refused before any forward of that iteration
    for run in (lambda g: epoch.train_epoch(g, [a, [a[0], _ramp(3, 3072)]], _MSE(), _SGD(g)),
                lambda g: epoch.validate(g, [va + va, [va[0], _ramp(3, 1100) + (None,)]], _MSE())):
        g = _Group(2, sch)
        with pytest.raises(ValueError, match=r"replica 1 has shape \(3, 1, \d+\), that of replica 0 \(2, 1, \d+\)"):
            run(g)
        assert [e[0] for e in g.log].count("reset") == 1          # the first iteration ran, the second launched nothing
    dd = _Group(2, epoch.DIFFDEL_SCHEDULE)

    class Other:
        fs, max_delay = 100, 0.7
    with pytest.raises(ValueError, match=r"different warm-up lengths \[32, 128\]"):
        epoch.train_epoch(dd, [[_dd_batch(2, 5000)]] * 2, _MSE(), _SGD(dd), dataset=[_DS, Other])
    assert dd.log == []


@pytest.mark.parametrize("outputs", [1, 2])
@pytest.mark.parametrize("segment_length", [4, 10])
def test_the_segment_helper_equals_one_whole_call(segment_length, outputs):
    x = torch.arange(10, dtype=torch.float32).expand(2, 1, 10).contiguous()

    def stateful():
        state, ran = [0.0], []

        def run(sl):
            seg = x[:, :, sl]
            ran.append((int(seg[0, 0, 0]), seg.shape[-1]))
            y = seg.cumsum(-1) + state[0]
            state[0] = y[:, :, -1:]
            return (y, -y)[:outputs]
        return run, ran
    run, _ = stateful()
    whole = epoch.in_segments(run, x, None, outputs)
    run, ran = stateful()
    got = epoch.in_segments(run, x, segment_length, outputs)
    assert ran == ([(0, 4), (4, 4), (8, 2)] if segment_length == 4 else [(0, 10)])
    assert len(got) == len(whole) == outputs and all(torch.equal(a, b) for a, b in zip(got, whole))
    assert torch.equal(whole[0], x.cumsum(-1))
