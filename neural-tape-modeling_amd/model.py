"""Host-side mirror of the reference's model objects for the tape-nonlinearity forward path.

Same class names, constructor arguments, state_dict keys, methods, argument order, return arity and
error behaviour as code/model.py of the reference (RNN :20-246, TimeVaryingDelayLine :249-332,
DiffDelRNN :335-653), so a caller such as code/test-model.py:217-234,346,353 can switch by changing
one import.  The arithmetic runs in libntm.so (hand-written HIP, gfx950); torch is used for device
memory, streams and parameter bookkeeping only.  There is NO CPU path: a non-HIP tensor raises.

Deliberate differences from the reference (documented in DESIGN.md):
  * predict() works for any batch size: the zero-input warm-up (identical for every stream) is run
    once with B=1 and its state broadcast -- per stream this is exactly the reference's B=1 maths
    (the reference raises for B>1).
  * predict() runs the whole sequence in one persistent launch; `segment_length=2048` reproduces
    the reference's chunk loop (same result, state is carried either way).
  * validate() (code/model.py:163-216, :513-616 -- the reference's own batched, inference-only use of forward,
    called by code/train.py:242) and detach_hidden / detach_buffer are here.  RNN.train_epoch (code/model.py:90-161) trains
    GRU-HS[64] with input_size = output_size = 1 and no skip connection on the kernels of csrc/gru_train.hip (training.py);
    parameters are created with requires_grad=False and train_epoch turns it on.  forward() builds a graph only when grad
    mode is on AND a parameter requires grad; every other call is the inference path, unchanged.  DiffDelRNN.train_epoch
    (code/model.py:426-511) trains DiffDelGRU-HS[64] the same way, with the delay line's adjoint on the device.  The loops
    themselves -- warm-up, windows, pieces, the window counts -- are written once, in epoch.py (epoch.RNN_SCHEDULE,
    epoch.DIFFDEL_SCHEDULE, epoch.train_epoch, epoch.validate): the train_epoch / validate methods of RNN, DiffDelRNN and
    Replicas are their docstring and one call, a single model going in as a group of one (_Single) that calls its own forward.
  * warm_start() from a fresh state is a pure function of the parameters.  With `warm_cache = True` its result (hidden
    state; for the DiffDelGRU also the delay buffer) is computed by the kernel ONCE per (parameter storage + torch version
    counter, device, kernel variant, delay-line length) and kept, so a predict() is one launch instead of two -- same numbers
    as recomputing it (code/model.py:58-65, :382-391 recompute it every time).  The class default is OFF (every predict()
    recomputes, exactly the reference's behaviour): torch's version counters see load_state_dict, `.to()`, and every in-place
    op on the Parameter, but NOT writes through `.data` (`p.data.mul_()`, `p.data.copy_()`) -- a cache keyed on them would
    serve a stale state there without any error.  harness.build_model() turns the cache ON for the evaluation path
    (code/test-model.py:192-247: construct, load best.pth, .eval(), never touched again) and bench.py reports the step both
    ways; whoever enables it elsewhere and writes through `.data` calls `invalidate_warm_cache()` (tests/test_gpu_round4.py).
"""
import contextlib

import numpy as np
import torch

from . import _lib, epoch, training
from ._lib import ptr

START_LEN = 2**10          # warm_start(): samples of silence (code/model.py:58-65, :382-391)


class _GRUParams(torch.nn.Module):
    """Parameter container with torch.nn.GRU's names/shapes/init (single layer, gate order r,z,n)."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        k = 1.0 / np.sqrt(hidden_size)
        mk = lambda *shape: torch.nn.Parameter(torch.empty(*shape).uniform_(-k, k), requires_grad=False)  # noqa: E731
        self.weight_ih_l0 = mk(3 * hidden_size, input_size)
        self.weight_hh_l0 = mk(3 * hidden_size, hidden_size)
        self.bias_ih_l0 = mk(3 * hidden_size)
        self.bias_hh_l0 = mk(3 * hidden_size)


class _LinearParams(torch.nn.Module):
    """Parameter container with torch.nn.Linear's names/shapes/init."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        k = 1.0 / np.sqrt(in_features)
        self.weight = torch.nn.Parameter(torch.empty(out_features, in_features).uniform_(-k, k),
                                         requires_grad=False)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_features).uniform_(-k, k), requires_grad=False)
        else:
            self.register_parameter("bias", None)


def _require_hip(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on '{t.device}'; this engine runs on a HIP device only "
                           "(no CPU fallback)")


def _as_bt(x, what):
    """(B,1,T) float32/float64 -> contiguous float32 [B,T] view, like code/model.py:76-77."""
    if x.dim() != 3:
        raise RuntimeError(f"{what}: expected (N_BATCHES, N_CHANNELS, N_SAMPLES), got {tuple(x.shape)}")
    if x.shape[1] != 1:
        raise RuntimeError(f"{what}: input_size 1 expected, got {x.shape[1]} channels")
    _require_hip(x, what)
    x = x.float() if x.dtype != torch.float32 else x
    return x.contiguous().view(x.shape[0], x.shape[2])


def _bt_pair(who, x, del_traj, delays=True):
    """(x, del_traj) (N,1,T) -> their [B,T] fp32 forms, of one shape; without `delays` (x [B,T], None)."""
    xbt = _as_bt(x, who)
    if not delays:
        return xbt, None
    if del_traj is None:
        raise RuntimeError(f"{who}: DiffDelRNN replicas need a delay trajectory")
    dbt = _as_bt(del_traj, who)
    if dbt.shape != xbt.shape:
        raise RuntimeError(f"shape mismatch: x {tuple(x.shape)} vs del_traj {tuple(del_traj.shape)}")
    return xbt, dbt


def _initial_state(hidden, B, H, device, own=False):
    """The initial hidden state [B,H] fp32 on `device` for B streams from the carried `hidden` (1,B,H): zeros when none is
    carried, else a VIEW of it that stays in its graph (the training paths chain dh0 to the previous window through it);
    `own`: a detached tensor of its own, which the inference kernels update in place."""
    if hidden is None:
        return torch.zeros(B, H, device=device, dtype=torch.float32)
    if tuple(hidden.shape) != (1, B, H):
        raise RuntimeError(f"Expected hidden size (1, {B}, {H}), got {list(hidden.shape)}")
    if own:
        hidden = hidden.detach()
    h0 = hidden.to(device=device, dtype=torch.float32).reshape(B, H)
    return h0.clone() if own else h0


def _train_forward(who, owner, x, del_traj, warmup, params, R, dl):
    """The stateful forward of RNN, DiffDelRNN (R None, `params` the six parameters, b_o None for the bias-free head) and Replicas
    (`params` the [R, ...] stacks) as graph nodes: training.GRUTrainStep from `owner.hidden`, which becomes the differentiable
    final state, then with a delay line `dl` training.DelayLineStep.  -> (y, pre_d) (N,1,T); (y, None) without a delay line.
    The new delay buffer is a fresh tensor (the warm-up's outputs in it stay in the graph of the first window); a delay above
    the buffer raises AssertionError (code/model.py:284) with the buffer as it was -- the hidden state has moved on by then, as in
    the reference, where the GRU runs before the delay line asserts."""
    if x.requires_grad or (del_traj is not None and del_traj.requires_grad):
        what, state, only = (("input", "the parameters and the hidden state", training.SUPPORTED) if dl is None else
                             ("input or the delay trajectory", "the parameters, the hidden state and the delay buffer",
                              training.SUPPORTED_DIFFDEL))
        raise RuntimeError(f"{who}: the {what} requires grad; the training kernels give gradients for {state} only ({only})")
    xbt, dbt = _bt_pair(who, x, del_traj, dl is not None)
    B, T = xbt.shape
    if R is not None and B % R:
        raise ValueError(f"{who}: {B} streams do not divide into {R} replicas")
    h0 = _initial_state(owner.hidden, B, training.HIDDEN, xbt.device)
    if dl is not None:
        dl._prepare(B, xbt.device)
    pre, h = training.GRUTrainStep.apply(xbt, h0, *params, R)
    owner.hidden = h.view(1, B, training.HIDDEN)
    if dl is None:
        return pre.view(B, 1, T), None
    y, buf = training.DelayLineStep.apply(pre, dl.buffer, dbt, bool(warmup), dl._err)
    dl._launched()               # raises BEFORE the buffer moves on: a violating call leaves it as it was
    dl.buffer = buf
    return y.view(B, 1, T), pre.view(B, 1, T)


class _GRUHead(torch.nn.Module):
    """GRU(1,H) + Linear(H,1[,bias]) state and launch logic shared by RNN and DiffDelRNN."""

    # product kernels (libntm.so): "auto" | "mfma2" | "lat" | "f16x3" / "bf16x3" (opt-in split engines);  laboratory kernels for A/B and as
    # independent implementations in the tests (libntm_lab.so): "mfma" | "valu"  (NTM_GRU_*)
    kernel_variant = "auto"
    warm_cache = False         # True: keep the warm-start state per parameter version (module docstring; harness.build_model turns it on)

    def _warm_key(self, *extra):
        """Identity of everything warm_start() depends on: the parameter tensors (storage + torch version counter,
        bumped by load_state_dict / any in-place update; .to(device) replaces the storage), kernel variant, sizes."""
        ps = [self.GRU.weight_ih_l0, self.GRU.weight_hh_l0, self.GRU.bias_ih_l0, self.GRU.bias_hh_l0,
              self.output.weight, self.output.bias]
        return (tuple((p.data_ptr(), p._version, str(p.device)) for p in ps if p is not None), self.kernel_variant,
                self.hidden_size, bool(self.skip)) + extra

    def invalidate_warm_cache(self):
        self._warm = None

    def _init_net(self, input_size, hidden_size, output_size, skip, head_bias, general_io=False):
        for what, v in (("input_size", input_size), ("output_size", output_size)):
            if not isinstance(v, (int, np.integer)) or not 1 <= v <= 1024:
                raise ValueError(f"{what} {v!r}: an integer in [1, 1024]")
        if (input_size != 1 or output_size != 1) and not general_io:
            raise ValueError("DiffDelRNN is built for input_size = output_size = 1 (its delay line is single-channel; every "
                             "reference checkpoint and caller uses 1: code/test-model.py:124-125); RNN takes any sizes")
        input_size, output_size = int(input_size), int(output_size)
        # any hidden size the reference can be trained with (`--HIDDEN_SIZE` is a free integer, code/train.py:50): 64 (every
        # shipped checkpoint) has the matrix-pipe / low-latency kernels, 8 / 16 / 32 their own, every other size up to
        # 1024 the padded or wide kernels of csrc/gru_small.hip
        if not isinstance(hidden_size, (int, np.integer)) or not 1 <= hidden_size <= _lib.MAX_HIDDEN:
            raise ValueError(f"hidden_size {hidden_size!r}: an integer in [1, {_lib.MAX_HIDDEN}] (reference default 8, "
                             "code/model.py:22; training default 16, code/train.py:50; every shipped checkpoint is HS[64])")
        hidden_size = int(hidden_size)
        self.input_size, self.hidden_size, self.output_size, self.skip = input_size, hidden_size, output_size, skip
        self.GRU = _GRUParams(input_size, hidden_size)
        self.output = _LinearParams(hidden_size, output_size, bias=head_bias)
        self.hidden = None
        self._warm = None          # (key, state tensors) of the last warm_start() from a fresh state

    def _hidden_for(self, B, device):
        """The carried state as the (1,B,H) tensor of its own that the inference kernels update in place."""
        return _initial_state(self.hidden, B, self.hidden_size, device, own=True).view(1, B, self.hidden_size)

    def _train_params(self):
        """The six parameters in GRUTrainStep's order (the bias-free head: b_o None)."""
        g, o = self.GRU, self.output
        return g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0, o.weight, o.bias

    def _one_launch(self):
        """Whether a loss entry forms its sums in the GRU's own C call (where the matrix-pipe kernel runs they ride in the
        recurrent launch): the product "auto" variant and no skip connection (y = GRU(x) + x sits between the two)."""
        return self.kernel_variant == "auto" and not self.skip

    def _launch(self, x2d, y2d, tbt=None, skip=0, R=None):
        """The GRU C call for a row-strided [B,T] fp32 input / output pair with unit stride along time; carries self.hidden
        (code/model.py:81-82).  With a target [B,T]: + the per-stream ESR sums (B,2) fp64 over samples [skip,T)
        (ntm_gru_forward_esr), with a pole R also the DCPreESR sums (ntm_gru_forward_losses); -> the tuple of those sums."""
        if self.input_size != 1 or self.output_size != 1:
            raise RuntimeError(f"input_size {self.input_size} / output_size {self.output_size}: the one-call entry points run the "
                               "single-channel kernels; use forward() plus the loss functions (esr_sums, esr_dcpre_sums)")
        B, T = x2d.shape
        _require_hip(self.GRU.weight_hh_l0, "model parameters (call .to('cuda'))")
        h = self._hidden_for(B, x2d.device)
        g, o, L = self.GRU, self.output, _lib.lib()
        args = (ptr(g.weight_ih_l0), ptr(g.weight_hh_l0), ptr(g.bias_ih_l0), ptr(g.bias_hh_l0), ptr(o.weight), ptr(o.bias),
                self.hidden_size, ptr(x2d), ptr(y2d), B, T, max(x2d.stride(0), T), max(y2d.stride(0), T), ptr(h))
        sums = tuple(torch.empty(B, 2, device=x2d.device, dtype=torch.float64)
                     for _ in range(0 if tbt is None else 1 if R is None else 2))
        if tbt is None:
            fn, err = _lib.gru_forward_fn(self.kernel_variant, self.hidden_size)
            _lib.check(fn(*args, _lib.VARIANTS[self.kernel_variant], _lib.current_stream()), "ntm_gru_forward", err)
        elif R is None:
            _lib.check(L.ntm_gru_forward_esr(*args, ptr(tbt), int(skip), ptr(sums[0]), _lib.current_stream()), "ntm_gru_forward_esr")
        else:
            _lib.check(L.ntm_gru_forward_losses(*args, ptr(tbt), int(skip), ptr(sums[0]), float(R), ptr(sums[1]),
                                                _lib.current_stream()), "ntm_gru_forward_losses")
        self.hidden = h
        return sums

    @torch.no_grad()
    def forward_into(self, x2d, y2d):
        """Stateful forward on ROW-STRIDED [B,Tc] fp32 views (unit stride along time), e.g. the time chunk
        `x[:, 0, c0:c1]` of a resident (B,1,T) batch, written into the matching view of the output -- the C ABI
        takes row strides, so a chunked / streamed predict needs no gather or scatter copies."""
        for t, what in ((x2d, "input"), (y2d, "output")):
            _require_hip(t, f"forward_into {what}")
            if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
                raise RuntimeError(f"forward_into: {what} must be a 2-D float32 view with unit stride along time")
        if x2d.shape != y2d.shape:
            raise RuntimeError("forward_into: shape mismatch")
        self._launch(x2d, y2d)
        if self.skip:
            y2d += x2d


class _Single:
    """A single RNN / DiffDelRNN as the group of one that epoch.train_epoch / validate walk: the model's OWN forward (the R = None
    nodes and entry points in training; `kernel_variant`, `skip`, any hidden size and the hand-over to the matrix-pipe kernel in
    validation), its own state, and `loss_fcn(pred, target)` itself."""

    def __init__(self, model):
        self.models, self.name, self.schedule = [model], type(model).__name__, model.schedule
        self.device = model.GRU.weight_hh_l0.device
        self.detach_hidden, self.zero_grad = model.detach_hidden, model.zero_grad

    def reset(self, Bper):
        m = self.models[0]
        if self.schedule.delays:
            m.initialize_hidden(Bper, m.max_delay)
        else:
            m.initialize_hidden()

    def stepper(self, train):
        m = self.models[0]          # its forward() takes the training or the inference form by grad mode and requires_grad
        return m.forward if self.schedule.delays else lambda x, d_traj, warmup: (m.forward(x), None)

    def grouped_loss(self, loss_fcn):
        return None


class RNN(_GRUHead):
    """GRU + fully connected output layer (reference: code/model.py:20-246)."""

    schedule = epoch.RNN_SCHEDULE

    def __init__(self, input_size=1, hidden_size=8, output_size=1, skip=False):
        super().__init__()
        self._init_net(input_size, hidden_size, output_size, skip, head_bias=True, general_io=True)
        self.initialize_hidden()

    def initialize_hidden(self):
        """Initialize GRU hidden state to zeros (code/model.py:50-52)."""
        self.hidden = None

    @property
    def _general_io(self):
        return self.input_size != 1 or self.output_size != 1

    def _forward_io(self, x):
        """forward() for input_size / output_size other than 1 (code/model.py:22,44-45,67-88; ntm_gru_forward_io): the reference
        reinterprets (B, C, T) as (B, T, C) with `reshape`, so the contiguous input row IS the [T][C] matrix the GRU reads and the
        [T][O] matrix the head writes IS the output row.  A plain kernel -- no caller of the reference uses these sizes."""
        if x.dim() != 3:
            raise RuntimeError(f"RNN.forward: expected (N_BATCHES, N_CHANNELS, N_SAMPLES), got {tuple(x.shape)}")
        B, C, T = x.shape
        I, O, H = self.input_size, self.output_size, self.hidden_size
        if C != I:          # torch.nn.GRU's own check on the reshaped input
            raise RuntimeError(f"input.size(-1) must be equal to input_size. Expected {I}, got {C}")
        _require_hip(x, "RNN.forward")
        _require_hip(self.GRU.weight_hh_l0, "model parameters (call .to('cuda'))")
        if self.skip and not (O == I or I == 1):    # y (B, T, O) += skip (B, T, C): only these shapes broadcast in place
            raise RuntimeError(f"The size of tensor a ({O}) must match the size of tensor b ({I}) at non-singleton dimension 2")
        xr = (x.float() if x.dtype != torch.float32 else x).contiguous().view(B, C * T)
        h = self._hidden_for(B, x.device)
        y = torch.empty(B, O * T, device=x.device, dtype=torch.float32)
        g, o = self.GRU, self.output
        rc = _lib.lib().ntm_gru_forward_io(ptr(g.weight_ih_l0), ptr(g.weight_hh_l0), ptr(g.bias_ih_l0), ptr(g.bias_hh_l0), ptr(o.weight),
                                           ptr(o.bias), H, I, O, ptr(xr), ptr(y), B, T, C * T, O * T, ptr(h), _lib.current_stream())
        _lib.check(rc, "ntm_gru_forward_io")
        self.hidden = h
        if self.skip:       # on the (B, T, .) views the reference adds in
            yv = y.view(B, T, O)
            yv += xr.view(B, T, I)
        return y.view(B, O, T)

    def warm_start(self):
        """Process 1024 samples of silence, B=1 (code/model.py:58-65).  From a fresh state (hidden None) the result
        depends on the parameters only and is kept per parameter version (module docstring)."""
        if self.input_size != 1:           # the reference feeds zeros((1, 1, 1024)) whatever input_size is: torch.nn.GRU raises
            raise RuntimeError(f"input.size(-1) must be equal to input_size. Expected {self.input_size}, got 1")
        fresh = self.hidden is None and self.warm_cache
        if fresh:
            key = self._warm_key()
            if self._warm is not None and self._warm[0] == key:
                self.hidden = self._warm[1].clone()
                return
        with torch.no_grad():
            x = torch.zeros((1, 1, START_LEN), device=self.GRU.weight_hh_l0.device)
            _ = self(x)
        if fresh:
            self._warm = (key, self.hidden.clone())

    def detach_hidden(self):
        """Detach the hidden state from the computational graph (code/model.py:54-56)."""
        self.hidden = self.hidden.clone().detach()

    def _check_trainable(self, what):
        """The configuration the training kernels cover (csrc/gru_train.hip), else a RuntimeError that names it."""
        if self.hidden_size != training.HIDDEN or self._general_io or self.skip:
            raise RuntimeError(f"{what}: training runs for {training.SUPPORTED} only; this model is RNN(input_size="
                               f"{self.input_size}, hidden_size={self.hidden_size}, output_size={self.output_size}, skip={self.skip})")
        _require_hip(self.GRU.weight_hh_l0, what)

    def forward(self, x):
        """x (N_BATCHES, N_CHANNELS = input_size, N_SAMPLES) -> y (N_BATCHES, output_size, N_SAMPLES); stateful
        (code/model.py:67-88).  input_size = output_size = 1 (every shipped checkpoint and caller) runs the kernels of DESIGN.md 0.
        With grad mode on and a parameter that requires grad (RNN.train_epoch) the call is a node of the autograd graph
        (training.GRUTrainStep: the low-latency kernel's step with its activations saved, same y bits) and self.hidden
        becomes its differentiable final state; otherwise nothing is recorded and the output does not require grad."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._forward_train(x)
        with torch.no_grad():
            return self._forward_infer(x)

    def _forward_train(self, x):
        self._check_trainable("RNN.forward")
        return _train_forward("RNN.forward", self, x, None, False, self._train_params(), None, None)[0]

    def _forward_infer(self, x):
        if self._general_io:
            return self._forward_io(x)
        xbt = _as_bt(x, "RNN.forward")
        y = torch.empty_like(xbt)
        self._launch(xbt, y)
        if self.skip:
            y += xbt
        return y.view(xbt.shape[0], 1, xbt.shape[1])

    @torch.no_grad()
    def forward_esr(self, x, target, skip=0):
        """forward(x) AND the per-stream ESR sums against `target` over samples [skip, T) -- `output = model(input)` followed
        by the ESR entry of the loss loop (code/test-model.py:346, :386-388) -- in one call: (y (N,1,T), sums (N,2) fp64 =
        [sum (t-y)^2, sum t^2]), the same numbers as `esr_sums(self(x), target, skip)` up to fp64 summation order.  With
        `kernel_variant == "auto"` and no skip connection it is ONE launch where the matrix-pipe kernel runs."""
        return self._forward_sums("RNN.forward_esr", x, target, skip, None)

    @torch.no_grad()
    def forward_losses(self, x, target, skip=0, R=None):
        """forward(x) AND both time-domain entries of the loss dict against `target` over samples [skip, T) -- `output =
        model(input)` followed by the ESR and DCPreESR losses (code/test-model.py:250-252,346,386-388) -- in one call:
        (y (N,1,T), ESR sums (N,2) fp64 = [sum (t-y)^2, sum t^2], DCPreESR sums (N,2) fp64 = the same of the DC-blocked
        signals): the numbers of `esr_sums` / `esr_dcpre_sums` on `self(x)` (ESR up to fp64 summation order, DCPreESR up to
        the fp32 evaluation order of the one-pole filter, ~1e-6 relative).  With `kernel_variant == "auto"` and no skip
        connection it is ONE launch where the matrix-pipe kernel runs."""
        return self._forward_sums("RNN.forward_losses", x, target, skip, DC_PRE_R if R is None else R)

    def _forward_sums(self, what, x, target, skip, R):
        """forward_losses; R None: without the DCPreESR sums (forward_esr)."""
        xbt = _as_bt(x, what)
        tbt = _as_bt(target, what)
        if tbt.shape != xbt.shape:
            raise RuntimeError(f"shape mismatch: x {tuple(x.shape)} vs target {tuple(target.shape)}")
        y = torch.empty_like(xbt)
        y3 = y.view(xbt.shape[0], 1, xbt.shape[1])
        if self._one_launch():
            return (y3,) + self._launch(xbt, y, tbt, skip, R)
        self._launch(xbt, y)
        if self.skip:
            y += xbt
        return (y3, esr_sums(y3, target, skip)) + (() if R is None else (esr_dcpre_sums(y3, target, skip, R),))

    def _predict_start(self, B):
        """The prologue of every predict: initialize_hidden, warm_start, the warm state broadcast to B streams."""
        self.initialize_hidden()
        self.warm_start()
        if B != 1:
            self.hidden = self.hidden.expand(1, B, self.hidden_size).contiguous()

    @torch.no_grad()
    def predict_esr(self, input, target, skip=0):
        """predict(input) + the ESR sums against `target` over [skip, T): initialize_hidden, warm_start, forward_esr."""
        self._predict_start(input.shape[0])
        return self.forward_esr(input, target, skip)

    @torch.no_grad()
    def predict_losses(self, input, target, skip=0, R=None):
        """predict(input) + the ESR and DCPreESR sums against `target` over [skip, T)."""
        self._predict_start(input.shape[0])
        return self.forward_losses(input, target, skip, R)

    @torch.no_grad()
    def predict(self, input, segment_length=None):
        """initialize_hidden + warm_start + forward over the sequence (code/model.py:218-246)."""
        self._predict_start(input.shape[0])
        return epoch.in_segments(lambda sl: (self.forward(input[:, :, sl]),), input, segment_length)[0]

    def train_epoch(self, dataloader, loss_fcn, optimizer):
        """One epoch of truncated back-propagation through time (code/model.py:90-161, run by code/train.py): per batch the
        hidden state is reset, aggregated on the first 1024 samples, then every whole window of 1024 samples is predicted,
        scored with `loss_fcn(pred, target)`, back-propagated and followed by `optimizer.step()`; returns the mean over batches
        of the mean window loss.  As in the reference the warm-up forward runs with grad enabled and is not detached, so the
        first window's backward reaches through it (2048 samples); detach_hidden cuts the graph after every window.
        `dataloader`: any iterable of batches whose first two items are input and target (B, C, T) -- `(x, t, meta)` as the
        reference's DataLoader gives, or SegmentFeeder.batches; only channel 0 is used.  `loss_fcn`: ESRLoss / DCPreESR (or
        any function of (pred, target) that is differentiable through torch); `optimizer`: any torch.optim optimizer over
        model.parameters().
        Supported: RNN(1, 64, 1, skip=False) on a HIP device (RuntimeError otherwise).  On entry it sets requires_grad on the
        GRU and head parameters (they are created without it, so that inference never records a graph).  The loop is
        epoch.train_epoch, the lengths epoch.RNN_SCHEDULE."""
        return epoch.train_epoch(_Single(self), [dataloader], loss_fcn, optimizer)[0]

    def validate(self, dataloader, loss_fcn, store_examples=True):
        """Loss over a validation set (code/model.py:163-216; called by code/train.py:242): per batch the hidden state
        is aggregated on the first 1024 REAL samples, the rest is predicted in one launch and scored with
        `loss_fcn(pred, target)`; returns (mean loss over batches, examples).  `dataloader`: anything with len() that
        yields (input, target, meta) batches of shape (B, C, T); only channel 0 is used, as in the reference.  The loop is
        epoch.validate, the lengths epoch.RNN_SCHEDULE."""
        return epoch.validate(_Single(self), [dataloader], loss_fcn, store_examples)[0]


class TimeVaryingDelayLine(torch.nn.Module):
    """Time-varying feed-forward delay line, linear interpolation (reference: code/model.py:249-332).

    The reference asserts `max_delay >= max(dt)` at the top of forward() (code/model.py:284).  Here the range check
    rides along in the kernel that reads dt anyway and raises a device-side flag; the carried buffer is never
    modified by a violating call (nor by any later one until the flag is cleared), exactly the state the reference
    is left in when its assert fires.  forward() by default looks at the flag before it returns, so a direct call
    raises AssertionError where the reference does (one host synchronisation, as `torch.max(dt)` in the reference's
    assert is).  Callers that stream many chunks set `defer_check = True` (DiffDelRNN.predict, the feeder's
    streamed predict, BlockStreamer-style loops do): no host synchronisation per call, `raise_if_violated()` once at
    the end."""

    def __init__(self, max_delay=40000, channels=1):
        super().__init__()
        if channels != 1:
            raise ValueError("only 1 channel is built (reference default, code/model.py:251)")
        self.max_delay = max_delay
        # like the reference, batch 2 until init_buffer() is called (code/model.py:267)
        self.buffer = torch.zeros(2, channels, max_delay)
        self._err = None
        self._unchecked = False      # deferred launches since the flag was last looked at
        self._fresh = False
        self.defer_check = False

    def init_buffer(self, N, max_d):
        """Zero buffer for mini-batch size N; overwrites max_delay (code/model.py:326-332)."""
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if self._unchecked:
            # deferred forward() calls whose range check nobody has looked at yet: a violation among them must not
            # vanish with the state it froze -- the reference would have raised at that call (code/model.py:284)
            self.raise_if_violated()
        self.max_delay = max_d
        self.buffer = torch.zeros(N, 1, self.max_delay).to(device)
        self._fresh = True           # all zeros, untouched since (DiffDelRNN.warm_start's cache looks at it)
        if self._err is not None:
            self._err.zero_()

    def detach_buffer(self):
        """Detach the buffer from the computational graph (code/model.py:322-324): a clone here."""
        self.buffer = self.buffer.clone().detach()

    def raise_if_violated(self):
        """The reference's `assert self.max_delay >= torch.max(dt)` for every forward() since the last check
        (one host synchronisation).  The buffer holds the state before the first violating call."""
        self._unchecked = False
        if self._err is not None and int(self._err.item()) != 0:
            self._err.zero_()
            raise AssertionError("max_delay >= max(dt) violated")

    def _prepare(self, B, device):
        """Before every launch for batch B on `device`: the buffer is (B,1,max_delay), fp32, contiguous and there, and so is
        the violation flag; the buffer no longer counts as fresh.  -> max_delay as an int."""
        D = int(self.max_delay)
        if self.buffer.shape[0] != B or self.buffer.shape[2] != D:
            raise RuntimeError(f"Sizes of tensors must match: buffer {list(self.buffer.shape)} vs input batch {B}")
        if self.buffer.device != device or self.buffer.dtype != torch.float32 or not self.buffer.is_contiguous():
            self.buffer = self.buffer.to(device=device, dtype=torch.float32).contiguous()
        if self._err is None or self._err.device != device:
            self._err = torch.zeros(1, device=device, dtype=torch.int32)
        self._fresh = False
        return D

    def _launched(self):
        """After every launch: look at the violation flag now, or note that a deferred launch is waiting for that."""
        if not self.defer_check:
            self.raise_if_violated()
        else:
            self._unchecked = True

    @contextlib.contextmanager
    def deferred(self):
        """Inside: no launch looks at the violation flag (no host synchronisation per chunk).  On a clean exit the assert of
        code/model.py:284 is evaluated ONCE for all of them, unless the caller had deferred it already."""
        before, self.defer_check = self.defer_check, True
        try:
            yield
        finally:
            self.defer_check = before
        if not before:
            self.raise_if_violated()

    def _run(self, xbt, dbt, warmup):
        """[B,T] fp32 -> y [B,T]; the carried buffer is updated IN PLACE (no clone, no scratch, no host sync)."""
        B, T = xbt.shape
        D = self._prepare(B, xbt.device)
        y = torch.empty_like(xbt)
        rc = _lib.lib().ntm_delay_forward(ptr(xbt), ptr(dbt), ptr(y), B, T, ptr(self.buffer), D, int(bool(warmup)),
                                          ptr(self._err), _lib.current_stream())
        _lib.check(rc, "ntm_delay_forward")
        self._launched()
        return y

    def _run_f64(self, xbt, d64, warmup):
        """_run with the delays in float64 [B,T] (ntm_delay_forward_f64): the weights and products in float64, as the reference
        forms them from a float64 trajectory."""
        B, T = xbt.shape
        D = self._prepare(B, xbt.device)
        y = torch.empty_like(xbt)
        rc = _lib.lib().ntm_delay_forward_f64(ptr(xbt), ptr(d64), ptr(y), B, T, ptr(self.buffer), D, int(bool(warmup)),
                                              ptr(self._err), _lib.current_stream())
        _lib.check(rc, "ntm_delay_forward_f64")
        self._launched()
        return y

    @torch.no_grad()
    def forward(self, x, dt, warmup=False):
        """x, dt (N,1,T), dt in samples -> y (N,1,T) (code/model.py:269-320)."""
        xbt = _as_bt(x, "TimeVaryingDelayLine.forward")
        dbt = _as_bt(dt, "TimeVaryingDelayLine.forward")
        if dbt.shape != xbt.shape:
            raise RuntimeError(f"shape mismatch: x {tuple(x.shape)} vs dt {tuple(dt.shape)}")
        return self._run(xbt, dbt, warmup).view(xbt.shape[0], 1, xbt.shape[1])


class DiffDelRNN(_GRUHead):
    """RNN (bias-free head) + differentiable delay line (reference: code/model.py:335-653)."""

    schedule = epoch.DIFFDEL_SCHEDULE

    def __init__(self, input_size=1, hidden_size=8, output_size=1, skip=False, max_delay=10000):
        super().__init__()
        self._init_net(input_size, hidden_size, output_size, skip, head_bias=False)
        self.max_delay = max_delay
        self.diffdel = TimeVaryingDelayLine(max_delay=max_delay)
        self.initialize_hidden(2, max_delay)     # as the reference does (code/model.py:370)

    def initialize_hidden(self, N, max_D):
        """hidden <- None; delay buffer <- zeros(N,1,int(max_D)+1) (code/model.py:372-375)."""
        self.hidden = None
        self.diffdel.init_buffer(N, int(max_D) + 1)

    def warm_start(self):
        """1024 samples of silence with zero delay, B=1 (code/model.py:382-391).  From a fresh state (hidden None,
        zero buffer of batch 1) the result -- hidden state and delay buffer -- depends on the parameters and the
        delay-line length only and is kept per parameter version (module docstring)."""
        dev =self.GRU.weight_hh_l0.device
        dl = self.diffdel
        fresh = (self.warm_cache and self.hidden is None and dl._fresh and dl.buffer.shape[0] == 1
                 and dl.buffer.device == dev)
        if fresh:
            key = self._warm_key(int(dl.max_delay), self.delay_mode)     # fused / two-pass warm-ups run different GRU kernels at B = 1
            if self._warm is not None and self._warm[0] == key:
                self.hidden = self._warm[1].clone()
                dl.buffer = self._warm[2].clone()
                dl._fresh = False
                return
        with torch.no_grad():
            x = torch.zeros((1, 1, START_LEN), device=dev)
            d_traj = torch.zeros((1, 1, START_LEN), device=dev)
            _, __ = self(x, d_traj)
        if fresh:
            self._warm = (key, self.hidden.clone(), dl.buffer.clone())

    def detach_hidden(self):
        """Detach hidden state and delay buffer from the computational graph (code/model.py:377-380): clones here."""
        self.hidden = self.hidden.clone().detach()
        self.diffdel.detach_buffer()

    # "auto": ONE launch for the whole step where the matrix-pipe kernel runs (the delay line fused into the GRU
    # kernel's output flush, include/ntm.h ntm_diffdel_gru_forward), GRU launch + streaming delay pass elsewhere;
    # "two_pass" / "fused" force either form (A/B measurements, tests).  A laboratory or explicitly chosen GRU kernel
    # (`kernel_variant` other than "auto") and `skip=True` (pre_d = GRU(x) + x sits between the two) take the two calls.
    delay_mode = "auto"

    def _one_launch(self, losses=True):
        """Whether a call takes the one-C-call step: forward() unless `delay_mode` is "two_pass", the loss entries (whose
        C entry points run the "auto" mode) only under "auto"."""
        return super()._one_launch() and (self.delay_mode == "auto" if losses else self.delay_mode != "two_pass")

    def forward(self, x, del_traj, warmup=False, _events=None):
        """(x, del_traj) (N,1,T) -> (y, pre_d) (code/model.py:393-424).  With grad mode on and a parameter that requires grad
        (DiffDelRNN.train_epoch) the call is two nodes of the autograd graph: training.GRUTrainStep (the low-latency kernel's
        step, no head bias) and training.DelayLineStep; y, pre_d, self.hidden and the delay buffer are then in the graph, with
        the bits of kernel_variant "lat" / delay_mode "two_pass".  Otherwise nothing is recorded."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._forward_train(x, del_traj, warmup)
        with torch.no_grad():
            return self._forward_infer(x, del_traj, warmup, _events)

    def _check_trainable(self, what):
        """The configuration the training kernels cover, else a RuntimeError that names it."""
        if self.hidden_size != training.HIDDEN or self.skip:
            raise RuntimeError(f"{what}: training runs for {training.SUPPORTED_DIFFDEL} only; this model is DiffDelRNN(input_size="
                               f"{self.input_size}, hidden_size={self.hidden_size}, output_size={self.output_size}, skip={self.skip})")
        dev = self.GRU.weight_hh_l0.device
        if not self.GRU.weight_hh_l0.is_cuda:
            raise RuntimeError(f"{what}: DiffDelRNN training is not implemented for parameters on '{dev}': it runs on a HIP "
                               f"device only ({training.SUPPORTED_DIFFDEL})")

    def _forward_train(self, x, del_traj, warmup):
        self._check_trainable("DiffDelRNN.forward")
        return _train_forward("DiffDelRNN.forward", self, x, del_traj, warmup, self._train_params(), None, self.diffdel)

    def _forward_infer(self, x, del_traj, warmup=False, _events=None):
        """(x, del_traj) (N,1,T) -> (y, pre_d) (code/model.py:393-424).  `_events`: three torch.cuda.Event objects
        recorded before the GRU launch, between it and the delay pass, and after (bench.py's per-kernel timing; with the
        fused step the middle one is recorded right behind the fused launch, ahead of the buffer update)."""
        xbt, dbt = _bt_pair("DiffDelRNN.forward", x, del_traj)
        B, T = xbt.shape
        if self._one_launch(losses=False):
            y, pre = self._fused_step(xbt, dbt, warmup, _events)
            return y.view(B, 1, T), pre.view(B, 1, T)
        if _events:
            _events[0].record()
        pre = torch.empty_like(xbt)
        self._launch(xbt, pre)
        if self.skip:
            pre += xbt
        if _events:
            _events[1].record()
        y = self.diffdel._run(pre, dbt, warmup)
        if _events:
            _events[2].record()
        return y.view(B, 1, T), pre.view(B, 1, T)

    @torch.no_grad()
    def forward_f64_delays(self, x, del_traj, warmup=False):
        """forward(x, del_traj) without grad for a FLOAT64 delay trajectory (N,1,T) in samples, kept in float64 down to the
        interpolation weights (forward() rounds the delays to float32 first, which at several hundred samples of delay moves a
        noise-like output by 1e-5): the GRU launch of forward(), then ntm_delay_forward_f64.  -> (y, pre_d) float32; pre_d and
        the hidden state are forward()'s bits, the state is carried the same way.  What the reference computes when its data
        set hands float64 trajectories (the validation pass of code/train-adversarial.py)."""
        xbt = _as_bt(x, "DiffDelRNN.forward_f64_delays")
        if del_traj.dim() != 3 or del_traj.shape[1] != 1 or del_traj.dtype != torch.float64:
            raise RuntimeError(f"DiffDelRNN.forward_f64_delays: a float64 (N, 1, T) delay trajectory, got {tuple(del_traj.shape)} {del_traj.dtype}")
        _require_hip(del_traj, "DiffDelRNN.forward_f64_delays")
        d64 = del_traj.contiguous().view(del_traj.shape[0], del_traj.shape[2])
        if d64.shape != xbt.shape:
            raise RuntimeError(f"shape mismatch: x {tuple(x.shape)} vs del_traj {tuple(del_traj.shape)}")
        B, T = xbt.shape
        pre = torch.empty_like(xbt)
        self._launch(xbt, pre)
        if self.skip:
            pre += xbt
        y = self.diffdel._run_f64(pre, d64, warmup)
        return y.view(B, 1, T), pre.view(B, 1, T)

    @torch.no_grad()
    def forward_esr(self, x, del_traj, target, skip=0):
        """forward(x, del_traj) AND the per-stream ESR sums of the delayed output against `target` over samples [skip, T)
        (`model(input, d_traj)` followed by the ESR entry of the loss loop, code/test-model.py:353, :386-388) in one call:
        (y, pre_d, sums (N,2) fp64).  ONE launch where the fused step runs (`delay_mode` / `kernel_variant` "auto", no skip
        connection): the sums are accumulated in the fused delay stage; otherwise forward() + esr_sums()."""
        return self._forward_sums("DiffDelRNN.forward_esr", x, del_traj, target, skip, None)

    @torch.no_grad()
    def forward_losses(self, x, del_traj, target, skip=0, R=None):
        """forward(x, del_traj) AND both time-domain entries of the loss dict for the delayed output against `target` over
        samples [skip, T) (code/test-model.py:250-252,353,386-388) in one call: (y, pre_d, ESR sums (N,2) fp64, DCPreESR sums
        (N,2) fp64).  ONE launch where the fused step runs (`delay_mode` / `kernel_variant` "auto", no skip connection); otherwise
        forward() + the two streaming passes."""
        return self._forward_sums("DiffDelRNN.forward_losses", x, del_traj, target, skip, DC_PRE_R if R is None else R)

    def _forward_sums(self, what, x, del_traj, target, skip, R):
        """forward_losses; R None: without the DCPreESR sums (forward_esr)."""
        xbt = _as_bt(x, what)
        dbt = _as_bt(del_traj, what)
        tbt = _as_bt(target, what)
        if dbt.shape != xbt.shape or tbt.shape != xbt.shape:
            raise RuntimeError(f"shape mismatch: x {tuple(x.shape)} vs del_traj {tuple(del_traj.shape)} vs target {tuple(target.shape)}")
        if not self._one_launch():
            y, pre = self.forward(x, del_traj)
            return (y, pre, esr_sums(y, target, skip)) + (() if R is None else (esr_dcpre_sums(y, target, skip, R),))
        B, T = xbt.shape
        y, pre, *sums = self._fused_step(xbt, dbt, False, None, tbt, int(skip), R)
        return (y.view(B, 1, T), pre.view(B, 1, T), *sums)

    def _predict_start(self, B):
        """The prologue of every predict: initialize_hidden, warm_start, the warm state and delay buffer broadcast to B streams."""
        self.initialize_hidden(1, self.max_delay)
        self.warm_start()
        if B != 1:
            self.hidden = self.hidden.expand(1, B, self.hidden_size).contiguous()
            self.diffdel.buffer = self.diffdel.buffer.expand(B, 1, -1).contiguous()

    def _predict_with(self, fn, input):
        """_predict_start, then fn() with the delay-range assert of code/model.py:284 evaluated ONCE, after the last launch
        has been enqueued (no host synchronisation per chunk)."""
        self._predict_start(input.shape[0])
        with self.diffdel.deferred():
            out = fn()
        return out

    @torch.no_grad()
    def predict_esr(self, input, d_traj, target, skip=0):
        """predict(input, d_traj) + the ESR sums of the output against `target` over [skip, T)."""
        return self._predict_with(lambda: self.forward_esr(input, d_traj, target, skip), input)

    @torch.no_grad()
    def predict_losses(self, input, d_traj, target, skip=0, R=None):
        """predict(input, d_traj) + the ESR and DCPreESR sums of the output against `target` over [skip, T)."""
        return self._predict_with(lambda: self.forward_losses(input, d_traj, target, skip, R), input)

    def _fused_step(self, xbt, dbt, warmup, _events=None, tbt=None, skip=0, dcp_R=None):
        """One C-ABI call for GRU + head + delay line (ntm_diffdel_gru_forward_ex); carries self.hidden and the delay
        buffer exactly as the two calls do.  With a target: + the ESR sums (ntm_diffdel_gru_forward_esr), with `dcp_R` also
        the DCPreESR sums (ntm_diffdel_gru_forward_losses) of the delayed output.  -> (y, pre_d, *sums)."""
        B, T = xbt.shape
        dl = self.diffdel
        _require_hip(self.GRU.weight_hh_l0, "model parameters (call .to('cuda'))")
        D = dl._prepare(B, xbt.device)
        h = self._hidden_for(B, xbt.device)
        y, pre = torch.empty_like(xbt), torch.empty_like(xbt)
        sums = tuple(torch.empty(B, 2, device=xbt.device, dtype=torch.float64)
                     for _ in range(0 if tbt is None else 1 if dcp_R is None else 2))
        g, L = self.GRU, _lib.lib()
        args = (ptr(g.weight_ih_l0), ptr(g.weight_hh_l0), ptr(g.bias_ih_l0), ptr(g.bias_hh_l0), ptr(self.output.weight),
                self.hidden_size, ptr(xbt), ptr(dbt), ptr(y), ptr(pre), B, T, ptr(h), ptr(dl.buffer), D)
        if _events:
            _events[0].record()
        if tbt is None:
            rc = L.ntm_diffdel_gru_forward_ex(*args, int(bool(warmup)), ptr(dl._err), _lib.DIFFDEL_MODES[self.delay_mode],
                                              _lib.current_stream())
        elif dcp_R is None:
            rc = L.ntm_diffdel_gru_forward_esr(*args, ptr(dl._err), ptr(tbt), int(skip), ptr(sums[0]), _lib.current_stream())
        else:
            rc = L.ntm_diffdel_gru_forward_losses(*args, ptr(dl._err), ptr(tbt), int(skip), ptr(sums[0]), float(dcp_R), ptr(sums[1]),
                                                  _lib.current_stream())
        _lib.check(rc, "ntm_diffdel_gru_forward")
        if _events:
            _events[1].record()
            _events[2].record()
        self.hidden = h
        dl._launched()
        return (y, pre) + sums

    @torch.no_grad()
    def predict(self, input, d_traj, segment_length=None, _events=None):
        """initialize_hidden + warm_start + forward (code/model.py:618-653); any batch size.  The delay-range assert
        of code/model.py:284 is evaluated ONCE, after the last chunk has been enqueued (no host synchronisation
        per chunk)."""
        events = _events if segment_length is None else None
        return self._predict_with(lambda: epoch.in_segments(
            lambda sl: self.forward(input[:, :, sl], d_traj[:, :, sl], _events=events), input, segment_length, 2), input)

    def train_epoch(self, dataloader, loss_fcn, optimizer, dataset=None):
        """One epoch of truncated back-propagation through time (code/model.py:426-511, run by code/train.py --MODEL DiffDelGRU):
        per batch the state is reset (zero delay buffer of max_delay + 1 samples), aggregated with grad enabled on the first
        TBPTT_INIT = nextpow2(int(analyser max_delay * fs)) samples (`warmup=True`: the delay line only fills its buffer), then
        every whole window of 2048 samples is predicted, scored with `loss_fcn(pred, target)`, back-propagated and followed by
        `optimizer.step()`; returns the mean over batches of the mean window loss.  As in the reference the warm-up is not
        detached: the first window's backward reaches it through the hidden state and through the delay taps that read the
        buffer.  `dataset` (default `dataloader.dataset`): `fs` and `delay_analyzer.max_delay` (the reference's dataset) or
        `max_delay` (SegmentFeeder), in seconds.  `dataloader`: the reference's (x, t, meta) batches with
        meta['delay_trajectory'] (B, T) in seconds, or SegmentFeeder.batches' (x, t, d_seconds (B,1,T), metas).  The delays are
        the fp32 product d_seconds * fs, as the reference forms them.
        Supported: DiffDelRNN(1, 64, 1, skip=False) on a HIP device (RuntimeError otherwise).  On entry it sets requires_grad on
        the GRU and head parameters.  The loop is epoch.train_epoch, the lengths epoch.DIFFDEL_SCHEDULE."""
        return epoch.train_epoch(_Single(self), [dataloader], loss_fcn, optimizer, dataset=dataset)[0]

    def validate(self, dataloader, loss_fcn, store_examples=True):
        """Loss over a validation set (code/model.py:513-616): INIT_LEN = nextpow2(int(analyser max_delay * fs)); per
        batch the state is aggregated on the first INIT_LEN real samples (`warmup=True`: the delay line only fills its
        buffer), then the rest is predicted and `loss_fcn` is evaluated on 2048-sample pieces whose mean is the batch's
        loss -- the reference forwards those pieces one by one; here they come out of ONE launch (chunked == one-shot
        bit for bit, state carried either way) and only the loss loop runs per piece.  Needs of the dataloader what the
        reference needs: len(), (input, target, meta) batches with meta['delay_trajectory'] (B, T) in seconds,
        `.dataset.delay_analyzer.max_delay` (seconds) and `.dataset.fs`.  The loop is epoch.validate, the lengths
        epoch.DIFFDEL_SCHEDULE."""
        return epoch.validate(_Single(self), [dataloader], loss_fcn, store_examples)[0]


class Replicas:
    """R independent models of one supported training configuration -- R `RNN(1, 64, 1)` or R `DiffDelRNN(1, 64, 1)`, no skip
    connection, all on the same HIP device -- trained side by side: what the reference runs as an array of jobs
    (scripts/sbatch-train-exp1a.sh:7-15, --array=0-2, each at code/train.py:94's batch of 32, i.e. 32 of 256 CUs).  Per TBPTT
    window there is ONE forward launch, ONE BPTT launch, ONE gradient reduction and ONE launch per loss kernel for all R; the
    streams are stacked replica-major (training.GRUTrainStep with R).  Every replica ends up bit-identical to the same model
    trained alone by its own train_epoch: everything on the path is per stream and free of atomics.
    The models stay ordinary modules with their own parameters (the [R, ...] stacks are built inside the graph by torch.stack, so
    autograd hands each model its own .grad): each state_dict() is the reference's checkpoint format, and each can validate()
    or predict() on its own afterwards.  After every window each model's `hidden` (and delay buffer) is its slice of the group's.
    The other half of the epoch loop (code/train.py:238-267) is grouped as well: infer() / validate() / predict() run all R models
    in one launch of the low-latency kernel (ntm_gru_forward_replicas) and give every replica the bits of its own
    validate() / predict().
    Out of scope: replicas of different architectures, per-replica batch sizes, skip=True and hidden sizes other than 64 (the
    single models refuse to train there too), several devices."""

    def __init__(self, models):
        models = list(models)
        if not models:
            raise ValueError("Replicas: at least one model")
        kinds = {type(m) for m in models}
        if kinds != {RNN} and kinds != {DiffDelRNN}:
            raise TypeError("Replicas: all models must be RNN or all DiffDelRNN, got " + ", ".join(sorted(k.__name__ for k in kinds)))
        if len({id(m) for m in models}) != len(models):
            raise ValueError("Replicas: the same module appears twice; every replica needs a model of its own")
        ps = [p for m in models for p in m.parameters()]
        if len({id(p) for p in ps}) != len(ps):
            raise ValueError("Replicas: the same parameter appears twice; every replica needs parameters of its own")
        for m in models:
            m._check_trainable("Replicas")
        devs = {m.GRU.weight_hh_l0.device for m in models}
        if len(devs) != 1:
            raise ValueError(f"Replicas: all models must be on one device, got {sorted(map(str, devs))}")
        self.models = models
        self.name, self.schedule = "Replicas", models[0].schedule      # a group for epoch.train_epoch / validate as it stands
        self.diffdel = self.schedule.delays
        self.device = devs.pop()
        self.hidden = None                               # (1, R*Bper, 64) replica-major, in the graph between detach_hidden() calls
        self._dl = TimeVaryingDelayLine(max_delay=models[0].max_delay) if self.diffdel else None

    def __len__(self):
        return len(self.models)

    def _stacks(self):
        """The six parameters as [R, ...] stacks, nodes of the graph (the bias-free head: b_o None)."""
        return tuple(None if ps[0] is None else torch.stack(ps) for ps in zip(*(m._train_params() for m in self.models)))

    def initialize_hidden(self, Bper=None):
        """Every replica's initialize_hidden: hidden <- None, for DiffDelRNN also a zero delay buffer of max_delay + 1 samples for
        `Bper` streams per replica."""
        self.hidden = None
        for m in self.models:
            m.hidden = None
        if self.diffdel:
            D = {int(m.max_delay) for m in self.models}
            if len(D) != 1:
                raise ValueError(f"Replicas: the models' max_delay differ ({sorted(D)}); one delay-buffer length is needed")
            self._dl.init_buffer(len(self.models) * int(Bper), D.pop() + 1)
            self._share()

    def _share(self):
        """Each model's state <- its slice of the group's (views)."""
        R = len(self.models)
        h = self.hidden
        for r, m in enumerate(self.models):
            if h is not None:
                n = h.shape[1] // R
                m.hidden = h[:, r * n:(r + 1) * n]
            if self.diffdel:
                n = self._dl.buffer.shape[0] // R
                m.diffdel.max_delay = self._dl.max_delay
                m.diffdel.buffer = self._dl.buffer[r * n:(r + 1) * n]
                m.diffdel._fresh = False

    def detach_hidden(self):
        """Every replica's detach_hidden (one clone for all)."""
        self.hidden = self.hidden.clone().detach()
        if self.diffdel:
            self._dl.detach_buffer()
        self._share()

    def zero_grad(self):
        for m in self.models:
            m.zero_grad()

    def forward(self, x, del_traj=None, warmup=False, _share=True):
        """One stateful training forward of all replicas: x (and del_traj, in samples) (R*Bper, 1, T) replica-major -> y for RNN,
        (y, pre_d) for DiffDelRNN, as the models' own forward() gives on their slices (same bits), as graph nodes.  A delay above
        the buffer in ANY replica raises AssertionError with every replica's delay buffer as it was."""
        out = _train_forward("Replicas.forward", self, x, del_traj, warmup, self._stacks(), len(self.models), self._dl)
        if _share:
            self._share()
        return out if self.diffdel else out[0]

    __call__ = forward

    # ---- the group as epoch.train_epoch / validate see it (beside models, name, device, schedule, detach_hidden, zero_grad)
    reset = initialize_hidden

    def stepper(self, train):
        """(x, d_traj or None, warmup) -> (pred, pre_d or None): forward() (the models' views of the state are refreshed by
        detach_hidden() after every window), or infer() with the parameter stacks built once."""
        if train:
            run = lambda x, d_traj, warmup: self.forward(x, d_traj, warmup, _share=False)  # noqa: E731
        else:
            stacks = self._infer_stacks()
            run = lambda x, d_traj, warmup: self.infer(x, d_traj, warmup, _stacks=stacks)  # noqa: E731
        return run if self.diffdel else lambda x, d_traj, warmup: (run(x, d_traj, warmup), None)

    def grouped_loss(self, loss_fcn):
        """ESRLoss / DCPreESR: all R losses from one launch per kernel; any other callable: None (it is applied per replica)."""
        if isinstance(loss_fcn, (ESRLoss, DCPreESR)):
            return lambda pred, target: loss_fcn.replicas(pred, target, len(self.models))
        return None

    def train_epoch(self, dataloaders, loss_fcn, optimizers, dataset=None, losses_hook=None):
        """One epoch of every replica's train_epoch (RNN: code/model.py:90-161, TBPTT_INIT = TBPTT_LEN = 1024; DiffDelRNN:
        code/model.py:426-511, the analyser's nextpow2 warm-up, windows of 2048, the fp32 d * fs product, the `//` window count)
        in lock step; -> the list of R epoch losses.  Per replica the loop is statement for statement that of its own
        train_epoch (it is the same loop, epoch.train_epoch): warm-up forward in the graph, zero_grad, then per window forward,
        loss, backward (of the sum of the R losses: they share no node, so each model receives its own gradient), every
        optimizer's step(), detach_hidden, zero_grad.
        `dataloaders`: a list / tuple of R loaders (zipped; the epoch ends with the shortest), or ONE loader whose batches every
        replica sees.  In every iteration the R batches must have the same shape (ValueError otherwise).
        `optimizers`: a list / tuple of optimizers (e.g. one per replica), or one optimizer over every replica's parameters;
        only step() is called on each.
        `loss_fcn`: an ESRLoss or DCPreESR instance is evaluated for all replicas at once (one launch per kernel, one host
        synchronisation per window); any other callable of (pred, target) is applied to each replica's slice in turn.
        `dataset` (DiffDelRNN; one or a list of R; default each loader's .dataset): as DiffDelRNN.train_epoch's; all must give
        the same warm-up length, and the models the same max_delay.
        `losses_hook(list of R floats)` is called once per window with the window's losses, in replica order."""
        return epoch.train_epoch(self, dataloaders, loss_fcn, optimizers, dataset, losses_hook)

    # ---- inference of the group: one launch of the low-latency kernel for all R models

    @staticmethod
    def _streams_per_replica(B, R, what):
        """Bper of B replica-major streams, or the ValueError that names both numbers."""
        if R < 1 or B % R:
            raise ValueError(f"{what}: {B} streams do not divide into {R} replicas")
        return B // R

    @torch.no_grad()
    def _infer_stacks(self):
        """The six [R, ...] parameter stacks as plain tensors (no graph, whatever requires_grad says)."""
        return tuple(None if t is None else t.detach().contiguous() for t in self._stacks())

    @torch.no_grad()
    def infer(self, x, del_traj=None, warmup=False, _stacks=None):
        """The stateful inference forward of all replicas in ONE GRU launch: x (and del_traj, in samples) (R*Bper, 1, T)
        replica-major -> y for RNN replicas, (y, pre_d) for DiffDelRNN replicas; carries the group's `hidden` (and delay buffer)
        and refreshes each model's views of them.  Nothing is recorded, whatever requires_grad says (it works straight after
        train_epoch), and the outputs do not require grad.
        Grouped inference ALWAYS runs the low-latency kernel (ntm_gru_forward_replicas: a workgroup per stream, each reading its
        replica's slice of the parameter stacks), for any R * Bper; DiffDelRNN replicas follow it with the streaming delay pass on
        all R * Bper streams (the delay line has no parameters).  Every replica's result is bit-identical to the same model's own
        forward() on its slice with `kernel_variant = "lat"` (and `delay_mode = "two_pass"`) -- which is what the default "auto"
        runs up to NTM_GRU_LAT_MAX_B = 1024 streams per model (csrc/ntm_api.hip, mfma2_streams); above that a single model's
        "auto" hands over to the matrix-pipe kernel (another summation order) and this entry does not.
        A delay above the buffer in ANY replica raises AssertionError with every replica's delay buffer as it was (one range
        flag for the group; the hidden state has moved on by then, as in the single model)."""
        R = len(self.models)
        H = training.HIDDEN
        xbt, dbt = _bt_pair("Replicas.infer", x, del_traj, self.diffdel)
        B, T = xbt.shape
        Bper = self._streams_per_replica(B, R, "Replicas.infer")
        _require_hip(self.models[0].GRU.weight_hh_l0, "model parameters (call .to('cuda'))")
        h = _initial_state(self.hidden, B, H, xbt.device, own=True)
        w_ih, w_hh, b_ih, b_hh, w_o, b_o = self._infer_stacks() if _stacks is None else _stacks
        pre = torch.empty_like(xbt)
        rc = _lib.lib().ntm_gru_forward_replicas(ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(w_o), ptr(b_o), ptr(xbt), ptr(pre),
                                                 R, Bper, T, max(xbt.stride(0), T), max(pre.stride(0), T), ptr(h), _lib.current_stream())
        _lib.check(rc, "ntm_gru_forward_replicas")
        self.hidden = h.view(1, B, H)
        if not self.diffdel:
            self._share()
            return pre.view(B, 1, T)
        try:
            y = self._dl._run(pre, dbt, warmup)          # raises BEFORE any buffer moves on (or defers, as predict() asks)
        finally:
            self._share()
        return y.view(B, 1, T), pre.view(B, 1, T)

    def validate(self, dataloaders, loss_fcn, store_examples=True):
        """Every replica's validate() (RNN: code/model.py:163-216, INIT_LEN = 1024, one loss per batch; DiffDelRNN:
        code/model.py:513-616, INIT_LEN = the analyser's nextpow2 warm-up run with `warmup=True`, the loss on 2048-sample pieces,
        the mean over pieces, ZeroDivisionError for T <= INIT_LEN) in lock step, with ONE GRU launch per forward for all R;
        -> the list of R (val_loss, examples), each the bits of that model's own validate() on its own loader (see infer()).
        `dataloaders`: a list / tuple of R loaders of equal length (zipped), or ONE loader whose batches every replica sees
        (train_epoch's rule); in every iteration the R batches must have one shape (ValueError otherwise).  DiffDelRNN: every
        loader needs `.dataset.fs` and `.dataset.delay_analyzer.max_delay`, all giving one warm-up length.
        `loss_fcn`: an ESRLoss or DCPreESR instance is evaluated for all replicas at once (one launch per kernel); any other
        callable of (pred, target) is applied to each replica in turn, on tensors laid out as that model's own validate() lays
        them out (a fresh prediction tensor, the replica's own target), so that a torch reduction takes the same path.  The losses
        of a batch reach the host in one .tolist() and are added in Python in the order the single validate adds its .item()s.
        The examples of replica r are the first stream of its slice, with the single model's keys."""
        return epoch.validate(self, dataloaders, loss_fcn, store_examples)

    @torch.no_grad()
    def predict(self, input, d_traj=None, segment_length=None):
        """Every replica's predict() (code/model.py:218-246, :618-653) on input (and d_traj, in samples) (R*Bper, 1, T)
        replica-major: initialize_hidden, the warm start of all R models -- ONE grouped launch of R x 1 stream over 1024 zeros --
        each warm state (hidden, and delay buffer) broadcast to its Bper streams, then the sequence whole or in `segment_length`
        pieces; -> y for RNN replicas, (y, pre_d) for DiffDelRNN replicas, the bits of each model's own predict() on its slice
        (see infer()).  The warm start is recomputed on every call (the models' `warm_cache` is neither read nor written: what it
        would hold is what the launch computes, and a stale key cannot arise).  As in DiffDelRNN.predict the delay-range assert
        is evaluated once, after the last piece has been enqueued."""
        R = len(self.models)
        if input.dim() != 3:
            raise RuntimeError(f"Replicas.predict: expected (N_BATCHES, N_CHANNELS, N_SAMPLES), got {tuple(input.shape)}")
        Bper = self._streams_per_replica(input.shape[0], R, "Replicas.predict")
        if self.diffdel and d_traj is None:
            raise RuntimeError("Replicas.predict: DiffDelRNN replicas need a delay trajectory")
        step = self.stepper(train=False)
        n_out = 2 if self.diffdel else 1
        self.initialize_hidden(1)
        zeros = torch.zeros((R, 1, START_LEN), device=self.device)
        with self._dl.deferred() if self.diffdel else contextlib.nullcontext():
            step(zeros, zeros, False)
            if Bper != 1:
                self.hidden = self.hidden.repeat_interleave(Bper, dim=1)
                if self.diffdel:
                    self._dl.buffer = self._dl.buffer.repeat_interleave(Bper, dim=0)
            self._share()
            outs = epoch.in_segments(lambda sl: step(input[:, :, sl], d_traj[:, :, sl] if self.diffdel else None, False)[:n_out],
                                     input, segment_length, n_out)
        return outs if self.diffdel else outs[0]


# ------------------------------------------------------------------------------------------
# ESR (the loss that follows the path in code/test-model.py:250-254,386-388)
# ------------------------------------------------------------------------------------------
ESR_EPS = 1e-5


@torch.no_grad()
def esr_sums(output, target, skip=0):
    """Per-stream [sum (t-y)^2, sum t^2] over samples [skip,T) as a (B,2) float64 HIP tensor."""
    y = _as_bt(output, "esr_sums")
    t = _as_bt(target, "esr_sums")
    B, T = y.shape
    L = _lib.lib()
    splits = L.ntm_esr_splits(B, T, int(skip))
    out = torch.empty(B, splits, 2, device=y.device, dtype=torch.float64)
    rc = L.ntm_esr_sums(ptr(y), ptr(t), B, T, int(skip), splits, ptr(out), _lib.current_stream())
    _lib.check(rc, "ntm_esr_sums")
    # the partial rows of a stream are added in index order (deterministic: no atomics on either side)
    return out[:, 0] if splits == 1 else out.sum(dim=1)


def esr_per_segment(output, target, skip=0):
    """CoreAudioML ESRLoss per stream: mean(e^2) / (mean(t^2) + 1e-5) over samples [skip,T)."""
    s = esr_sums(output, target, skip)
    n = output.shape[-1] - skip
    return (s[:, 0] / n) / (s[:, 1] / n + ESR_EPS)


def _replica_sums(rows, R, Bper, splits):
    """[R,2] fp64 whole-batch sums of R replicas from the per-stream rows [R*Bper, splits, 2] (ntm_loss_sums_replicas: one
    launch, the fixed order in which the single-model losses add the rows of one batch)."""
    s = torch.empty(R, 2, device=rows.device, dtype=torch.float64)
    _lib.check(_lib.lib().ntm_loss_sums_replicas(ptr(rows), R, Bper, splits, ptr(s), _lib.current_stream()), "ntm_loss_sums_replicas")
    return s


def _replica_split(output, R, what):
    B = output.shape[0]
    if R < 1 or B % R:
        raise ValueError(f"{what}: {B} streams do not divide into {R} replicas")
    return B // R


def _esr_ratio(s, n):
    """(loss, s) from whole-batch sums s [..., 2] fp64 over n elements."""
    return ((s[..., 0] / n) / (s[..., 1] / n + ESR_EPS)).float(), s


@torch.no_grad()
def _esr_value(output, target, R=None):
    """(ESR of the whole tensor, its sums [2] fp64); with R the [R] losses of the replica-major slices and their sums [R,2]."""
    if R is None:
        return _esr_ratio(esr_sums(output, target).sum(dim=0), output.numel())
    y = _as_bt(output, "esr_sums")
    t = _as_bt(target, "esr_sums")
    B, T = y.shape
    Bper = _replica_split(output, R, "ESRLoss.replicas")
    L = _lib.lib()
    splits = L.ntm_esr_splits(Bper, T, 0)          # of ONE replica's batch: the partial rows esr_sums forms for it alone
    rows = torch.empty(B, splits, 2, device=y.device, dtype=torch.float64)
    _lib.check(L.ntm_esr_sums(ptr(y), ptr(t), B, T, 0, splits, ptr(rows), _lib.current_stream()), "ntm_esr_sums")
    return _esr_ratio(_replica_sums(rows, R, Bper, splits), output.numel() // R)


def _loss(value, pole, output, target, R=None):
    """`value(output, target, R)`'s loss: a node of the graph where the output requires grad (training.loss_with_grad)."""
    if output.requires_grad and torch.is_grad_enabled():
        return training.loss_with_grad(output, target, value, pole, R)
    return value(output, target, R)[0]


class ESRLoss(torch.nn.Module):
    """ESR of a whole (B,1,T) tensor, as `loss_fcn(output, target)` in code/test-model.py:386-388.  With an output that
    requires grad (RNN.train_epoch, code/train.py:176) the same value as a differentiable scalar (adjoint: ntm_esr_grad)."""

    def forward(self, output, target):
        return _loss(_esr_value, None, output, target)

    def replicas(self, output, target, R):
        """[R] losses of a replica-major (R*Bper,1,T) tensor (Replicas.train_epoch): entry r is forward() on slice r, value and
        adjoint bit for bit, from one launch per kernel for all R."""
        return _loss(_esr_value, None, output, target, R)


DC_PRE_R = 0.995


@torch.no_grad()
def esr_dcpre_sums(output, target, skip=0, R=DC_PRE_R):
    """Per-stream ESR sums of the DC-blocked signals ((1 - z^-1)/(1 - R z^-1), zero state at `skip`).
    The filter runs in float32: against the exact recursion on the same inputs the sums are within 2e-5 relative at the
    shipped pole 0.995 for every length tested (to 65 536 samples: 2.9e-6) and at R = 0.9999 up to 16 384 samples (1.7e-5 on a
    DC level with small noise); at R = 0.9999 the error grows with the length, 2.6e-5 at 32 768 and 3.0e-5 at 65 536 samples
    (measured on an MI355X, tests/test_gpu_losses.py)."""
    y = _as_bt(output, "esr_dcpre_sums")
    t = _as_bt(target, "esr_dcpre_sums")
    B, T = y.shape
    out = torch.empty(B, 2, device=y.device, dtype=torch.float64)
    rc = _lib.lib().ntm_esr_dcpre_sums(ptr(y), ptr(t), B, T, int(skip), float(R), ptr(out), _lib.current_stream())
    _lib.check(rc, "ntm_esr_dcpre_sums")
    return out


class DCPreESR(torch.nn.Module):
    """`DCPreESR(dc_pre=True)` of code/test-model.py:252 / code/train.py:174 on a whole (B,1,T) tensor
    (GreyBoxDRC ESRLoss, un-vendored: definition re-derived, parity unpinned)."""

    def __init__(self, dc_pre=True, R=DC_PRE_R):
        super().__init__()
        self.dc_pre, self.R = dc_pre, R

    @property
    def _pole(self):
        return self.R if self.dc_pre else None

    @torch.no_grad()
    def _value(self, output, target, R=None):
        """_esr_value of the DC-blocked signals (of the signals themselves with dc_pre=False)."""
        if not self.dc_pre:
            return _esr_value(output, target, R)
        rows = esr_dcpre_sums(output, target, 0, self.R)
        if R is None:
            return _esr_ratio(rows.sum(dim=0), output.numel())
        Bper = _replica_split(output, R, "DCPreESR.replicas")
        return _esr_ratio(_replica_sums(rows, R, Bper, 1), output.numel() // R)

    def forward(self, output, target):
        """With an output that requires grad (RNN.train_epoch, code/train.py:174) the same value as a differentiable scalar
        (adjoint: ntm_esr_dcpre_grad, or ntm_esr_grad with dc_pre=False)."""
        return _loss(self._value, self._pole, output, target)

    def replicas(self, output, target, R):
        """[R] losses of a replica-major (R*Bper,1,T) tensor: entry r is forward() on slice r, value and adjoint bit for bit."""
        return _loss(self._value, self._pole, output, target, R)


MRSTFT_FFT_SIZES, MRSTFT_HOP_SIZES, MRSTFT_WIN_LENGTHS = (1024, 2048, 512), (120, 240, 50), (600, 1200, 240)
STFT_EPS = 1e-8


def _n_frames(T, skip, hop, what):
    """Frames of a centred STFT over samples [skip, T): 1 + (T - skip) // hop.  A hop below 1 is refused here with the
    library's own error type: the division would otherwise raise ZeroDivisionError before the library sees the call."""
    if int(hop) <= 0:
        raise _lib.NtmError(f"{what}: bad hop or win_length (hop = {hop})")
    return 1 + (T - int(skip)) // int(hop)


@torch.no_grad()
def stft_sums(output, target, skip=0, n_fft=1024, hop=120, win_length=600, eps=STFT_EPS):
    """Per-stream sums of one STFT resolution over samples [skip, T) (ntm_stft_sums):
    (B,4) fp64 = sum (mag_t - mag_y)^2 | sum mag_t^2 | sum |ln mag_y - ln mag_t| | sum |mag_y - mag_t|,
    and the number of (bin, frame) cells per stream."""
    y = _as_bt(output, "stft_sums")
    t = _as_bt(target, "stft_sums")
    B, T = y.shape
    n_frames = _n_frames(T, skip, hop, "stft_sums")
    # enough workgroups to fill 256 CUs a few times over, at least ~8 frames per wave
    chunks = max(1, min(-(-2048 // max(B, 1)), n_frames // 32))
    out = torch.empty(B, 4 * chunks, 4, device=y.device, dtype=torch.float64)
    rc = _lib.lib().ntm_stft_sums(ptr(y), ptr(t), B, T, int(skip), int(n_fft), int(hop), int(win_length), float(eps),
                                  chunks, ptr(out), _lib.current_stream())
    _lib.check(rc, "ntm_stft_sums")
    return out.sum(dim=1), n_frames * (int(n_fft) // 2 + 1)


class MRSTFTLoss(torch.nn.Module):
    """`MultiResolutionSTFTLoss()` of code/test-model.py:25,253 (auraloss.freq, un-vendored: definition taken
    from the published package, parity unpinned by the reference; arithmetic pinned to torch.stft by golden g10).
    Same constructor arguments as upstream for what the kernel covers: per resolution
    w_sc * ||mag_t - mag_y||_F / ||mag_t||_F + w_log_mag * mean|ln mag_y - ln mag_t| + w_lin_mag * mean|mag_y - mag_t|,
    averaged over the resolutions.  `forward(input, target)` treats the whole (B,1,T) tensor as one batch, as
    upstream does; `per_segment` gives one value per stream, which is how the harness aggregates
    (code/test-model.py:386-398, BATCH_SIZE = 1)."""

    def __init__(self, fft_sizes=MRSTFT_FFT_SIZES, hop_sizes=MRSTFT_HOP_SIZES, win_lengths=MRSTFT_WIN_LENGTHS,
                 w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, eps=STFT_EPS):
        super().__init__()
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)     # same check as upstream
        self.resolutions = list(zip(fft_sizes, hop_sizes, win_lengths))
        self.w_sc, self.w_log_mag, self.w_lin_mag, self.eps = w_sc, w_log_mag, w_lin_mag, eps

    @torch.no_grad()
    def _terms(self, output, target, skip, whole_batch, sums=None):
        """The loss value(s); `sums`, a list, receives the per-stream (B,4) fp64 sums of every resolution (what the adjoint needs)."""
        total = 0.0
        for n_fft, hop, win in self.resolutions:
            s, cells = stft_sums(output, target, skip, n_fft, hop, win, self.eps)
            if sums is not None:
                sums.append(s)
            if whole_batch:
                cells, s = cells * s.shape[0], s.sum(dim=0)
            total = total + (self.w_sc * torch.sqrt(s[..., 0]) / torch.sqrt(s[..., 1])
                             + self.w_log_mag * s[..., 2] / cells + self.w_lin_mag * s[..., 3] / cells)
        return total / len(self.resolutions)

    def _value(self, output, target, skip, whole_batch, sums=None):
        v = self._terms(output, target, skip, whole_batch, sums)
        return v.float() if whole_batch else v

    def _loss(self, output, target, skip, whole_batch):
        if output.requires_grad and torch.is_grad_enabled():
            return training.mrstft_with_grad(self, output, target, int(skip), whole_batch)
        return self._value(output, target, skip, whole_batch)

    def per_segment(self, output, target, skip=0):
        """[B] fp64 losses, one per stream.  With an output that requires grad a node of the graph (adjoint: ntm_stft_grad with
        each stream's own sums), same values."""
        return self._loss(output, target, skip, False)

    def forward(self, output, target):
        """With an output that requires grad (RNN.train_epoch / DiffDelRNN.train_epoch) the same value as a differentiable scalar:
        the adjoint runs ntm_stft_grad once per resolution, in constructor order, each after the first adding to dy.  A window
        must be longer than half the largest frame (reflect padding, as torch.stft): the default 2048-point resolution needs
        more than 1024 samples."""
        return self._loss(output, target, 0, True)


SPEC_SCALES = (2048, 1024, 512, 256, 128, 64)     # code/evaluation.py:23
SPEC_LOG_FLOOR = 1e-5                              # code/evaluation.py:44


@torch.no_grad()
def spec_sums(output, target, skip=0, n_fft=1024, hop=None, win_length=None, log_floor=SPEC_LOG_FLOOR):
    """Per-stream sums of the power-spectrogram terms (ntm_spec_sums): (B,4) fp64 =
    sum |P_y - P_t| | sum |log10 max(P_y,f) - log10 max(P_t,f)| | sum P_t | sum P_y, and the cells per stream."""
    hop = int(n_fft) // 4 if hop is None else int(hop)
    win_length = int(n_fft) if win_length is None else int(win_length)
    y = _as_bt(output, "spec_sums")
    t = _as_bt(target, "spec_sums")
    B, T = y.shape
    n_frames = _n_frames(T, skip, hop, "spec_sums")
    chunks = max(1, min(-(-2048 // max(B, 1)), n_frames // 32))
    out = torch.empty(B, 4 * chunks, 4, device=y.device, dtype=torch.float64)
    rc = _lib.lib().ntm_spec_sums(ptr(y), ptr(t), B, T, int(skip), int(n_fft), hop, win_length, float(log_floor), chunks,
                                  ptr(out), _lib.current_stream())
    _lib.check(rc, "ntm_spec_sums")
    return out.sum(dim=1), n_frames * (int(n_fft) // 2 + 1)


_MEL_CACHE = {}


@torch.no_grad()
def mel_sums(output, target, skip=0, n_fft=2048, hop=None, n_mels=160, sampling_rate=44100, log_floor=SPEC_LOG_FLOOR):
    """Per-stream sums of the two mel entries of code/evaluation.py:86-92 (ntm_mel_sums): (B,4) fp64 =
    sum |mel_y - mel_t| | sum |log10 max(mel_y,f) - log10 max(mel_t,f)| | sum mel_t | sum mel_y, and the cells per
    stream (frames x mel bands).  The mel basis (`librosa.filters.mel(sr, n_fft, n_mels)`, restated in
    utilities.mel_filterbank_sparse: parity unpinned) is built once per (sr, n_fft, n_mels, device) and kept."""
    from .utilities import mel_filterbank_sparse
    hop = int(n_fft) // 4 if hop is None else int(hop)
    y = _as_bt(output, "mel_sums")
    t = _as_bt(target, "mel_sums")
    B, T = y.shape
    key = (int(sampling_rate), int(n_fft), int(n_mels), y.device)
    if key not in _MEL_CACHE:
        first, start, w = mel_filterbank_sparse(sampling_rate, n_fft, n_mels)
        _MEL_CACHE[key] = tuple(torch.from_numpy(a).to(y.device) for a in (first, start, w))
    first, start, w = _MEL_CACHE[key]
    n_frames = _n_frames(T, skip, hop, "mel_sums")
    chunks = max(1, min(-(-2048 // max(B, 1)), n_frames // 32))
    out = torch.empty(B, 4 * chunks, 4, device=y.device, dtype=torch.float64)
    rc = _lib.lib().ntm_mel_sums(ptr(y), ptr(t), B, T, int(skip), int(n_fft), hop, int(n_fft), float(log_floor), chunks,
                                 int(n_mels), ptr(first), ptr(start), ptr(w), ptr(out), _lib.current_stream())
    _lib.check(rc, "ntm_mel_sums")
    return out.sum(dim=1), n_frames * int(n_mels)


class ValLossSupervised(torch.nn.Module):
    """`val_loss_supervised` of code/evaluation.py:18-100 (the validation metric bundle of the adversarial run) on
    the device, for what can be pinned here: `ms_spec_loss` / `ms_log_spec_loss` (sum over the six scales of the
    mean absolute difference of the power spectrograms / of their clamped log10; `TimeFreqConverter` is torchaudio's
    Spectrogram(n_fft, hop = n_fft/4, power 2) = torch.stft, golden g13), `mel_spec_loss` / `log_mel_spec_loss` (the
    n_fft = 2048 power spectrogram projected on 160 mel bands, :86-92; librosa's filter bank restated, parity
    unpinned), `ESR`, `ESRDCPre`, `MSE` -- the same seven keys as the reference's dict.
    forward(output, target) with (B, T) or (B, 1, T) tensors -> dict of python floats."""

    def __init__(self, spec_scales=SPEC_SCALES, log_eps=SPEC_LOG_FLOOR, n_mel_channels=160, sampling_rate=44100):
        super().__init__()
        self.spec_scales, self.log_eps = tuple(spec_scales), log_eps
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate

    @torch.no_grad()
    def forward(self, output, target):
        if output.dim() == 2:
            output, target = output.unsqueeze(1), target.unsqueeze(1)
        losses = {"ms_spec_loss": 0.0, "ms_log_spec_loss": 0.0}
        for n_fft in self.spec_scales:
            s, cells = spec_sums(output, target, 0, n_fft, log_floor=self.log_eps)
            tot = s.sum(dim=0) / (cells * s.shape[0])
            losses["ms_spec_loss"] += float(tot[0])
            losses["ms_log_spec_loss"] += float(tot[1])
        m, cells = mel_sums(output, target, 0, 2048, None, self.n_mel_channels, self.sampling_rate, self.log_eps)
        mt = m.sum(dim=0) / (cells * m.shape[0])
        losses["mel_spec_loss"], losses["log_mel_spec_loss"] = float(mt[0]), float(mt[1])
        n = output.numel()
        e = esr_sums(output, target).sum(dim=0)
        losses["ESR"] = float((e[0] / n) / (e[1] / n + ESR_EPS))
        losses["MSE"] = float(e[0] / n)
        d = esr_dcpre_sums(output, target).sum(dim=0)
        losses["ESRDCPre"] = float((d[0] / n) / (d[1] / n + ESR_EPS))
        return losses


class TimeFreqConverter(torch.nn.Module):
    """`TimeFreqConverter` of code/utilities/utilities.py:627-672, the front end of the reference's spectral critics, on the
    device and differentiable: same constructor arguments, same buffers (`window`, `mel_basis`) and attributes.  As in the
    reference the transform is torchaudio's Spectrogram(n_fft, hop_length = n_fft // 4, power = 2) -- the hop is n_fft / 4 and the
    window a periodic Hann of n_fft samples WHATEVER `hop_length` and `win_length` say (they are stored, and `window` is built
    from `win_length`, but neither reaches the transform).  `mel_basis` is the dense [n_mels, n_fft/2 + 1] float32 form of
    utilities.mel_filterbank_sparse (librosa's published algorithm restated: parity unpinned).
    forward(audio (..., T), mel=False) -> power spectrogram (..., bins, frames).squeeze(); mel=True -> (P, mel_basis @ P).
    With an input that requires grad the output is a node of the graph (training.SpectrogramFn: ntm_spectrogram /
    ntm_spectrogram_grad; the mel product is torch.matmul); otherwise no node is recorded."""

    def __init__(self, n_fft=2048, hop_length=512, win_length=2048, sampling_rate=44100, n_mel_channels=160, mel_fmin=0.0,
                 mel_fmax=None):
        super().__init__()
        from .utilities import mel_filterbank_sparse
        first, start, w = mel_filterbank_sparse(sampling_rate, n_fft, n_mel_channels, mel_fmin, mel_fmax)
        basis = np.zeros((n_mel_channels, n_fft // 2 + 1), np.float32)
        for m in range(n_mel_channels):
            basis[m, first[m]:first[m] + start[m + 1] - start[m]] = w[start[m]:start[m + 1]]
        self.register_buffer("mel_basis", torch.from_numpy(basis))
        self.register_buffer("window", torch.hann_window(win_length).float())
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.sampling_rate, self.n_mel_channels = sampling_rate, n_mel_channels

    def n_frames(self, n_samples):
        """Frames the transform makes of `n_samples` samples: the hop is n_fft // 4, not `hop_length`."""
        return 1 + int(n_samples) // (int(self.n_fft) // 4)

    def forward(self, audio, mel=False):
        _require_hip(audio, "TimeFreqConverter")
        n_fft = int(self.n_fft)
        lead = audio.shape[:-1]
        y = audio.reshape(-1, audio.shape[-1])
        y = (y if y.dtype == torch.float32 else y.float()).contiguous()
        if y.requires_grad and torch.is_grad_enabled():
            P = training.SpectrogramFn.apply(y, n_fft, n_fft // 4, n_fft)
        else:
            P = training.spectrogram(y.detach(), n_fft, n_fft // 4, n_fft)
        magnitude = P.reshape(lead + P.shape[-2:]).squeeze()
        if mel:
            return magnitude, torch.matmul(self.mel_basis, magnitude)
        return magnitude
