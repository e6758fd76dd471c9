"""Autograd nodes of the training path (RNN.train_epoch, code/model.py:90-161): GRU-HS[64] with input_size = output_size = 1 and
no skip connection, exact fp32, on the kernels of csrc/gru_train.hip.

  * GRUTrainStep: one stateful forward call of the GRU + head as a graph node.  forward = ntm_gru_train_forward (the step of the
    low-latency kernel -- the same code, csrc/gru_lat_step.h, so the same bits as kernel_variant "lat" -- plus the activations
    saved for BPTT); backward = ntm_gru_train_backward (one workgroup per stream) + ntm_gru_train_reduce (fixed-order sum over
    the streams): the gradients of the six parameters and of the initial state h0.  dh0 is what chains a window to the one before it (the warm-up of
    train_epoch is such a node: code/model.py:122 runs it with grad enabled and does not detach it).
  * DelayLineStep: one call of the time-varying fractional delay line of DiffDelRNN (code/model.py:269-320) as a graph node.
    forward = ntm_delay_forward into a FRESH new-buffer tensor (the old buffer stays as it was: an in-place update would cut
    the edge from the first window back to the warm-up, whose outputs fill the buffer the first window's taps read);
    backward = ntm_delay_backward, the deterministic adjoint (gradients for pre and, where it is in the graph, the old buffer).
  * loss_with_grad: the ESR / DCPreESR loss value exactly as the no-grad path computes it, and its adjoint on the device
    (ntm_esr_grad / ntm_esr_dcpre_grad).
  * mrstft_with_grad: the MRSTFTLoss value(s) exactly as the no-grad path computes them, and the adjoint of the STFT sums on the
    device (ntm_stft_grad, one call per resolution).
  * SpectrogramFn: the power spectrogram |STFT|^2 as a graph node whose OUTPUT a network reads (TimeFreqConverter, the front end
    of the reference's spectral critics): forward = ntm_spectrogram, backward = ntm_spectrogram_grad on the upstream gradient.
  * SpecCritFn: the conv stack of a spectral critic behind its spectrogram (critics.SpecCrit: weight-normed Conv1d layers with
    LeakyReLU(0.2) between them, the log10 head read into the first) as ONE graph node: forward = ntm_speccrit_forward,
    backward = ntm_speccrit_backward (data, weight and weight-norm gradients; the input gradient only where it is needed).
  * ConvStackFn: the dilated conv stack of the time-domain critic (critics.DilatedConvDisc: weight-normed Conv1d layers with a
    dilation each and LeakyReLU(slope) between them, on the raw waveform) as ONE graph node: forward = ntm_convstack_forward,
    backward = ntm_convstack_backward, with the same rules as SpecCritFn.
  * StridedConvStackFn: the strided, grouped, padded conv stack of the MelGAN critic (critics.NLayerDiscriminator) as ONE graph
    node that returns EVERY layer's output: forward = ntm_sconvstack_forward, backward = ntm_sconvstack_backward, which takes a
    gradient (or none) at each of them.
  * AdvHeadFn: the hinge / mean losses of the adversarial run on the K outputs of a critic (train_crit / train_gen of
    code/critics.py) as ONE graph node on the kernels of csrc/advhead_kernels.hip: forward = ntm_adv_head_forward, backward =
    ntm_adv_head_backward.
  * ResBlockFn: one ResnetBlock of the diffusion generators' UNet1D (diffusion.py) in its whole form as ONE graph node on the
    kernels of csrc/unet_train.hip: forward = ntm_unet_resblock_forward_save, backward = ntm_unet_resblock_backward +
    ntm_unet_wgrad_reduce.  UNet1D.forward_train builds its graph from these and torch ops.
  * ResBlockTiledFn: the same node in the block's tiled form, at any length (the levels of the noise net above 1024 frames):
    forward = ntm_unet_resblock_tiled_forward_save, backward = ntm_unet_resblock_tiled_backward + ntm_unet_wgrad_reduce.
  * DownCombineFn / UpCombineFn: one Downsample + CombinerDown, or CombinerUp + Upsample (S = 1: the combiner alone), step of
    that network as ONE graph node each on csrc/unet_resample_train.hip: forward = the inference launch (ntm_unet_down_combine /
    ntm_unet_up_combine), backward = ntm_unet_down_combine_backward / ntm_unet_up_combine_backward + ntm_unet_wgrad_reduce.
    diffusion.down_combine / up_combine route through them when an operand requires a gradient.
  * GRUTrainStep and loss_with_grad take an optional replica count R: the same nodes for R independent models stacked
    replica-major (model.Replicas) through the `_replicas` entry points -- one forward, one BPTT, one reduction and one loss
    launch for all of them, each replica's bits those of the R = None node on its slice.  The reduction and the loss adjoints
    are one kernel each either way (one model is its R = 1); the forward and the BPTT keep a plain and a replica form.
"""
import torch

from . import _lib
from ._lib import ptr

HIDDEN = 64
SUPPORTED = "RNN(input_size=1, hidden_size=64, output_size=1, skip=False) on a HIP device"
SUPPORTED_DIFFDEL = "DiffDelRNN(input_size=1, hidden_size=64, output_size=1, skip=False) on a HIP device"


def _entry(name, B, R):
    """The C entry point of a node and its leading size arguments: `name`(..., B, ...) for one model (R None), else
    `name`_replicas(..., R, Bper, ...)."""
    if R is None:
        return name, (B,)
    return name + "_replicas", (R, B // R)


class GRUTrainStep(torch.autograd.Function):
    """(x [B,T] fp32 contiguous, h0 [B,64], w_ih, w_hh, b_ih, b_hh, w_o, b_o, R=None) -> (y [B,T], h_T [B,64]), both fresh tensors.
    R None: one model, the parameters in their own shapes (b_o None for the bias-free head).  R an integer: R independent models
    in one launch each way (model.Replicas) -- x and h0 stacked replica-major, B = R * Bper, the parameters as contiguous
    [R, ...] stacks; every replica's slice has the bits the R = None node gives on it alone, and the gradients come back as
    [R, ...] stacks (the caller builds the stacks with torch.stack inside the graph, so each model gets its own .grad)."""

    @staticmethod
    def forward(ctx, x, h0, w_ih, w_hh, b_ih, b_hh, w_o, b_o, R=None):
        B, T = x.shape
        if R is not None:
            if R < 1 or B % R:
                raise RuntimeError(f"GRUTrainStep: {B} streams do not divide into {R} replicas")
            for w in (w_ih, w_hh, b_ih, b_hh, w_o, b_o):
                if w is not None and (w.shape[0] != R or not w.is_contiguous() or w.dtype != torch.float32):
                    raise RuntimeError("GRUTrainStep: the parameters must be contiguous float32 [R, ...] stacks")
        L = _lib.lib()
        h = h0.detach().to(torch.float32).reshape(B, HIDDEN).clone(memory_format=torch.contiguous_format)
        y = torch.empty(B, T, device=x.device, dtype=torch.float32)
        ws = torch.empty(max(int(L.ntm_gru_train_workspace_floats(B, T)), 1), device=x.device, dtype=torch.float32)
        name, sizes = _entry("ntm_gru_train_forward", B, R)
        _lib.check(getattr(L, name)(ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(w_o), ptr(b_o), ptr(x), ptr(y), *sizes, T, T, T,
                                    ptr(h), ptr(ws), _lib.current_stream()), name)
        # the weights through save_for_backward: torch's version counters then refuse a backward after an in-place update
        ctx.save_for_backward(x, ws, w_ih, w_hh, b_ih, b_hh, w_o, b_o)
        ctx.h0_shape, ctx.R = h0.shape, R
        ctx.set_materialize_grads(False)
        return y, h

    @staticmethod
    def backward(ctx, dy, dh):
        x, ws, w_ih, w_hh, b_ih, b_hh, w_o, b_o = ctx.saved_tensors
        B, T = x.shape
        R, dev = ctx.R, x.device
        dy = None if dy is None else dy.to(torch.float32).contiguous()
        dh = None if dh is None else dh.to(torch.float32).reshape(B, HIDDEN).contiguous()
        dh0 = torch.empty(B, HIDDEN, device=dev, dtype=torch.float32)
        part = torch.empty(max(B, 1), _lib.TRAIN_GRAD_FLOATS, device=dev, dtype=torch.float32)
        grad = torch.empty(1 if R is None else R, _lib.TRAIN_GRAD_FLOATS, device=dev, dtype=torch.float32)
        L, s = _lib.lib(), _lib.current_stream()
        name, sizes = _entry("ntm_gru_train_backward", B, R)
        _lib.check(getattr(L, name)(ptr(w_hh), ptr(w_o), ptr(x), T, ptr(ws), ptr(dy), T, ptr(dh), *sizes, T, ptr(dh0), ptr(part), s), name)
        name, sizes = _entry("ntm_gru_train_reduce", B, R)
        _lib.check(getattr(L, name)(ptr(part), *sizes, ptr(grad), s), name)
        H3 = 3 * HIDDEN
        g_wih, g_whh, g_bih, g_bhh, g_wo, g_bo = torch.split(grad, [H3, H3 * HIDDEN, H3, H3, HIDDEN, 1], dim=1)
        return (None, dh0.view(ctx.h0_shape), g_wih.reshape(w_ih.shape), g_whh.reshape(w_hh.shape), g_bih.reshape(b_ih.shape),
                g_bhh.reshape(b_hh.shape), g_wo.reshape(w_o.shape), None if b_o is None else g_bo.reshape(b_o.shape), None)


class DelayLineStep(torch.autograd.Function):
    """(pre [B,L] fp32 contiguous, buffer [B,1,D], d [B,L] in samples, warmup, err_flag) -> (y [B,L], new_buffer [B,1,D]), both
    fresh tensors.  The range check (code/model.py:284) raises the caller's sticky device flag; the new buffer is then the old
    one unchanged (ntm_delay_forward skips its update), and the caller raises AssertionError before it keeps anything."""

    @staticmethod
    def forward(ctx, pre, buffer, d, warmup, err):
        B, T = pre.shape
        D = buffer.shape[-1]
        y = torch.empty_like(pre)
        nb = buffer.detach().to(torch.float32).reshape(B, D).clone(memory_format=torch.contiguous_format)
        _lib.check(_lib.lib().ntm_delay_forward(ptr(pre), ptr(d), ptr(y), B, T, ptr(nb), D, int(bool(warmup)), ptr(err),
                                                _lib.current_stream()), "ntm_delay_forward")
        ctx.save_for_backward(d)
        ctx.warmup, ctx.buf_shape = bool(warmup), buffer.shape
        ctx.set_materialize_grads(False)
        return y, nb.view(buffer.shape)

    @staticmethod
    def backward(ctx, gy, gnb):
        d, = ctx.saved_tensors
        B, T = d.shape
        D = ctx.buf_shape[-1]
        gy = None if gy is None else gy.to(torch.float32).contiguous()
        gnb = None if gnb is None else gnb.to(torch.float32).reshape(B, D).contiguous()
        gpre = torch.empty(B, T, device=d.device, dtype=torch.float32)
        gbuf = torch.empty(B, D, device=d.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().ntm_delay_backward(ptr(gy), ptr(d), ptr(gnb), ptr(gpre), ptr(gbuf), B, T, D, int(ctx.warmup), 0,
                                                 _lib.current_stream()), "ntm_delay_backward")
        return gpre, None if gbuf is None else gbuf.view(ctx.buf_shape), None, None, None


class _LossFn(torch.autograd.Function):
    """Shared body of the two loss nodes: `value(output, target, R)` -> (loss, whole-batch sums fp64) runs under no_grad.  R None:
    one scalar loss, sums [2]; R an integer: [R] losses of the replica-major slices, sums [R,2]."""

    @staticmethod
    def forward(ctx, output, target, value, pole, R):
        loss, sums = value(output, target, R)
        ctx.save_for_backward(output, target, sums)
        ctx.pole, ctx.R = pole, R
        return loss

    @staticmethod
    def backward(ctx, gout):
        from .model import ESR_EPS, _as_bt
        output, target, sums = ctx.saved_tensors
        y = _as_bt(output, "loss backward")
        t = _as_bt(target, "loss backward")
        B, T = y.shape
        R = ctx.R
        g = gout.detach().to(device=y.device, dtype=torch.float32).reshape(1 if R is None else R).contiguous()
        dy = torch.empty(B, T, device=y.device, dtype=torch.float32)
        L, s = _lib.lib(), _lib.current_stream()
        if ctx.pole is None:
            name, sizes = _entry("ntm_esr_grad", B, R)
            _lib.check(getattr(L, name)(ptr(y), ptr(t), *sizes, T, ptr(sums), ptr(g), ESR_EPS, ptr(dy), s), name)
        else:
            name, sizes = _entry("ntm_esr_dcpre_grad", B, R)
            _lib.check(getattr(L, name)(ptr(y), ptr(t), *sizes, T, float(ctx.pole), ptr(sums), ptr(g), ESR_EPS, ptr(dy), s), name)
        return dy.view(output.shape).to(output.dtype), None, None, None, None


def loss_with_grad(output, target, value, pole, R=None):
    """The loss node: `value` computes the no-grad path's value(s) and the whole-batch sums; pole None = ESR, else DCPreESR's
    coefficient.  R None: the scalar loss of the whole tensor; R an integer: the [R] losses of a replica-major (R*Bper,1,T) output."""
    if target.requires_grad:
        raise RuntimeError("ESRLoss / DCPreESR: gradients flow to the prediction only; the target must not require grad")
    return _LossFn.apply(output, target, value, pole, R)


class _MRSTFTLossFn(torch.autograd.Function):
    """MRSTFTLoss.forward (whole_batch: one float32 scalar from the batch totals) / per_segment ([B] float64) as a graph node.  The
    value is model.MRSTFTLoss._value's, computed under no_grad; the per-stream sums (B,4) fp64 of every resolution are saved."""

    @staticmethod
    def forward(ctx, output, target, loss, skip, whole_batch):
        sums = []
        value = loss._value(output, target, skip, whole_batch, sums)
        ctx.save_for_backward(output, target, *sums)
        ctx.loss, ctx.skip, ctx.whole_batch = loss, skip, whole_batch
        return value

    @staticmethod
    def backward(ctx, gout):
        from .model import _as_bt, _n_frames
        output, target, *sums = ctx.saved_tensors
        loss, skip = ctx.loss, ctx.skip
        y = _as_bt(output, "MRSTFTLoss backward")
        t = _as_bt(target, "MRSTFTLoss backward")
        B, T = y.shape
        nres = len(loss.resolutions)
        # coefficient rows (c_sc, c_log, c_lin) per stream in float64 on the device (no host synchronisation), rounded once
        g = gout.detach().to(device=y.device, dtype=torch.float64).reshape(1 if ctx.whole_batch else B)
        dy = torch.empty(B, T, device=y.device, dtype=torch.float32)
        L, st = _lib.lib(), _lib.current_stream()
        # resolutions in constructor order: the first call stores dy, every later one adds to it (dy = dy + gradient)
        for r, ((n_fft, hop, win), s) in enumerate(zip(loss.resolutions, sums)):
            cells = _n_frames(T, skip, hop, "MRSTFTLoss backward") * (int(n_fft) // 2 + 1)
            if ctx.whole_batch:
                cells, s = cells * B, s.sum(dim=0, keepdim=True)
            den = torch.sqrt(s[:, 0]) * torch.sqrt(s[:, 1])
            zero = s[:, 0] == 0                                     # torch.norm's subgradient at 0
            c_sc = torch.where(zero, torch.zeros_like(den), g * loss.w_sc / (nres * torch.where(zero, torch.ones_like(den), den)))
            c_log = g * (loss.w_log_mag / (nres * cells))
            c_lin = g * (loss.w_lin_mag / (nres * cells))
            coef = torch.stack([c_sc, c_log, c_lin], dim=1).to(torch.float32).expand(B, 3).contiguous()
            ws = torch.empty(max(int(L.ntm_stft_grad_workspace_floats(B, T, skip, int(n_fft), int(hop))), 1), device=y.device,
                             dtype=torch.float32)
            _lib.check(L.ntm_stft_grad(ptr(y), ptr(t), B, T, skip, int(n_fft), int(hop), int(win), float(loss.eps), ptr(coef),
                                       ptr(ws), ptr(dy), int(r > 0), st), "ntm_stft_grad")
        return dy.view(output.shape).to(output.dtype), None, None, None, None


def mrstft_with_grad(loss, output, target, skip, whole_batch):
    """The MRSTFTLoss node: value(s) of the no-grad path bit for bit; gradients flow to the prediction only."""
    if target.requires_grad:
        raise RuntimeError("MRSTFTLoss: gradients flow to the prediction only; the target must not require grad")
    return _MRSTFTLossFn.apply(output, target, loss, skip, whole_batch)


def spectrogram(y, n_fft, hop, win):
    """ntm_spectrogram on a contiguous float32 [B,T] device tensor -> P [B, n_fft/2 + 1, 1 + T // hop] float32, no graph."""
    B, T = y.shape
    if int(hop) <= 0:
        raise _lib.NtmError(f"ntm_spectrogram: bad hop or win_length (hop = {hop})")
    P = torch.empty(B, int(n_fft) // 2 + 1, 1 + T // int(hop), device=y.device, dtype=torch.float32)
    _lib.check(_lib.lib().ntm_spectrogram(ptr(y), B, T, int(n_fft), int(hop), int(win), ptr(P), _lib.current_stream()),
               "ntm_spectrogram")
    return P


class SpectrogramFn(torch.autograd.Function):
    """(y [B,T] fp32 contiguous, n_fft, hop, win) -> P [B, bins, frames].  Only y is saved: the adjoint recomputes the spectrum.
    Gradients go to the signal; no double backward."""

    @staticmethod
    def forward(ctx, y, n_fft, hop, win):
        P = spectrogram(y, n_fft, hop, win)
        ctx.save_for_backward(y)
        ctx.res = (int(n_fft), int(hop), int(win))
        return P

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gP):
        y, = ctx.saved_tensors
        n_fft, hop, win = ctx.res
        B, T = y.shape
        gP = gP.to(torch.float32).contiguous()
        L = _lib.lib()
        ws = torch.empty(max(int(L.ntm_stft_grad_workspace_floats(B, T, 0, n_fft, hop)), 1), device=y.device, dtype=torch.float32)
        dy = torch.empty(B, T, device=y.device, dtype=torch.float32)
        _lib.check(L.ntm_spectrogram_grad(ptr(y), ptr(gP), B, T, n_fft, hop, win, ptr(ws), ptr(dy), 0, _lib.current_stream()),
                   "ntm_spectrogram_grad")
        return dy, None, None, None


# The three critic conv stacks (SpecCritFn, ConvStackFn, StridedConvStackFn) differ in their layer records, in the scalar beside
# them and in where the outputs live; the rest is these helpers.  `name` is the class, `prefix` the entry points' (ntm_<prefix>_*),
# `make_layers` the _lib builder of the layer array.

def _stack_begin(name, prefix, make_layers, x, spec, params):
    """The preamble of a forward: checks, fp32 contiguous copies, the layer array and the `saved` buffer at its size.
    -> (x, ps, spec, layers, saved)"""
    spec = tuple(tuple(int(q) for q in s) for s in spec)
    n = len(spec)
    if len(params) != 3 * n:
        raise RuntimeError(f"{name}: {n} layers need {3 * n} parameters (weight_g, weight_v, bias each), got {len(params)}")
    if not x.is_cuda:
        raise RuntimeError(f"{name}: HIP device only (no CPU fallback)")
    x = x.detach().to(torch.float32).contiguous()
    ps = [p.detach().to(torch.float32).contiguous() for p in params]
    B, C0, F0 = x.shape
    L = _lib.lib()
    layers = make_layers(spec)
    n_saved = int(getattr(L, f"ntm_{prefix}_saved_floats")(B, C0, F0, n, layers))
    if n_saved < 0:
        raise _lib.NtmError(f"ntm_{prefix}_forward refused the sizes: {L.ntm_last_error().decode()}")
    return x, ps, spec, layers, torch.empty(max(n_saved, 1), device=x.device, dtype=torch.float32)


def _stack_forward(prefix, x, scalar, spec, layers, ps, saved, out):
    """ntm_<prefix>_forward; out: the output tensor, or the list of every layer's."""
    B, C0, F0 = x.shape
    _lib.check(getattr(_lib.lib(), f"ntm_{prefix}_forward")(
        ptr(x), B, C0, F0, scalar, len(spec), layers, _lib.ptr_array(ps[0::3]), _lib.ptr_array(ps[1::3]), _lib.ptr_array(ps[2::3]),
        ptr(saved), _lib.ptr_array(out) if isinstance(out, list) else ptr(out), _lib.current_stream()), f"ntm_{prefix}_forward")


def _stack_backward(ctx, prefix, make_layers, x, saved, ps, arriving, call=True):
    """ntm_<prefix>_backward and the bookkeeping around it: gx and the parameter gradients only where needs_input_grad asks,
    zeros where B == 0 or nothing is to be computed (call False).  arriving: the tensors that stand between `saved` and gx in the
    entry point's arguments -- the gradient at the output, or the lists outs and gouts.  -> backward's return value"""
    scalar, spec = ctx.res
    n = len(spec)
    B, C0, F0 = x.shape
    gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    want = any(ctx.needs_input_grad[3:])
    grads = [torch.empty_like(p) for p in ps] if want else []
    if call:
        L = _lib.lib()
        layers = make_layers(spec)
        ws = torch.empty(max(int(getattr(L, f"ntm_{prefix}_workspace_floats")(B, C0, F0, n, layers)), 1), device=x.device,
                         dtype=torch.float32)
        arr = (lambda q: _lib.ptr_array(q) if want else None)
        _lib.check(getattr(L, f"ntm_{prefix}_backward")(
            ptr(x), B, C0, F0, scalar, n, layers, _lib.ptr_array(ps[0::3]), _lib.ptr_array(ps[1::3]), ptr(saved), *[_lib.ptr_array(t) if isinstance(t, list) else ptr(t) for t in arriving], ptr(gx),
            arr(grads[0::3]), arr(grads[1::3]), arr(grads[2::3]), ptr(ws), _lib.current_stream()), f"ntm_{prefix}_backward")
    if B == 0 or not call:
        gx = None if gx is None else gx.zero_()
        grads = [g.zero_() for g in grads]
    pg = [g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:])] if want else [None] * (3 * n)
    return (gx, None, None, *pg)


class SpecCritFn(torch.autograd.Function):
    """(x [B, C0, F0] fp32 contiguous, log_floor, spec, g_0, v_0, bias_0, g_1, ...) -> out [B, c_out of the last layer, F_out].
    spec: ((c_in, c_out, k, groups), ...), one entry per layer; the parameters are the layers' weight_g [c_out, 1, 1], weight_v
    [c_out, c_in/groups, k] and bias [c_out], three per layer.  log_floor > 0: the first layer reads log10(max(x, log_floor)).
    Saved: x, the parameters and the buffer ntm_speccrit_forward fills (effective weights, 1/|v|, every layer's output but the last).
    The input gradient is computed only where needs_input_grad asks for it; no double backward."""

    @staticmethod
    def forward(ctx, x, log_floor, spec, *params):
        x, ps, spec, layers, saved = _stack_begin("SpecCritFn", "speccrit", _lib.conv_layers, x, spec, params)
        F_out = x.shape[2] - sum(k - 1 for _, _, k, _ in spec)
        out = torch.empty(x.shape[0], spec[-1][1], F_out, device=x.device, dtype=torch.float32)
        _stack_forward("speccrit", x, float(log_floor), spec, layers, ps, saved, out)
        ctx.save_for_backward(x, saved, *ps)
        ctx.res = (float(log_floor), spec)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, saved, *ps = ctx.saved_tensors
        gout = gout.to(torch.float32).contiguous()
        return _stack_backward(ctx, "speccrit", _lib.conv_layers, x, saved, ps, [gout])


class ConvStackFn(torch.autograd.Function):
    """(x [B, C0, F0] fp32 contiguous, slope, spec, g_0, v_0, bias_0, g_1, ...) -> out [B, c_out of the last layer, F_out].
    spec: ((c_in, c_out, k, groups, dilation), ...), one entry per layer (at most 16); the parameters are the layers' weight_g
    [c_out, 1, 1], weight_v [c_out, c_in/groups, k] and bias [c_out], three per layer.  slope in (0, 1): the LeakyReLU after every
    layer but the last.  Saved: x, the parameters and the buffer ntm_convstack_forward fills (effective weights, 1/|v|, every
    layer's output but the last).  The input gradient and the parameter gradients are computed only where needs_input_grad asks
    for them; no double backward."""

    @staticmethod
    def forward(ctx, x, slope, spec, *params):
        x, ps, spec, layers, saved = _stack_begin("ConvStackFn", "convstack", _lib.conv_layers_d, x, spec, params)
        F_out = x.shape[2] - sum((k - 1) * d for _, _, k, _, d in spec)
        out = torch.empty(x.shape[0], spec[-1][1], F_out, device=x.device, dtype=torch.float32)
        _stack_forward("convstack", x, float(slope), spec, layers, ps, saved, out)
        ctx.save_for_backward(x, saved, *ps)
        ctx.res = (float(slope), spec)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, saved, *ps = ctx.saved_tensors
        gout = gout.to(torch.float32).contiguous()
        return _stack_backward(ctx, "convstack", _lib.conv_layers_d, x, saved, ps, [gout])


def _sconvstack_frames(F0, spec):
    """Frames entering every layer and leaving the last: F[l+1] = floor((F[l] + 2 pad - k) / stride) + 1."""
    F = [int(F0)]
    for _, _, k, _, stride, pad, _ in spec:
        F.append((F[-1] + 2 * pad - k) // stride + 1)
    return F


class StridedConvStackFn(torch.autograd.Function):
    """(x [B, C0, F0] fp32 contiguous, slope, spec, g_0, v_0, bias_0, g_1, ...) -> a tuple of n tensors, the output of every layer:
    [B, c_out[l], F[l+1]], post-activation for all but the last.  spec: ((c_in, c_out, k, groups, stride, pad, pad_mode), ...), one
    entry per layer (at most 16), pad_mode 0 zeros, 1 reflect (first layer only); the parameters are the layers' weight_g
    [c_out, 1, 1], weight_v [c_out, c_in/groups, k] and bias [c_out], three per layer.  slope in (0, 1): the LeakyReLU after every
    layer but the last.  Saved: x, the parameters, the buffer ntm_sconvstack_forward fills (effective weights, 1/|v|) and the
    OUTPUTS themselves -- they are the activations the backward reads, so an in-place edit of a returned feature before backward
    raises torch's version error.  An output no gradient arrives at is a NULL entry of gouts; the input gradient and the parameter
    gradients are computed only where needs_input_grad asks for them; no double backward."""

    @staticmethod
    def forward(ctx, x, slope, spec, *params):
        x, ps, spec, layers, saved = _stack_begin("StridedConvStackFn", "sconvstack", _lib.conv_layers_s, x, spec, params)
        F = _sconvstack_frames(x.shape[2], spec)
        outs = [torch.empty(x.shape[0], spec[l][1], F[l + 1], device=x.device, dtype=torch.float32) for l in range(len(spec))]
        _stack_forward("sconvstack", x, float(slope), spec, layers, ps, saved, outs)
        ctx.save_for_backward(x, saved, *ps, *outs)
        ctx.res = (float(slope), spec)
        ctx.set_materialize_grads(False)        # an output no gradient arrives at stays None: a NULL gouts entry, no zero tensor
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        n = len(ctx.res[1])
        x, saved, *rest = ctx.saved_tensors
        ps, outs = rest[:3 * n], rest[3 * n:]
        gouts = [None if g is None else g.to(torch.float32).contiguous() for g in gouts]
        return _stack_backward(ctx, "sconvstack", _lib.conv_layers_s, x, saved, ps, [list(outs), gouts],
                               call=not all(g is None for g in gouts) and x.shape[0] != 0)


class AdvHeadFn(torch.autograd.Function):
    """(mode, n_fake, *outs) -> the adversarial loss on the K outputs of a critic as ONE graph node, a 0-dim float32 tensor:
    mode "crit"  sum_k relu(1 + o_k[:n_fake]).mean() + sum_k relu(1 - o_k[n_fake:]).mean()   (train_crit, code/critics.py:47-58),
    mode "gen"   sum_k -o_k.mean()                                                          (train_gen, :60-68; n_fake is not read).
    outs: K (at most 8) float32 tensors [rows, ...] of one row count (`.contiguous()` is called on the others): a MultiSpecCrit's
    list, [D] of a DilatedConvDisc, [scale[-1] for scale in D] of a MelGCrit.  forward = ntm_adv_head_forward (the terms in fp32 as
    torch forms them, fixed-order fp64 sums, every mean rounded to fp32 once, the means added in fp32 in the reference's order;
    two launches), backward = ntm_adv_head_backward (one launch writes all K gradients with the bits of torch's autograd on the
    reference's expression; a None upstream gradient writes nothing).  No atomics; no double backward."""

    @staticmethod
    def forward(ctx, mode, n_fake, *outs):
        if mode not in _lib.ADV_HEAD_MODES:
            raise RuntimeError(f"AdvHeadFn: mode {mode!r}; built: 'crit' and 'gen'")
        K = len(outs)
        if not 1 <= K <= _lib.ADV_HEAD_MAX_K:
            raise RuntimeError(f"AdvHeadFn: {K} outputs; built: 1 to {_lib.ADV_HEAD_MAX_K}")
        if not all(o.is_cuda for o in outs):
            raise RuntimeError("AdvHeadFn: HIP device only (no CPU fallback)")
        outs = [o.detach().to(torch.float32).contiguous() for o in outs]
        rows = outs[0].shape[0] if outs[0].dim() else 0
        if any(o.dim() < 1 or o.shape[0] != rows for o in outs):
            raise RuntimeError(f"AdvHeadFn: the outputs must share their first dimension, got {[tuple(o.shape) for o in outs]}")
        n_fake = int(n_fake) if mode == "crit" else 0
        elems = [o.numel() // max(rows, 1) for o in outs]
        segs = K if mode == "gen" else 2 * K
        longest = max(max(n_fake, rows - n_fake) * e for e in elems)
        n_ws = segs * max(-(-longest // _lib.ADV_HEAD_CHUNK), 1)
        ws = torch.empty(n_ws, device=outs[0].device, dtype=torch.float64)
        loss = torch.empty((), device=outs[0].device, dtype=torch.float32)
        _lib.check(_lib.lib().ntm_adv_head_forward(_lib.ptr_array(outs), _lib.i64_array(elems), K, rows, n_fake,
                                                   _lib.ADV_HEAD_MODES[mode], ptr(ws), n_ws, ptr(loss), _lib.current_stream()),
                   "ntm_adv_head_forward")
        ctx.save_for_backward(*outs)
        ctx.res = (mode, n_fake, rows, elems)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        outs = ctx.saved_tensors
        if gout is None:
            return (None, None) + (None,) * len(outs)
        mode, n_fake, rows, elems = ctx.res
        g = gout.detach().to(device=outs[0].device, dtype=torch.float32).reshape(1).contiguous()
        grads = [torch.empty_like(o) for o in outs]
        _lib.check(_lib.lib().ntm_adv_head_backward(_lib.ptr_array(outs), _lib.i64_array(elems), len(outs), rows, n_fake,
                                                    _lib.ADV_HEAD_MODES[mode], ptr(g), _lib.ptr_array(grads), _lib.current_stream()),
                   "ntm_adv_head_backward")
        return (None, None, *[gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[2:])])


# The two block nodes (ResBlockFn, ResBlockTiledFn) differ in their entry points, in the form they ask for and in how the
# partials are laid out; the rest is these two helpers.  `fam`: (class name, form, prefix of the entry points).

def _resblock_forward(ctx, fam, src0, src1, film, w_first, w_gated, w_res, init_w, off0):
    from . import diffusion as D
    name, form, prefix = fam
    D._require_hip(name, src0, src1, film, w_first, w_gated, w_res, init_w)
    if init_w is not None and src0.requires_grad:
        raise RuntimeError(f"{name}: with init_w the waveform takes no gradient")
    src0, film, w_first, w_gated = (t.detach().contiguous() for t in (src0, film, w_first, w_gated))
    src1, w_res, init_w = (None if t is None else t.detach().contiguous() for t in (src1, w_res, init_w))
    B, T0 = src0.shape[0], src0.shape[2]
    c0 = init_w.shape[0] if init_w is not None else src0.shape[1]
    c1, T1 = (0, 0) if src1 is None else src1.shape[1:]
    T = T1 if src1 is not None else T0 - int(off0)
    if form == "tiled" and T > D.WHOLE_MAX_T:
        form = "auto"               # what the entry points pick themselves at this length; "tiled" forces it on a shorter block
    spec = D.BlockSpec(c0, c1, w_first.shape[0], w_gated.shape[0], T, T0, int(off0), T1, 0, int(init_w is not None),
                       D.FORMS[form])
    L, ref = _lib.lib(), _lib.ctypes.byref(spec)
    n_save = getattr(L, prefix + "save_floats")(B, ref)
    if n_save < 0:
        raise _lib.NtmError(f"{prefix}save_floats refused: {L.ntm_last_error().decode()}")
    if film.shape[0] not in (1, B) or film.shape[1] != c0 + c1:
        raise RuntimeError(f"{name}: film {tuple(film.shape)} for {B} streams of {c0 + c1} channels")
    ysave = torch.empty(max(n_save, 1), dtype=torch.float32, device=src0.device)
    out = torch.empty(B, spec.c_out, T, dtype=torch.float32, device=src0.device)
    fstride = 0 if film.shape[0] == 1 else film.stride(0)
    _lib.check(getattr(L, prefix + "forward_save")(ptr(src0), ptr(src1), ptr(init_w), ptr(film), fstride, ptr(w_first),
                                                   ptr(w_gated), ptr(w_res), B, ref, ptr(ysave), ptr(out),
                                                   _lib.current_stream()), prefix + "forward_save")
    ctx.save_for_backward(src0, src1, film, w_first, w_gated, w_res, init_w, ysave)
    ctx.spec = spec
    return out


def _resblock_backward(ctx, fam, gout):
    src0, src1, film, w_first, w_gated, w_res, init_w, ysave = ctx.saved_tensors
    spec, need = ctx.spec, ctx.needs_input_grad
    tiled = fam[1] == "tiled"
    prefix = fam[2]
    L, ref = _lib.lib(), _lib.ctypes.byref(spec)
    B, cin, cout, n, dev = src0.shape[0], spec.c0 + spec.c1, spec.c_out, spec.n_layers, src0.device
    gout = gout.detach().to(torch.float32).contiguous()
    per, total = getattr(L, prefix + "wgrad_floats")(ref), getattr(L, prefix + "partial_floats")(B, ref)
    n_ws = L.ntm_unet_resblock_tiled_workspace_floats(B, ref) if tiled else B * cout * spec.T
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)       # noqa: E731
    g0 = torch.empty_like(src0) if need[0] and init_w is None else None
    g1 = torch.empty_like(src1) if src1 is not None and need[1] else None
    gfilm, part, ws, grads = new(B, cin), new(max(total, 1)), new(max(n_ws, 1)), new(per)
    fstride = 0 if film.shape[0] == 1 else film.stride(0)
    _lib.check(getattr(L, prefix + "backward")(ptr(src0), ptr(src1), ptr(init_w), ptr(film), fstride, ptr(w_first), ptr(w_gated),
                                               ptr(w_res), B, ref, ptr(ysave), ptr(gout), ptr(ws), ptr(g0), ptr(g1), ptr(gfilm),
                                               ptr(part), _lib.current_stream()), prefix + "backward")
    # whole: every (stream, wave) partial; tiled: the per-stream sums the backward left at the head of the buffer
    _lib.check(L.ntm_unet_wgrad_reduce(ptr(part), B if tiled else total // per, per, ptr(grads), _lib.current_stream()),
               "ntm_unet_wgrad_reduce")
    n_g, n_1 = n * cout * cout * 5, cout * cin
    d_gated = grads[:n_g].view(n, cout, cout, 5)
    d_first = grads[n_g:n_g + n_1].view(cout, cin, 1)
    d_res = None if w_res is None else grads[n_g + n_1:n_g + 2 * n_1].view(cout, cin, 1)
    d_init = None if init_w is None else grads[n_g + 2 * n_1:].view(spec.c0, 1, 5)
    if film.shape[0] == 1 and B != 1:
        gfilm = gfilm.sum(0, keepdim=True)            # one FiLM vector for all streams: the rows add
    return g0, g1, gfilm, d_first, d_gated, d_res, d_init, None


class ResBlockFn(torch.autograd.Function):
    """(src0, src1 | None, film, w_first, w_gated, w_res | None, init_w | None, off0) -> one ResnetBlock of the diffusion
    generators' UNet1D as ONE graph node, in the whole form (at most 1024 frames): the operands of diffusion.resblock_forward,
    film (1 | B, c0 + c1) per stream.  forward = ntm_unet_resblock_forward_save (the inference kernel's body, which also keeps
    y_0 .. y_{n-1}); backward = ntm_unet_resblock_backward (one workgroup per stream: the sources' and FiLM's gradients and
    per-(stream, wave) weight-gradient partials) + ntm_unet_wgrad_reduce (their sum in index order in fp64).  No atomics: equal
    calls give equal bits.  With init_w, src0 is the waveform and takes no gradient.  No double backward."""
    _family = ("ResBlockFn", "whole", "ntm_unet_resblock_")

    @staticmethod
    def forward(ctx, src0, src1, film, w_first, w_gated, w_res, init_w, off0):
        return _resblock_forward(ctx, ResBlockFn._family, src0, src1, film, w_first, w_gated, w_res, init_w, off0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        return _resblock_backward(ctx, ResBlockFn._family, gout)


class ResBlockTiledFn(torch.autograd.Function):
    """ResBlockFn's signature and return values for the TILED form of the block, at any length (the levels of the noise net
    above 1024 frames; a shorter block runs forced through the same windows): forward = ntm_unet_resblock_tiled_forward_save
    (out is the tiled inference forward's bits), backward = ntm_unet_resblock_tiled_backward (one workgroup per (tile, stream) on
    the forward's windows of a tile of 512 frames and 256 of halo a side; gfilm and the weight gradients summed per stream in a
    fixed order) + ntm_unet_wgrad_reduce over the streams.  No atomics: equal calls give equal bits, and a stream's source and
    FiLM gradients do not depend on its batch.  With init_w the waveform takes no gradient.  No double backward."""
    _family = ("ResBlockTiledFn", "tiled", "ntm_unet_resblock_tiled_")

    @staticmethod
    def forward(ctx, src0, src1, film, w_first, w_gated, w_res, init_w, off0):
        return _resblock_forward(ctx, ResBlockTiledFn._family, src0, src1, film, w_first, w_gated, w_res, init_w, off0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        return _resblock_backward(ctx, ResBlockTiledFn._family, gout)


def _grad32(g):
    return None if g is None else g.detach().to(torch.float32).contiguous()


class DownCombineFn(torch.autograd.Function):
    """(x (B, C, F), pyr (B, 1, F), kernel (1, 1, 2 width + S), wc (C, 1, 1), S, width) -> (xo, po): the Downsample(S) +
    CombinerDown step of the diffusion generators' UNet1D (diffusion.down_combine) as ONE graph node.  forward =
    ntm_unet_down_combine, the inference launch, so the outputs are its bits; backward = ntm_unet_down_combine_backward (one
    launch: g_x, g_pyr and the per-stream partials of the combiner weight, summed in fp64 in a fixed order) +
    ntm_unet_wgrad_reduce (the partials over the streams in index order).  An output that nothing reads arrives as no gradient
    and costs nothing; an input that needs no gradient (the top level's pyramid is the network input) is not computed.  No
    gradient goes to the filter, S or width.  No atomics: equal calls give equal bits.  No double backward."""

    @staticmethod
    def forward(ctx, x, pyr, kernel, wc, S, width):
        from . import diffusion as D
        D._require_hip("DownCombineFn", x, pyr, kernel, wc)
        x, pyr, kernel, wc = (t.detach().contiguous() for t in (x, pyr, kernel, wc))
        xo, po = D._bind_down(x.device, x, pyr, kernel, wc, int(S), int(width))(_lib.current_stream())
        ctx.save_for_backward(kernel, wc, po)
        ctx.res = (x.shape, int(S), int(width))
        ctx.set_materialize_grads(False)
        return xo, po

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_xo, g_po):
        kernel, wc, po = ctx.saved_tensors
        (B, C, Fr), S, width = ctx.res
        need, L = ctx.needs_input_grad, _lib.lib()
        if (g_xo is None and g_po is None) or not (need[0] or need[1] or need[3]):
            return None, None, None, None, None, None
        g_xo, g_po = _grad32(g_xo), _grad32(g_po)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=po.device)       # noqa: E731
        g_x = new(B, C, Fr) if need[0] else None
        g_pyr = new(B, 1, Fr) if need[1] else None
        part, g_wc = (new(B, C), new(C)) if need[3] else (None, None)
        _lib.check(L.ntm_unet_down_combine_backward(ptr(po), ptr(kernel), ptr(wc), ptr(g_xo), ptr(g_po), B, C, Fr, S, width,
                                                    kernel.shape[-1], ptr(g_x), ptr(g_pyr), ptr(part), _lib.current_stream()),
                   "ntm_unet_down_combine_backward")
        if part is not None:
            _lib.check(L.ntm_unet_wgrad_reduce(ptr(part), B, C, ptr(g_wc), _lib.current_stream()), "ntm_unet_wgrad_reduce")
            g_wc = g_wc.view(wc.shape)
        return g_x, g_pyr, None, g_wc, None, None


class UpCombineFn(torch.autograd.Function):
    """(x (B, C, F), pyr (B, 1, >= F) | None, kernel (S, 1, 2 width + 1) | None, wc (1, C, 1), S, width) -> (xo | None, po): the
    CombinerUp + Upsample(S) step of the diffusion generators' UNet1D (diffusion.up_combine) as ONE graph node; S = 1 with no
    kernel is the combiner alone, the network's last step, and returns (None, po).  forward = ntm_unet_up_combine, the inference
    launch, so the outputs are its bits; backward = ntm_unet_up_combine_backward (one launch: g_x, g_pyr -- zero behind frame F
    -- and the per-(stream, tile) partials of the combiner weight in fp64) + ntm_unet_wgrad_reduce.  The rules of
    DownCombineFn hold: absent gradients and unwanted outputs cost nothing, the filter, S and width take none, equal calls give
    equal bits, no double backward."""

    @staticmethod
    def forward(ctx, x, pyr, kernel, wc, S, width):
        from . import diffusion as D
        D._require_hip("UpCombineFn", x, pyr, kernel, wc)
        x, wc = x.detach().contiguous(), wc.detach().contiguous()
        pyr, kernel = (None if t is None else t.detach().contiguous() for t in (pyr, kernel))
        xo, po = D._bind_up(x.device, x, pyr, kernel, wc, int(S), int(width))(_lib.current_stream())
        ctx.save_for_backward(x, kernel, wc)
        ctx.res = (int(S), int(width), 0 if pyr is None else pyr.shape[-1])
        ctx.set_materialize_grads(False)
        return xo, po

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_xo, g_po):
        x, kernel, wc = ctx.saved_tensors
        S, width, pyr_T = ctx.res
        B, C, Fr = x.shape
        need, L = ctx.needs_input_grad, _lib.lib()
        if (g_xo is None and g_po is None) or not (need[0] or (need[1] and pyr_T) or need[3]):
            return None, None, None, None, None, None
        g_xo, g_po = _grad32(g_xo), _grad32(g_po)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x.device)        # noqa: E731
        g_x = new(B, C, Fr) if need[0] else None
        g_pyr = new(B, 1, pyr_T) if need[1] and pyr_T else None
        tiles = L.ntm_unet_up_combine_backward_partials(Fr)
        part, g_wc = (new(B * tiles, C), new(C)) if need[3] else (None, None)
        _lib.check(L.ntm_unet_up_combine_backward(ptr(x), ptr(kernel), ptr(wc), ptr(g_xo), ptr(g_po), B, C, Fr, S, width,
                                                  0 if kernel is None else kernel.shape[-1], pyr_T, ptr(g_x), ptr(g_pyr), ptr(part),
                                                  _lib.current_stream()), "ntm_unet_up_combine_backward")
        if part is not None:
            _lib.check(L.ntm_unet_wgrad_reduce(ptr(part), B * tiles, C, ptr(g_wc), _lib.current_stream()), "ntm_unet_wgrad_reduce")
            g_wc = g_wc.view(wc.shape)
        return g_x, g_pyr, None, g_wc, None, None
