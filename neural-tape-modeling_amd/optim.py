"""The optimiser step on the device: FusedAdam and ema_update_ (csrc/multi_tensor.hip behind ntm_multi_* of include/ntm.h).

torch's optimiser machinery runs once per parameter tensor and is bound by its launch count.  Here the gradient norm and clip
of torch.nn.utils.clip_grad_norm_, torch.optim.Adam's step and the EMA of the diffusion trainer each take one launch per
_lib.MULTI_MAX_TENSORS tensors, without a host synchronisation and without atomics: equal steps give equal bits.

  FusedAdam(params, lr, betas, eps)      a torch.optim.Optimizer with torch.optim.Adam's state layout; step(max_grad_norm=...)
  ema_update_(dst_params, src_params, s) dst = dst * s + src * (1 - s) over two parameter lists

There is no fallback: a tensor the kernels do not take (not on a HIP device, not float32, not contiguous, a sparse gradient)
is refused with a RuntimeError that says what is built.
"""
import math

import torch

from . import _lib

_BUILT = "FusedAdam is built for Adam without weight decay: weight_decay == 0, amsgrad=False, maximize=False"
_TAKES = "the HIP kernels take contiguous float32 tensors on a HIP device with dense gradients"


def _refuse(what, t, name):
    """The RuntimeError for a tensor the kernels do not take, or None."""
    if not t.is_cuda:
        return f"{what}: {name} is on {t.device}, not on a HIP device; {_TAKES}"
    if t.dtype != torch.float32:
        return f"{what}: {name} is {t.dtype}; {_TAKES}"
    if t.is_sparse or t.layout != torch.strided:
        return f"{what}: {name} is sparse; {_TAKES}"
    if not t.is_contiguous():
        return f"{what}: {name} is not contiguous; {_TAKES}"
    return None


def _check(what, t, name):
    msg = _refuse(what, t, name)
    if msg:
        raise RuntimeError(msg)


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (weight_decay = 0, amsgrad = False, maximize = False) as HIP launches over lists of tensors.

    The hyper-parameters of a group (lr, betas, eps) are read at every step, so a ramp or a scheduler works as with torch's.
    The state is torch's: state[p] = {"step": 0-dim float32 CPU tensor, "exp_avg", "exp_avg_sq"}, created at a parameter's first
    step with a gradient, so state_dict() / load_state_dict() interchange with torch.optim.Adam in both directions."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam: lr as a Tensor is not built (torch needs capturable=True for it); pass a float")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if weight_decay != 0 or amsgrad or maximize:
            raise ValueError(f"FusedAdam(weight_decay={weight_decay}, amsgrad={amsgrad}, maximize={maximize}): {_BUILT}")
        # torch.optim.Adam's keys, so that a state_dict of either loads into the other with nothing missing
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                                      capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False))
        self._partials = None           # float64 device workspace of the norm, grown on demand

    def _refuse_group(self, group):
        # a loaded state_dict or a caller may have set what the constructor refuses
        if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
            raise ValueError(f"FusedAdam.step: a param group asks for weight_decay={group.get('weight_decay')}, "
                             f"amsgrad={group.get('amsgrad')}, maximize={group.get('maximize')}; {_BUILT}")
        if group.get("capturable", False) or group.get("differentiable", False):
            raise ValueError(f"FusedAdam.step: capturable and differentiable are not built; {_BUILT}")

    @torch.no_grad()
    def step(self, closure=None, *, max_grad_norm=None):
        """One Adam step on every parameter that has a gradient.  With max_grad_norm the gradients are first scaled as one
        clip_grad_norm_(all parameters of all groups, max_grad_norm) call would scale them, and the total norm is returned as a
        0-dim float32 device tensor -- no host synchronisation; without it the return is None.  Parameters whose .grad is None
        are skipped entirely: no state is made for them and they do not enter the norm.  A closure is evaluated first; its
        loss is not returned."""
        if closure is not None:
            with torch.enable_grad():
                closure()
        # everything is checked before any state moves
        todo = []
        for gi, group in enumerate(self.param_groups):
            self._refuse_group(group)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                _check("FusedAdam.step", p, "a parameter")
                _check("FusedAdam.step", g, "a gradient")
                if g.device != p.device or g.shape != p.shape:
                    raise RuntimeError(f"FusedAdam.step: a gradient of shape {tuple(g.shape)} on {g.device} for a parameter of shape "
                                       f"{tuple(p.shape)} on {p.device}")
                st = self.state[p]
                for k in ("exp_avg", "exp_avg_sq") if len(st) else ():
                    _check("FusedAdam.step", st[k], f"the state {k}")
                    if st[k].device != p.device or st[k].shape != p.shape:
                        raise RuntimeError(f"FusedAdam.step: the state {k} does not match its parameter")
                todo.append((gi, p, g, st))
        if not todo:
            return None
        if any(g.device != todo[0][2].device for _, _, g, _ in todo):
            raise RuntimeError("FusedAdam.step: the parameters lie on several devices; one device per optimiser is built")
        # buckets of equal scalars: a group's parameters at one step count
        buckets = {}
        grads = []
        for gi, p, g, st in todo:
            if len(st) == 0:
                st["step"] = torch.zeros((), dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif not torch.is_tensor(st["step"]):
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
            st["step"] += 1
            buckets.setdefault((gi, st["step"].item()), []).append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            grads.append(g)
        device = grads[0].device
        L = _lib.lib()
        norm_coef = None
        with torch.cuda.device(device):
            stream = _lib.current_stream()
            if max_grad_norm is not None:
                n = _lib.i64_array([g.numel() for g in grads])
                need = L.ntm_multi_partials(n, len(grads))
                ws = getattr(self, "_partials", None)     # (absent after unpickling)
                if ws is None or ws.numel() < need or ws.device != device:
                    self._partials = torch.empty(max(need, 1), dtype=torch.float64, device=device)
                norm_coef = torch.empty(2, dtype=torch.float32, device=device)    # fresh: the returned norm is a view of it
                _lib.check(L.ntm_multi_sqnorm(_lib.ptr_array(grads), n, len(grads), _lib.ptr(self._partials), None, stream),
                           "ntm_multi_sqnorm")
                _lib.check(L.ntm_multi_clip_coef(_lib.ptr(self._partials), need, float(max_grad_norm), _lib.ptr(norm_coef), stream),
                           "ntm_multi_clip_coef")
            for (gi, t), entries in buckets.items():
                group = self.param_groups[gi]
                beta1, beta2 = group["betas"]
                # torch's Python scalars, in double; rounded to float32 at the call
                step_size = group["lr"] / (1 - beta1 ** t)
                bc2_sqrt = math.sqrt(1 - beta2 ** t)
                ps, gs, ms, vs = zip(*entries)
                _lib.check(L.ntm_multi_adam(_lib.ptr_array(ps), _lib.ptr_array(gs), _lib.ptr_array(ms), _lib.ptr_array(vs),
                                            _lib.i64_array([p.numel() for p in ps]), len(ps), _lib.ptr(norm_coef), step_size, bc2_sqrt,
                                            1 - beta1, beta2, 1 - beta2, group["eps"], stream), "ntm_multi_adam")
                # the kernels wrote behind torch's back: the caches keyed on _version and autograd's in-place check must see it
                torch.autograd.graph.increment_version(ps + ms + vs + (gs if norm_coef is not None else ()))
        return None if norm_coef is None else norm_coef[0]


@torch.no_grad()
def ema_update_(dst_params, src_params, s):
    """dst = dst * s + src * (1 - s) for every pair, float32(s) and float32(1 - s) from the host's doubles: the arithmetic of the
    reference's `dst.copy_(dst * s + src * (1 - s))`, one launch per _lib.MULTI_MAX_TENSORS tensors."""
    dst, src = list(dst_params), list(src_params)
    if len(dst) != len(src):
        raise ValueError(f"ema_update_: {len(dst)} destinations for {len(src)} sources")
    if not dst:
        return
    for d, q in zip(dst, src):
        _check("ema_update_", d, "a destination")
        _check("ema_update_", q, "a source")
        if d.shape != q.shape or d.device != q.device or d.device != dst[0].device:
            raise RuntimeError("ema_update_: a destination and its source differ in shape or device (one device per call)")
    s = float(s)
    with torch.cuda.device(dst[0].device):
        _lib.check(_lib.lib().ntm_multi_ema(_lib.ptr_array(dst), _lib.ptr_array(src), _lib.i64_array([d.numel() for d in dst]),
                                            len(dst), s, 1 - s, _lib.current_stream()), "ntm_multi_ema")
    torch.autograd.graph.increment_version(dst)
