"""The diffusion generators of the reference (`DiffusionGenerator`, code/model.py:656-891, on `UNet1D`,
code/networks/unet_1d.py): the wow-and-flutter delay trajectories that drive DiffDelRNN and the tape hiss added to its output.

  load_config(name)            configs/conf_{noise,trajectories,toytrajectories}.yaml as plain data with attribute access
  UNet1D(args, device)         the reference's parameters and buffers under the reference's state_dict keys;
                               _walk: the network's data flow, written once; forward_torch: it in torch ops (this project's
                               restatement, any dtype, any device); forward: it as launches of csrc/unet_kernels.hip bound once
                               per (B, T), HIP device only; record= of either reports the same names from the path that ran
                               forward_train: it as a differentiable graph whose ResnetBlocks are HIP nodes at any length
                               (training.ResBlockFn up to 1024 frames, training.ResBlockTiledFn above, on
                               csrc/unet_train.hip) and whose resample + combine steps are HIP
                               nodes at any length (training.DownCombineFn / UpCombineFn on csrc/unet_resample_train.hip);
                               FiLM and the embedding are torch ops under autograd
  down_combine / up_combine    one resample + combine step on the device; differentiable (the same nodes) when an operand
                               requires a gradient
  DiffusionGenerator(args, device)   the EDM sampler with the reference's attributes and methods; sampler="one_launch" (opt-in)
                               runs a whole sampler whose levels all fit one workgroup as ONE launch (csrc/unet_sampler.hip), bit
                               for bit what the default step-by-step path gives
  EDMTrainer(args, network, optimizer, device, backend)   the EDM training step and EMA of code/train-diffusion.py

The sampler and `forward` are inference only.  Two additions to the reference's protocol, both keyword arguments:
  draws=   an iterator of (B, seg_len) tensors that stands in for torch.randn, in the reference's draw order for one sample
           (the first latent; then per step the extra noise where gamma != 0, then the outpainting noise);
  sample_batch(B) / sample_long(Length, batch=B) run B independent samples through every launch together where the reference
           loops over them: the draw order then differs from the reference's loop, the distribution does not, and with draws=
           given per stream every stream equals its own sample() bit for bit.
"""
import copy
import glob
import math
import os
import pickle
import re
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, optim

SUPPORTED = "fp32 on a HIP device, Nin = 1, c_in <= 32, c_out <= 16, at most 8 gated layers, use_norm = False"
WHOLE_MAX_T, TILE = 1024, 512      # include/ntm.h NTM_UNET_WHOLE_MAX_T, NTM_UNET_TILE
FORMS = {"auto": 0, "whole": 1, "tiled": 2}

# ---- configurations: configs/conf_*.yaml restated ------------------------------------------------------------------------------

_TRAIN = {"optimizer": {"type": "adam", "beta1": 0.9, "beta2": 0.999, "eps": 1e-8}, "lr": 2e-4, "lr_rampup_it": 1000,
          "scheduler_step_size": 10000, "batch": 4, "scheduler_gamma": 0.8, "save_model": True, "save_interval": 10000,
          "resume": False, "use_grad_clip": True, "max_grad_norm": 1.0, "ema_rampup": 1000, "ema_rate": 0.999}
_HYDRA = {"job": {"config": {"override_dirname": {"kv_sep": "=", "item_sep": ",",
                                                  "exclude_keys": ["path_experiment", "hydra.job_logging.handles.file.filename"]}}}}
_TRAJ_NET = {"name": "unet_1d", "callable": "networks.unet_1d.UNet1D", "Nin": 1, "depth": 4, "Ns": [8, 16, 16, 16, 16, 16],
             "Ss": [2, 2, 4, 4, 4], "emb_dim": 16, "num_bottleneck_layers": 1, "use_norm": False}
_CONFIGS = {
    "noise": {
        "train": _TRAIN,
        "dset": {"callable": "datasets.tapehiss.TapeHissdset", "path": "../audio/Silence_AKAI_IPS[7.5]_MAXELL_SPLIT/Train",
                 "fs": 44100, "seg_len": 65536, "num_workers": 2},
        "model_dir": "../weights/83",
        "network": {"checkpoint": "../weights/83/noise-73000.pt", "name": "unet_1d", "callable": "networks.unet_1d.UNet1D",
                    "Nin": 1, "depth": 8, "emb_dim": 32, "Ns": [8, 16, 16, 16, 16, 16, 16, 16, 16],
                    "Ss": [4, 4, 4, 4, 4, 4, 4, 4, 4], "use_norm": False},
        "exp": {"exp_name": "noise_diffusion", "sample_rate": 44100, "out_sample_rate": 44100, "seg_len": 65536},
        "diff_params": {"T": 16, "sigma_data": 8e-4, "sigma_min": 5e-5, "sigma_max": 0.1, "ro": 10, "Schurn": 0.25,
                        "Snoise": 1.0},
        "outpainting": {"overlap": 0.2},
        "hydra": _HYDRA,
    },
    "trajectories": {
        "train": _TRAIN,
        "dset": {"callable": "datasets.tapehiss.TapeHissdset",
                 "path": "../audio/ReelToReel_Dataset_Mini192kHzPulse100_AKAI_IPS[7.5]_MAXELL_TRAJECTORIES_SPLIT/Train",
                 "fs": 192000, "seg_len": 983040, "num_workers": 2},
        "model_dir": "../weights/91",
        "network": dict(_TRAJ_NET, checkpoint="../weights/91/trajectories-41000.pt"),
        "exp": {"exp_name": "trajectories", "sample_rate": 100, "out_sample_rate": 44100, "seg_len": 512},
        "diff_params": {"T": 8, "sigma_data": 1e-4, "sigma_min": 1e-5, "sigma_max": 1e-2, "ro": 7, "Schurn": 0, "Snoise": 1},
        "outpainting": {"overlap": 1},
        "hydra": _HYDRA,
    },
    "toytrajectories": {
        "train": _TRAIN,
        "dset": {"callable": "datasets.tapehiss.TapeHissdset",
                 "path": "../audio/ReelToReel_Dataset_MiniPulse100_CHOWTAPE_F[0.6]_SL[60]_TRAJECTORIES/Train",
                 "fs": 44100, "seg_len": 225792, "num_workers": 2},
        "model_dir": "../weights/90",
        "network": dict(_TRAJ_NET, checkpoint="../weights/90/toytrajectories-36000.pt"),
        "exp": {"exp_name": "toytrajectories", "sample_rate": 100, "out_sample_rate": 44100, "seg_len": 512},
        "diff_params": {"T": 4, "sigma_data": 0.0068, "sigma_min": 1e-5, "sigma_max": 0.5, "Schurn": 0, "Snoise": 1, "ro": 7},
        "outpainting": {"overlap": 1},
        "hydra": _HYDRA,
    },
}


class Config(dict):
    """A dict whose keys are attributes too (args.network.depth), the way the reference reads its OmegaConf objects."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    def __setattr__(self, k, v):
        self[k] = v


_FLOAT = re.compile(r"[-+]?(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?$")


def _wrap(v):
    # PyYAML reads `8e-4` (no dot) as a string where OmegaConf, which the reference loads these files with, reads a float
    if isinstance(v, str) and _FLOAT.match(v):
        return float(v)
    if isinstance(v, dict):
        return Config({k: _wrap(x) for k, x in v.items()})
    if isinstance(v, (list, tuple)):
        return [_wrap(x) for x in v]
    return v


def load_config(name):
    """"noise" | "trajectories" | "toytrajectories" -> that configuration of the reference as data (a fresh copy every call);
    any other string is the path of a YAML file of the same layout, read with PyYAML."""
    if name in _CONFIGS:
        return _wrap(_CONFIGS[name])
    if not os.path.isfile(name):
        raise ValueError(f"load_config: {name!r} is neither one of {sorted(_CONFIGS)} nor a YAML file")
    import yaml
    with open(name) as f:
        return _wrap(yaml.safe_load(f))


# ---- torchaudio's polyphase filters ----------------------------------------------------------------------------------------------

def sinc_resample_kernel(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """torchaudio's published `_get_sinc_resample_kernel` (sinc_interp_hann) for the reduced ratio orig -> new: the
    (new, 1, 2 width + orig) float32 filter bank, computed in float64, and its width."""
    g = math.gcd(int(orig), int(new))
    orig, new = int(orig) // g, int(new) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    kernels = kernels * window * (base / orig)
    return kernels.to(torch.float32), width


def apply_resample_kernel(x, kernel, orig, new, width):
    """torchaudio's `_apply_sinc_resample_kernel`: pad (width, width + orig), conv1d of stride orig with the `new` phases,
    interleave, trim to ceil(new F / orig).  x (..., F)."""
    shape, length = x.shape, x.shape[-1]
    w = F.pad(x.reshape(-1, length), (width, width + orig))
    r = F.conv1d(w[:, None], kernel.to(x.dtype), stride=orig)
    r = r.transpose(1, 2).reshape(w.shape[0], -1)
    return r[..., :int(math.ceil(new * length / orig))].reshape(shape[:-1] + (-1,))


class _Resample(nn.Module):
    """What torchaudio.transforms.Resample(orig, new) leaves in a state_dict: the `kernel` buffer."""

    def __init__(self, orig, new):
        super().__init__()
        g = math.gcd(orig, new)
        self.orig, self.new = orig // g, new // g
        kernel, self.width = sinc_resample_kernel(self.orig, self.new)
        self.register_buffer("kernel", kernel)

    def forward(self, x):
        return apply_resample_kernel(x, self.kernel, self.orig, self.new, self.width)


class Upsample(nn.Module):
    def __init__(self, S):
        super().__init__()
        self.S = int(S)
        self.resample = _Resample(1, self.S)

    def forward(self, x):
        return self.resample(x)


class Downsample(nn.Module):
    def __init__(self, S):
        super().__init__()
        self.S = int(S)
        self.resample = _Resample(self.S, 1)

    def forward(self, x):
        return self.resample(x)


# ---- the network -------------------------------------------------------------------------------------------------------------------

class RFF_MLP_Block(nn.Module):
    def __init__(self, emb_dim):
        super().__init__()
        self.RFF_freq = nn.Parameter(16 * torch.randn([1, 16]), requires_grad=False)
        self.MLP = nn.ModuleList([nn.Linear(32, emb_dim), nn.Linear(emb_dim, emb_dim)])

    def forward(self, sigma):
        table = 2 * np.pi * sigma * self.RFF_freq
        x = torch.cat([torch.sin(table), torch.cos(table)], dim=1)
        for layer in self.MLP:
            x = F.relu(layer(x))
        return x


class Film(nn.Module):
    # the reference's Film(bias=False) drops beta, not the Linear's own bias: gamma = W emb + b
    def __init__(self, output_dim, emb_dim):
        super().__init__()
        self.output_layer = nn.Linear(emb_dim, output_dim)

    def forward(self, emb):
        return self.output_layer(emb).unsqueeze(-1)


class GatedResidualLayer(nn.Module):
    def __init__(self, dim, kernel_size, dilation):
        super().__init__()
        self.conv = nn.Conv1d(dim, dim, kernel_size=kernel_size, dilation=dilation, stride=1, padding="same",
                              padding_mode="zeros", bias=False)
        self.act = nn.GELU()

    def forward(self, x):
        return (x + self.conv(self.act(x))) / (2 ** 0.5)


class ResnetBlock(nn.Module):
    def __init__(self, dim, dim_out, emb_dim, num_dils=8):
        super().__init__()
        self.dim, self.dim_out, self.num_layers = dim, dim_out, num_dils
        self.film = Film(dim, emb_dim)
        self.res_conv = nn.Conv1d(dim, dim_out, 1, bias=False) if dim != dim_out else nn.Identity()
        self.first_conv = nn.Sequential(nn.GELU(), nn.Conv1d(dim, dim_out, 1, bias=False))
        self.H = nn.ModuleList([GatedResidualLayer(dim_out, 5, 2 ** i) for i in range(num_dils)])

    def forward(self, x, emb):
        x = x * self.film(emb)
        y = self.first_conv(x)
        for h in self.H:
            y = h(y)
        return (y + self.res_conv(x)) / (2 ** 0.5)


class CombinerUp(nn.Module):
    def __init__(self, Npyr, Nx):
        super().__init__()
        self.conv1x1 = nn.Conv1d(Nx, Npyr, 1, bias=False)
        torch.nn.init.constant_(self.conv1x1.weight, 0)

    def forward(self, pyr, x):
        x = self.conv1x1(x)
        return x if pyr is None else (pyr[..., 0:x.shape[-1]] + x) / (2 ** 0.5)


class CombinerDown(nn.Module):
    def __init__(self, Nin, Nout):
        super().__init__()
        self.conv1x1 = nn.Conv1d(Nin, Nout, 1, bias=False)

    def forward(self, pyr, x):
        return (self.conv1x1(pyr) + x) / (2 ** 0.5)


BlockSpec = _lib.UnetBlock       # include/ntm.h ntm_unet_block
SAMPLERS = ("steps", "one_launch")


def _require_hip(what, *tensors):
    for t in tensors:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError(f"{what}: HIP device only (no CPU fallback), fp32; supported: {SUPPORTED}")


class _Call:
    """One C call with its arguments bound: `args` in the entry point's order with the stream last, `slot` the positions by name
    of the pointers a plan patches, `out` what the call writes, `ws` its workspace, `launches` the kernels it starts."""

    def __init__(self, name, args, slot, out, ws=None, launches=1, spec=None):
        self.name, self.fn, self.args, self.slot = name, getattr(_lib.lib(), name), args, slot
        self.out, self.ws, self.launches, self.spec = out, ws, launches, spec

    def __call__(self, stream):
        self.args[-1] = stream
        _lib.check(self.fn(*self.args), self.name)
        return self.out


def _addr(t):
    """The pointer to bind for t.  A tensor on the meta device stands for an operand whose pointer comes per evaluation (it has
    the shape and the strides, no storage): it binds as null, like no tensor, and a null left unpatched is refused by the C side."""
    return None if t is None or t.device.type == "meta" else t.data_ptr()


def _bind_resblock(dev, src0, film, w_first, w_gated, w_res=None, src1=None, off0=0, frames=None, init_w=None, form="auto"):
    """ntm_unet_resblock_forward on resblock_forward's operands, with its block description, workspace and output made on dev."""
    B, T0 = src0.shape[0], src0.shape[2]
    c0 = init_w.shape[0] if init_w is not None else src0.shape[1]
    T = int(frames) if frames is not None else (src1.shape[2] if src1 is not None else T0 - off0)
    c1, T1 = (0, 0) if src1 is None else src1.shape[1:]
    spec = BlockSpec(c0, c1, w_first.shape[0], w_gated.shape[0], T, T0, off0, T1, 0, int(init_w is not None), FORMS[form])
    n = _lib.lib().ntm_unet_resblock_workspace_floats(B, _lib.ctypes.byref(spec))
    if n < 0:
        raise _lib.NtmError(f"ntm_unet_resblock_workspace_floats refused: {_lib.lib().ntm_last_error().decode()}")
    ws = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    out = torch.empty(B, spec.c_out, T, dtype=torch.float32, device=dev)
    assert src0.is_contiguous() and (src1 is None or src1.is_contiguous()) and film.stride(-1) == 1
    args = [_addr(src0), _addr(src1), _addr(init_w), _addr(film), 0 if film.shape[0] == 1 else film.stride(0), _addr(w_first),
            _addr(w_gated), _addr(w_res), B, _lib.ctypes.byref(spec), _addr(ws), _addr(out), None]
    # above NTM_UNET_WHOLE_MAX_T the tiled form runs the eight dilations in two launches
    return _Call("ntm_unet_resblock_forward", args, {"src0": 0, "film": 3}, out, ws, launches=2 if T > WHOLE_MAX_T else 1, spec=spec)


def _bind_down(dev, x, pyr, kernel, wc, S, width):
    """ntm_unet_down_combine on down_combine's operands, with its two outputs made on dev."""
    B, C, Fr = x.shape
    xo, po = (torch.empty(B, c, -(-Fr // S), dtype=torch.float32, device=dev) for c in (C, 1))
    assert x.is_contiguous() and pyr.is_contiguous()
    args = [_addr(x), _addr(pyr), _addr(kernel), _addr(wc), B, C, Fr, S, width, kernel.shape[-1], _addr(xo), _addr(po), None]
    return _Call("ntm_unet_down_combine", args, {"pyr": 1}, (xo, po))


def _bind_up(dev, x, pyr, kernel, wc, S, width, po=None):
    """ntm_unet_up_combine on up_combine's operands, with its outputs made on dev; po: takes the pyramid instead of a new tensor."""
    B, C, Fr = x.shape
    xo = torch.empty(B, C, S * Fr, dtype=torch.float32, device=dev) if S > 1 else None
    if po is None:
        po = torch.empty(B, 1, S * Fr, dtype=torch.float32, device=dev)
    assert x.is_contiguous() and (pyr is None or pyr.is_contiguous())
    args = [_addr(x), _addr(pyr), 0 if pyr is None else pyr.shape[-1], _addr(kernel), _addr(wc), B, C, Fr, S, width,
            0 if kernel is None else kernel.shape[-1], _addr(xo), _addr(po), None]
    return _Call("ntm_unet_up_combine", args, {"po": 12}, (xo, po))


def resblock_forward(src0, film, w_first, w_gated, w_res=None, src1=None, off0=0, frames=None, init_w=None, form="auto"):
    """One fused ResnetBlock on the device (ntm_unet_resblock_forward).
    src0 (B, c0, T0), read from frame off0; src1 (B, c1, frames) or None: the second half of the concatenation.  With init_w
    (c0, 1, 5), src0 is the (B, 1, T0) waveform and its c0 channels are Conv1d(1, c0, 5, "same") of it.  film (1 | B, c0 + c1);
    w_first (c_out, c0 + c1, 1); w_gated (n, c_out, c_out, 5), layer l at dilation 2^l; w_res (c_out, c0 + c1, 1) or None (identity).
    form "auto" | "whole" (one workgroup per stream, T <= 1024) | "tiled".  -> (B, c_out, frames)."""
    _require_hip("resblock_forward", src0, src1, film, w_first, w_gated, w_res, init_w)
    return _bind_resblock(src0.device, src0, film, w_first, w_gated, w_res, src1, off0, frames, init_w, form)(_lib.current_stream())


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def down_combine(x, pyr, kernel, wc, S, width):
    """Downsample(S) of x (B, C, F) and pyr (B, 1, F) with the (1, 1, 2 width + S) filter, then CombinerDown:
    -> ((conv1x1(pyr_d) + x_d) / sqrt 2, pyr_d), both ceil(F / S) frames (ntm_unet_down_combine).  With grad mode on and x, pyr
    or wc requiring a gradient the same launch runs as a graph node (training.DownCombineFn): same bits, differentiable."""
    _require_hip("down_combine", x, pyr, kernel, wc)
    if _wants_grad(x, pyr, wc):
        from .training import DownCombineFn
        return DownCombineFn.apply(x, pyr, kernel, wc, S, width)
    return _bind_down(x.device, x.contiguous(), pyr.contiguous(), kernel, wc, S, width)(_lib.current_stream())


def up_combine(x, pyr, kernel, wc, S, width):
    """CombinerUp then Upsample(S): p = conv1x1(x), or (pyr[..., :F] + conv1x1(x)) / sqrt 2 with a pyramid (B, 1, >= F);
    -> (x, p) both upsampled to S F frames with the (S, 1, 2 width + 1) filter bank.  S = 1 (kernel None): -> (None, p), no
    resampling -- the last level (ntm_unet_up_combine).  With grad mode on and x, pyr or wc requiring a gradient the same launch
    runs as a graph node (training.UpCombineFn): same bits, differentiable."""
    _require_hip("up_combine", x, pyr, kernel, wc)
    if _wants_grad(x, pyr, wc):
        from .training import UpCombineFn
        return UpCombineFn.apply(x, pyr, kernel, wc, S, width)
    return _bind_up(x.device, x.contiguous(), None if pyr is None else pyr.contiguous(), kernel, wc, S, width)(_lib.current_stream())


class _TorchWalk:
    """UNet1D._walk in torch ops: the module calls."""

    def __init__(self, net, emb, record):
        self.init_conv, self.emb, self.record = net.init_conv, emb, record or (lambda name, t: None)
        self.given = record is not None

    def rec(self, name, t):
        self.record(name, t)
        return t

    def block(self, k, name, blk, x, skip=None, off=0, first=False):
        if first:
            x = self.init_conv(x)
        if skip is not None:
            x = torch.cat((x[:, :, off:off + skip.shape[2]], skip), 1)
        return self.rec(name, blk(x, self.emb))

    def down(self, name, down, comb, x, pyr):
        x, pyr = down(x), down(pyr)
        return self.rec(name, comb(pyr, x)), pyr

    def up(self, name, up, comb, x, pyr):
        pyr = self.rec(name, comb(pyr, x))
        return up(x), up(pyr)

    def final(self, name, comb, x, pyr):
        return self.rec(name, comb(pyr, x).squeeze(1))


class _TrainWalk(_TorchWalk):
    """UNet1D._walk for training: a ResnetBlock is ONE autograd node on the HIP kernels -- training.ResBlockFn
    (ntm_unet_resblock_forward_save / _backward, the whole form) up to WHOLE_MAX_T frames, training.ResBlockTiledFn
    (ntm_unet_resblock_tiled_forward_save / _backward) above, the upper levels of the noise net.  tiled_blocks = False sends the
    longer blocks to the torch module instead (what tools/diffusion_train_probe.py times the tiled node against).  Every resample + combine step, at any length, is ONE node too (training.DownCombineFn / UpCombineFn: the
    inference launches ntm_unet_down_combine / ntm_unet_up_combine forward, their adjoints backward), the last step the
    S = 1 form of the up node.  FiLM and the embedding stay torch ops under autograd.  The block node reads the
    parameters themselves -- the gated weights stacked anew on every call, so that autograd routes the stack's gradient to the
    eight layers -- never _pack()'s copy."""

    tiled_blocks = True

    def block(self, k, name, blk, x, skip=None, off=0, first=False):
        frames = skip.shape[2] if skip is not None else x.shape[2]
        if frames > WHOLE_MAX_T and not self.tiled_blocks:
            return super().block(k, name, blk, x, skip, off, first)
        from .training import ResBlockFn, ResBlockTiledFn
        res = None if isinstance(blk.res_conv, nn.Identity) else blk.res_conv.weight
        w_gated = torch.stack([h.conv.weight for h in blk.H])
        node = ResBlockTiledFn if frames > WHOLE_MAX_T else ResBlockFn
        out = node.apply(x, skip, blk.film.output_layer(self.emb), blk.first_conv[1].weight, w_gated, res,
                               self.init_conv.weight if first else None, off)
        return self.rec(name, out)

    def down(self, name, down, comb, x, pyr):
        from .training import DownCombineFn
        r = down.resample
        xo, po = DownCombineFn.apply(x, pyr, r.kernel, comb.conv1x1.weight, r.orig, r.width)
        return self.rec(name, xo), po

    def up(self, name, up, comb, x, pyr):
        from .training import UpCombineFn
        r, wc = up.resample, comb.conv1x1.weight
        if self.given:            # the CombinerUp output before upsampling: the fused node never materialises it (_Plan.up)
            with torch.no_grad():
                self.record(name, UpCombineFn.apply(x, pyr, None, wc, 1, 0)[1])
        return UpCombineFn.apply(x, pyr, r.kernel, wc, r.new, r.width)

    def final(self, name, comb, x, pyr):
        from .training import UpCombineFn
        return self.rec(name, UpCombineFn.apply(x, pyr, None, comb.conv1x1.weight, 1, 0)[1].squeeze(1))


class _Plan:
    """The launches of one evaluation for a (B, T), bound once: UNet1D._walk drives block / down / up / final, which allocate
    every intermediate and bind every call, nothing runs.  run() then patches the pointers named here and loops over ready calls
    (the sampler runs 4 to 16 evaluations per sample and a launch is ~10 us: the host must not be the slow side).  The input, the
    FiLM rows and the output are meta tensors while binding (_addr).  Two streams running one plan would share its buffers."""

    def __init__(self, net, B, T, per_stream, dev):
        _, (w, _), self.offs, self.gated = net._pack()
        self.init_w, self.dev = net.init_conv.weight, dev
        self.x = torch.empty(B, 1, T, device="meta")
        self.film = torch.empty(B if per_stream else 1, w.shape[0], device="meta")
        self.calls = []                    # the evaluation, in launch order
        self.inputs, self.films, self.output = [], [], None   # (args, position[, byte offset into the FiLM row]) to patch
        self.buffers = {}                  # record name -> the tensor that holds it after a run, in network order
        self.record_calls = []             # fill the buffers that the evaluation itself never materialises ("ups.i.2")

    @property
    def launches(self):
        return sum(c.launches for c in self.calls)

    def run(self, inputs, films, out, stream):
        src, fbase = inputs.data_ptr(), films.data_ptr()
        for args, pos in self.inputs:
            args[pos] = src
        for args, pos, off in self.films:
            args[pos] = fbase + off
        args, pos = self.output
        args[pos] = out.data_ptr()
        for call in self.calls:                                   # _Call.__call__ written out: no frame per launch
            call.args[-1] = stream
            _lib.check(call.fn(*call.args), call.name)

    def stages(self):
        """The evaluation as records of the one-launch sampler's table (_lib.UnetStage, include/ntm.h ntm_unet_stage), in launch
        order.  They are read off `calls`, the list run() launches, so the two sampler modes cannot list different calls.  What
        run() patches per evaluation -- the input, the FiLM rows, the output -- is null in a record: the kernel puts the
        network's input, the step's FiLM row (from film_off) and the network's output there."""
        patched = {(id(a), pos) for a, pos in self.inputs} | {(id(self.output[0]), self.output[1])}
        kinds, out = _lib.USTAGE_KINDS, []
        for c in self.calls:
            a = [None if (id(c.args), i) in patched else v for i, v in enumerate(c.args)]
            if c.name == "ntm_unet_resblock_forward":
                st = _lib.UnetStage(kind=kinds["block"], film_off=c.film_off, blk=c.spec, a=a[0], b=a[1], w3=a[2], w0=a[5],
                                    w1=a[6], w2=a[7], o0=a[11])
            elif c.name == "ntm_unet_down_combine":
                st = _lib.UnetStage(kind=kinds["down"], a=a[0], b=a[1], w0=a[2], w1=a[3], C=a[5], F=a[6], S=a[7], width=a[8],
                                    taps=a[9], o0=a[10], o1=a[11])
            else:
                assert c.name == "ntm_unet_up_combine", c.name
                st = _lib.UnetStage(kind=kinds["final" if c is self.calls[-1] else "up"], a=a[0], b=a[1], pyr_T=a[2], w0=a[3],
                                    w1=a[4], C=a[6], F=a[7], S=a[8], width=a[9], taps=a[10], o0=a[11], o1=a[12])
            out.append(st)
        return out

    def add(self, name, call, buf):
        self.calls.append(call)
        self.buffers[name] = buf
        return buf

    def block(self, k, name, blk, x, skip=None, off=0, first=False):
        o = self.offs[k]
        res = None if isinstance(blk.res_conv, nn.Identity) else blk.res_conv.weight
        call = _bind_resblock(self.dev, x, self.film[:, o:o + blk.dim], blk.first_conv[1].weight, self.gated[k], res, skip, off,
                              init_w=self.init_w if first else None)
        self.films.append((call.args, call.slot["film"], 4 * o))
        call.film_off = o
        if x is self.x:
            self.inputs.append((call.args, call.slot["src0"]))
        return self.add(name, call, call.out)

    def down(self, name, down, comb, x, pyr):
        r = down.resample
        call = _bind_down(self.dev, x, pyr, r.kernel, comb.conv1x1.weight, r.orig, r.width)
        if pyr is self.x:
            self.inputs.append((call.args, call.slot["pyr"]))
        return self.add(name, call, call.out[0]), call.out[1]

    def up(self, name, up, comb, x, pyr):
        r, wc = up.resample, comb.conv1x1.weight
        # the CombinerUp output before upsampling: the fused call never materialises it, a combiner-only call does for record=
        self.record_calls.append(_bind_up(self.dev, x, pyr, None, wc, 1, 0))
        self.buffers[name] = self.record_calls[-1].out[1]
        self.calls.append(_bind_up(self.dev, x, pyr, r.kernel, wc, r.new, r.width))
        return self.calls[-1].out

    def final(self, name, comb, x, pyr):
        out = torch.empty(x.shape[0], x.shape[2], device="meta")
        call = _bind_up(self.dev, x, pyr, None, comb.conv1x1.weight, 1, 0, po=out)
        self.output = (call.args, call.slot["po"])
        return self.add(name, call, out)


class UNet1D(nn.Module):
    """The reference's UNet1D: same tree, same state_dict keys (load_state_dict(checkpoint["ema"], strict=True) works and
    replaces the recomputed resample filters with the checkpoint's own).  Up-path factors come from Ss[i] as in the reference."""

    def __init__(self, args, device):
        super().__init__()
        net = args.network
        if net.use_norm:
            raise ValueError("UNet1D: use_norm=True is not supported (no shipped configuration uses the GroupNorm); "
                             f"supported: {SUPPORTED}")
        if net.Nin != 1:
            raise ValueError(f"UNet1D: Nin = {net.Nin}; supported: {SUPPORTED}")
        self.args, self.device = args, device
        self.depth, self.emb_dim, self.use_norm = net.depth, net.emb_dim, False
        self.Ns, self.Ss = list(net.Ns), list(net.Ss)
        Ns, Ss, depth, E = self.Ns, self.Ss, self.depth, self.emb_dim
        self.embedding = RFF_MLP_Block(E)
        self.init_conv = nn.Conv1d(1, Ns[0], 5, padding="same", padding_mode="zeros", bias=False)
        self.downs, self.middle, self.ups = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for i in range(depth):
            dim_in, dim_out = Ns[max(i - 1, 0)], Ns[i]
            mods = [ResnetBlock(dim_in, dim_out, E)]
            if i < depth - 1:
                mods += [Downsample(Ss[i]), CombinerDown(1, dim_out)]
            self.downs.append(nn.ModuleList(mods))
        self.middle.append(nn.ModuleList([ResnetBlock(Ns[depth], Ns[depth], E)]))
        for i in range(depth - 1, -1, -1):
            dim_in, dim_out = Ns[i] * 2, Ns[max(i - 1, 0)]
            mods = [ResnetBlock(dim_in, dim_out, E)]
            if i > 0:
                mods += [Upsample(Ss[i]), CombinerUp(1, dim_out)]
            self.ups.append(nn.ModuleList(mods))
        self.to(device)
        self._packed, self._plans = None, {}

    def setup_CQT_len(self, len):
        pass

    def _apply(self, fn, *a, **k):
        self._packed, self._plans = None, {}
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed, self._plans = None, {}
        return super().load_state_dict(*a, **k)

    def _walk(self, be, x):
        """The data flow of the network, written once, over a backend `be` that says what a step is (_TorchWalk: module
        calls; _Plan: bound launches).  x (B, 1, T) -> what be.final returns.  be.block(k, name, blk, x, skip, off, first):
        ResnetBlock k of _pack()'s order on x -- through init_conv if first; with a skip, on x cropped to the skip's frames
        from frame `off` (CropConcatBlock's centre crop) and concatenated with it; be.down / be.up(name, resampler, combiner,
        x, pyr) -> (x, pyr) of the next level; `name` is the module name the result is recorded under."""
        frames, hs, k = x.shape[2], [], 0
        pyr = x
        for i, mods in enumerate(self.downs):
            x = be.block(k, f"downs.{i}.0", mods[0], x, first=i == 0)
            k += 1
            hs.append(x)
            if len(mods) == 3:
                x, pyr = be.down(f"downs.{i}.2", mods[1], mods[2], x, pyr)
        x = be.block(k, "middle.0.0", self.middle[0][0], x)
        k += 1
        pyr = None
        for i, mods in enumerate(self.ups):
            skip = hs.pop()
            off = (x.shape[2] - skip.shape[2]) // 2
            if off < 0:
                raise ValueError(f"UNet1D: the up path carries {x.shape[2]} frames into a skip of {skip.shape[2]}: nothing to crop")
            x = be.block(k, f"ups.{i}.0", mods[0], x, skip, off)
            k += 1
            if len(mods) == 3:
                x, pyr = be.up(f"ups.{i}.2", mods[1], mods[2], x, pyr)
        assert x.shape[2] == frames, "bad shapes"
        return be.final("final", self._final_combiner(), x, pyr)

    # The reference's last level calls `combiner(pyr, x)` with the combiner left over from the level before (the loop variable
    # of code/networks/unet_1d.py:163-183): ups[depth - 2][2].
    def _final_combiner(self):
        if self.depth < 2:
            raise ValueError("UNet1D: depth >= 2 (the last level reuses the combiner of the level before, as the reference does)")
        return self.ups[self.depth - 2][2]

    def level_lengths(self, T):
        """Frames of the network's levels for an input of T frames, top first: the lengths of its ResnetBlocks."""
        out = [int(T)]
        for S in self.Ss[:self.depth - 1]:
            out.append(-(-out[-1] // S))
        return out

    # -- the torch path --
    def forward_torch(self, inputs, sigma, record=None):
        """The network in torch ops.  record(name, tensor), if given, sees every ResnetBlock's and combiner's output under
        its module name ("downs.0.0", "downs.0.2", ..., "ups.3.0", "final")."""
        return self._walk(_TorchWalk(self, self.embedding(sigma), record), inputs.unsqueeze(1))

    # -- the training path --
    def forward_train(self, inputs, sigma, record=None):
        """The network as a differentiable graph whose ResnetBlocks, of any length, are HIP nodes (_TrainWalk):
        inputs (B, T), sigma (1 | B, 1) per stream -> (B, T).  HIP device only; `forward` (inference, bound plans) is
        untouched by it."""
        if not inputs.is_cuda:
            raise RuntimeError(f"UNet1D.forward_train: HIP device only (no CPU fallback); use forward_torch.  Supported: {SUPPORTED}")
        emb = self.embedding(sigma.reshape(-1, 1).float())
        if emb.shape[0] not in (1, inputs.shape[0]):
            raise ValueError(f"UNet1D.forward_train: sigma has {emb.shape[0]} rows for a batch of {inputs.shape[0]}")
        return self._walk(_TrainWalk(self, emb, record), inputs.float().unsqueeze(1))

    # -- the HIP path --
    def _versions(self):
        """What _pack()'s copies and the plans bound to them depend on: every parameter's storage and its in-place version
        counter, which an optimiser's step or any `p.add_()` moves."""
        return tuple((p._version, p.data_ptr()) for p in self.parameters())

    def _pack(self):
        """The parameters in the layouts the kernels read, gathered once per state of the parameters (_versions): per block
        the stacked gated weights; all FiLM matrices as one so that one matmul gives every block's vector.  A changed
        parameter drops the copies and the plans that hold their addresses."""
        versions = self._versions()
        if self._packed is not None and self._packed_versions != versions:
            self._packed, self._plans = None, {}
        if self._packed is None:
            self._packed_versions = versions
            blocks = [m for m in self.modules() if isinstance(m, ResnetBlock)]      # registration order: the order of _walk
            films = (torch.cat([b.film.output_layer.weight for b in blocks], 0).float().contiguous(),
                     torch.cat([b.film.output_layer.bias for b in blocks], 0).float().contiguous())
            offs, o = [], 0
            for b in blocks:
                offs.append(o)
                o += b.dim
            gated = [torch.stack([h.conv.weight for h in b.H]).float().contiguous() for b in blocks]
            self._packed = (blocks, films, offs, gated)
        return self._packed

    def films(self, sigma):
        """Every block's FiLM vector for this sigma, in torch as the reference computes it: (rows of sigma, sum of dims)."""
        _, (w, b), _, _ = self._pack()
        return F.linear(self.embedding(sigma), w, b)

    def _plan_for(self, B, T, per_stream, dev):
        """The _Plan of one evaluation for (B, T) on dev, with one FiLM row per stream or one for all: built on first use."""
        key = (B, T, per_stream, dev)
        self._pack()                              # drops the plans of parameters that have changed since
        if key not in self._plans:
            plan = _Plan(self, *key)
            self._walk(plan, plan.x)
            self._plans[key] = plan
        return self._plans[key]

    def forward(self, inputs, sigma, films=None, record=None):
        """The network on the HIP path: inputs (B, T), sigma (1 | B, 1) (or `films` from self.films(sigma), which the sampler
        computes once per step at construction).  -> (B, T).  record(name, tensor), if given, then sees what forward_torch's
        sees, from this evaluation's own buffers (as clones: the next evaluation writes them again)."""
        if not inputs.is_cuda:
            raise RuntimeError(f"UNet1D.forward: HIP device only (no CPU fallback); use forward_torch.  Supported: {SUPPORTED}")
        if films is None:
            films = self.films(sigma.reshape(-1, 1).float())
        inputs = inputs.float().contiguous()
        B, T = inputs.shape
        if films.shape[0] not in (1, B):
            raise ValueError(f"UNet1D.forward: sigma has {films.shape[0]} rows for a batch of {B}")
        assert films.is_contiguous() or films.shape[0] == 1
        plan = self._plan_for(B, T, films.shape[0] != 1, inputs.device)
        out, stream = torch.empty(B, T, dtype=torch.float32, device=inputs.device), _lib.current_stream()
        plan.run(inputs, films, out, stream)
        if record is not None:
            for call in plan.record_calls:
                call(stream)
            for name, buf in plan.buffers.items():
                record(name, out if buf.device.type == "meta" else buf.clone())
        return out


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------------

class _TolerantUnpickler(pickle.Unpickler):
    """The reference's checkpoints pickle their OmegaConf configuration next to the tensors: classes that are not installed
    here unpickle as empty stand-ins, everything else as usual."""

    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except (ImportError, AttributeError):
            return type(name, (), {"__init__": lambda self, *a, **k: None, "__setstate__": lambda self, s: None,
                                   "__module__": module})


_tolerant_pickle = types.ModuleType("ntm_tolerant_pickle")
_tolerant_pickle.Unpickler = _TolerantUnpickler
_tolerant_pickle.load = lambda f, **k: _TolerantUnpickler(f, **k).load()
_tolerant_pickle.__name__ = "pickle"


def load_checkpoint(path, device="cpu"):
    """A reference `.pt` (its "ema" dict) or an `.npz` export of one -> a state dict of tensors."""
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            return {k: torch.from_numpy(z[k].copy()).to(device) for k in z.files}
    ck = torch.load(path, map_location=device, pickle_module=_tolerant_pickle, weights_only=False)
    return ck["ema"]


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------

class DiffusionGenerator:
    """The reference's DiffusionGenerator.  On a HIP device every method runs the HIP path (network and EDM step kernels); with
    hip=False, or on the CPU, the torch path -- the reference's expressions on forward_torch.
    sampler (also a plain attribute, read by every call): "steps", one sampler step as ntm_edm_pre, the network's launches and
    ntm_edm_post; "one_launch", the whole sampler as ONE launch (ntm_unet_sample_one_launch, csrc/unet_sampler.hip) -- the same
    bits, for a network whose every level is at most 1024 frames at seg_len (the trajectory nets), HIP path only; anything it
    cannot run raises, it never falls back to "steps".  last_launches: this project's launches in the last sampler run (torch's
    own -- the draws, their stacking, the first latent's scaling -- not counted)."""

    def __init__(self, args, device, hip=None, sampler="steps"):
        if sampler not in SAMPLERS:
            raise ValueError(f"DiffusionGenerator: sampler {sampler!r}; built: {SAMPLERS}")
        self.sampler, self.last_launches, self._consts = sampler, 0, None
        self.args, self.device = args, torch.device(device)
        self.hip = self.device.type == "cuda" if hip is None else bool(hip)
        self.network = UNet1D(args, self.device)
        if args.network.get("checkpoint"):
            sd = load_checkpoint(args.network.checkpoint, self.device)
            levels = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("downs."))
            if levels != args.network.depth:
                # conf_noise.yaml says depth 8, the checkpoint it names (weights/83) holds 6 levels: say so by name
                raise ValueError(f"DiffusionGenerator: {args.network.checkpoint} holds a network of depth {levels}, "
                                 f"args.network.depth is {args.network.depth}: set args.network.depth = {levels}")
            self.network.load_state_dict(sd)
        self.network.eval()
        dp = args.diff_params
        self.sigma_min, self.sigma_max, self.ro, self.sigma_data = dp.sigma_min, dp.sigma_max, dp.ro, dp.sigma_data
        self.Schurn, self.Snoise = dp.Schurn, dp.Snoise
        self.seg_len, self.sample_rate, self.out_sample_rate = args.exp.seg_len, args.exp.sample_rate, args.exp.out_sample_rate
        # the schedule and gamma are computed on the host in float32, as the reference's expressions do, and copied
        self._schedule = self.create_schedule(dp.T)
        self._gamma = self.get_gamma(self._schedule)
        self.schedule, self.gamma = self._schedule.to(self.device), self._gamma.to(self.device)
        self._steps = self._bufs = None
        self._rs_kernel = None

    def create_schedule(self, nb_steps):
        i = torch.arange(0, nb_steps + 1)
        t = (self.sigma_max ** (1 / self.ro) + i / (nb_steps - 1) *
             (self.sigma_min ** (1 / self.ro) - self.sigma_max ** (1 / self.ro))) ** self.ro
        t[-1] = 0
        return t

    def cskip(self, sigma):
        return self.sigma_data ** 2 * (sigma ** 2 + self.sigma_data ** 2) ** -1

    def cout(self, sigma):
        return sigma * self.sigma_data * (self.sigma_data ** 2 + sigma ** 2) ** (-0.5)

    def cin(self, sigma):
        return (self.sigma_data ** 2 + sigma ** 2) ** (-0.5)

    def cnoise(self, sigma):
        return (1 / 4) * torch.log(sigma)

    def get_gamma(self, t):
        N = t.shape[0]
        gamma = torch.zeros(t.shape).to(t.device)
        return gamma + torch.min(torch.Tensor([self.Schurn / N, 2 ** (1 / 2) - 1])).to(t.dtype)

    def _net(self, x, cnoise, films=None):
        if self.hip:
            return self.network(x, cnoise, films=films)
        return self.network.forward_torch(x, cnoise.reshape(-1, 1) if cnoise.dim() < 2 else cnoise)

    def denoiser(self, xn, sigma):
        if len(sigma.shape) == 1:
            sigma = sigma.unsqueeze(-1)
        with torch.no_grad():
            return self.cskip(sigma) * xn + self.cout(sigma) * self._net(self.cin(sigma) * xn, self.cnoise(sigma))

    def ode_update(self, x, sigma_0, sigma_1):
        x_0_hat = self.denoiser(x, sigma_1)
        score = (x_0_hat - x) / sigma_1 ** 2
        return x - (sigma_0 - sigma_1) * sigma_1 * score

    # -- the per-step constants: fixed at construction of the schedule, computed once --
    def _plan(self):
        """Per step: the reference's scalars as float32 host tensors (its own expressions on the host schedule) and, on the HIP
        path, every block's FiLM vector for that step's cnoise."""
        if self._steps is None:
            sch = torch.flip(self._schedule, (0,))
            steps = []
            for i in range(len(sch) - 1):
                s0 = sch[-i - 1]
                if self._gamma[i] == 0:
                    s1, eps = sch[-i - 2], None
                else:
                    s1 = sch[-i - 2] + self._gamma[i] * sch[-i - 2]
                    eps = (s1 ** 2 - sch[-i - 2] ** 2) ** (1 / 2)
                st = {"s0": s0, "s1": s1, "eps": eps, "cskip": self.cskip(s0), "cout": self.cout(s0), "cin": self.cin(s0),
                      "cnoise": self.cnoise(s0), "b2": s0 ** 2, "k": (s1 - s0) * s0}
                if self.hip:
                    with torch.no_grad():
                        st["films"] = self.network.films(st["cnoise"].reshape(1, 1).to(self.device)).contiguous()
                    st["f"] = {n: float(st[n]) for n in ("s0", "cskip", "cout", "cin", "b2", "k")}
                    st["f"]["eps"] = 0.0 if eps is None else float(eps)
                steps.append(st)
            self._steps = steps
        return self._steps

    def _draw(self, draws, B):
        if draws is None:
            return torch.randn((B, self.seg_len), device=self.device)
        d = next(draws).to(self.device)
        assert d.shape == (B, self.seg_len), f"draws: expected {(B, self.seg_len)}, got {tuple(d.shape)}"
        return d

    def _sample(self, B, x_outpaint=None, mask=None, draws=None):
        if self.sampler not in SAMPLERS:
            raise ValueError(f"DiffusionGenerator: sampler {self.sampler!r}; built: {SAMPLERS}")
        if self.sampler == "one_launch":
            return self._sample_one_launch(B, x_outpaint, mask, draws)
        steps = self._plan()
        z = self._draw(draws, B) * self.schedule[0]
        if self.hip and mask is not None:                  # once per sample: every step reads the same two
            x_outpaint, mask = self._outpaint_operands(B, self.seg_len, x_outpaint, mask)
        for st in steps:
            eps = self._draw(draws, B) if st["eps"] is not None else None
            n = self._draw(draws, B) if mask is not None else None
            if self.hip:
                z = self._hip_step(z, st, eps, x_outpaint, mask, n, prepared=True)
                continue
            s0, s1 = st["s0"].to(z), st["s1"].to(z)
            if eps is not None:
                z = z + st["eps"].to(z) * (eps.to(z) * self.Snoise)
            if mask is not None:
                z = mask * (x_outpaint + n.to(z) * s0) + (1 - mask) * z
            z = self.ode_update(z, s1, s0)
        self.last_launches = len(steps) * (self.network._plan_for(B, self.seg_len, False, z.device).launches + 2) if self.hip else 0
        return z

    def _one_launch_consts(self):
        """The per-step operands of the one-launch sampler, made once per _plan() and Snoise: scal (steps, 8) -- the float32
        values _hip_step hands ntm_edm_pre and ntm_edm_post --, the steps' FiLM rows stacked, and the bit set of the steps
        that draw eps."""
        steps, sn = self._plan(), float(self.Snoise)
        if self._consts is None or self._consts[0] is not steps or self._consts[1] != sn:
            rows = [[st["f"]["eps"], sn] + [st["f"][n] for n in ("s0", "cin", "cskip", "cout", "b2", "k")] for st in steps]
            scal = torch.tensor(rows, dtype=torch.float32).to(self.device)
            films = torch.cat([st["films"] for st in steps], 0).contiguous()
            bits = sum(1 << i for i, st in enumerate(steps) if st["eps"] is not None)
            self._consts = (steps, sn, scal, films, bits)
        return self._consts[2:]

    def _sample_one_launch(self, B, x_outpaint, mask, draws):
        """_sample as one launch: the same draws taken in the same order first, then ntm_unet_sample_one_launch on the stage
        table of the step path's own plan (cached with it: per B, seg_len and state of the parameters)."""
        what, T = "DiffusionGenerator(sampler='one_launch')", self.seg_len
        if not self.hip or self.device.type != "cuda":
            raise RuntimeError(f"{what}: HIP device only (no CPU fallback, no torch path); supported: {SUPPORTED}")
        lengths = self.network.level_lengths(T)
        if max(lengths) > WHOLE_MAX_T:
            raise RuntimeError(f"{what}: every level must fit one workgroup, at most {WHOLE_MAX_T} frames; at seg_len {T} the "
                               f"levels have {lengths} frames, too long: {[n for n in lengths if n > WHOLE_MAX_T]}.  "
                               "Use sampler='steps'")
        steps = self._plan()
        if len(steps) > _lib.UNET_SAMPLE_MAX_STEPS:
            raise RuntimeError(f"{what}: {len(steps)} steps, at most {_lib.UNET_SAMPLE_MAX_STEPS}")
        z0 = (self._draw(draws, B) * self.schedule[0]).float().contiguous()
        if mask is not None:
            x_outpaint, mask = self._outpaint_operands(B, T, x_outpaint, mask)
        taken = []
        for st in steps:
            if st["eps"] is not None:
                taken.append(self._draw(draws, B))
            if mask is not None:
                taken.append(self._draw(draws, B))
        stacked = torch.stack([d.float() for d in taken]) if taken else None
        scal, films, bits = self._one_launch_consts()
        L, plan = _lib.lib(), self.network._plan_for(B, T, False, self.device)
        if getattr(plan, "one_launch", None) is None:
            host = _lib.unet_stages(plan.stages())
            if len(host) > _lib.UNET_SAMPLE_MAX_STAGES:
                raise RuntimeError(f"{what}: {len(host)} calls per evaluation, at most {_lib.UNET_SAMPLE_MAX_STAGES}")
            table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(self.device)
            n = L.ntm_unet_sample_workspace_floats(B, T)
            if n < 0:
                raise _lib.NtmError(f"ntm_unet_sample_workspace_floats refused: {L.ntm_last_error().decode()}")
            plan.one_launch = (host, table, torch.empty(max(n, 1), dtype=torch.float32, device=self.device))
        host, table, ws = plan.one_launch
        z = torch.empty_like(z0)
        _lib.check(L.ntm_unet_sample_one_launch(host, _lib.ptr(table), len(host), _lib.ptr(scal), _lib.ptr(films), films.shape[1],
                                                len(steps), bits, _lib.ptr(z0), _lib.ptr(stacked), len(taken), _lib.ptr(x_outpaint),
                                                _lib.ptr(mask), 0 if mask is None or mask.shape[0] == 1 else T, B, T, _lib.ptr(ws),
                                                _lib.ptr(z), _lib.current_stream()), "ntm_unet_sample_one_launch")
        self.last_launches = 1
        return z

    @staticmethod
    def _outpaint_operands(B, T, x_outpaint, mask):
        """x_outpaint and mask as ntm_edm_pre reads them: fp32, contiguous, (B, T) and (1 | B, T)."""
        mask = mask.float().expand(-1, T).contiguous() if mask.shape[0] != 1 else mask.float().contiguous()
        return x_outpaint.float().expand(B, T).contiguous(), mask

    def _hip_step(self, z, st, eps, x_outpaint, mask, n, prepared=False):
        """One sampler step on the device: ntm_edm_pre, the network, ntm_edm_post (prepared: by _outpaint_operands already)."""
        L, f = _lib.lib(), st["f"]
        z = z.float().contiguous()
        B, T = z.shape
        if self._bufs is None or self._bufs[0].shape != z.shape:
            self._bufs = (torch.empty_like(z), torch.empty_like(z))       # the step's two intermediates, reused by every step
        zin, net_in = self._bufs
        if mask is not None:
            if not prepared:
                x_outpaint, mask = self._outpaint_operands(B, T, x_outpaint, mask)
            n = n.float().contiguous()
        if eps is not None:
            eps = eps.float().contiguous()
        _lib.check(L.ntm_edm_pre(_lib.ptr(z), _lib.ptr(eps), f["eps"], float(self.Snoise), _lib.ptr(mask),
                                 0 if mask is None or mask.shape[0] == 1 else T, _lib.ptr(x_outpaint), _lib.ptr(n), f["s0"],
                                 f["cin"], B, T, _lib.ptr(zin), _lib.ptr(net_in), _lib.current_stream()), "ntm_edm_pre")
        with torch.no_grad():
            Fx = self.network(net_in, None, films=st["films"]).contiguous()
        out = torch.empty_like(z)
        _lib.check(L.ntm_edm_post(_lib.ptr(zin), _lib.ptr(Fx), f["cskip"], f["cout"], f["b2"], f["k"], B * T, _lib.ptr(out),
                                  _lib.current_stream()), "ntm_edm_post")
        return out

    def sample(self, draws=None):
        return self._sample(1, draws=draws)

    def outpaint_sample(self, x_oupaint, mask, draws=None):
        return self._sample(x_oupaint.shape[0], x_oupaint, mask, draws=draws)

    def sample_batch(self, batch_size, draws=None):
        """B independent samples through every launch together (the reference loops over sample())."""
        return self._sample(batch_size, draws=draws)

    def sample_long(self, Length, batch=1, draws=None):
        """The reference's sample_long; batch=B: B independent long samples side by side -> (B, ...).  self.segments counts the
        sampler runs of the last call."""
        Length_samples = int(Length * self.sample_rate)
        output = torch.zeros((batch, Length_samples), device=self.device)
        first = self._sample(batch, draws=draws)
        self.segments = 1
        if first.shape[-1] > Length_samples:
            output = first[:, :Length_samples]
        else:
            output[..., 0:first.shape[-1]] = first
            mask = torch.zeros_like(first[:1])
            samples_ov = int(self.args.outpainting.overlap * self.sample_rate)
            hop = self.seg_len - samples_ov
            mask[..., 0:samples_ov] = 1
            pointer = hop
            while (pointer + self.seg_len) < Length_samples:
                pred = self._sample(batch, output[..., pointer:(pointer + self.seg_len)], mask, draws=draws)
                output[..., pointer:(pointer + self.seg_len)] = pred
                pointer += hop
                self.segments += 1
            if pointer + samples_ov < Length_samples:
                x_pred = output[..., pointer::]
                x_pred = torch.cat((x_pred, torch.zeros(batch, self.seg_len - x_pred.shape[-1], device=self.device)), -1)
                pred = self._sample(batch, x_pred, mask, draws=draws)
                output[..., pointer::] = pred[..., 0:output.shape[-1] - pointer]
                self.segments += 1
        return self.resampler(output)

    def resampler(self, x):
        """torchaudio.functional.resample(x, sample_rate, out_sample_rate): equal rates return x; otherwise the polyphase filter
        bank of the reduced ratio (100 -> 44 100: 441 phases of 15 taps).  On the HIP path with an integer ratio, the
        upsampling kernel of the network (ntm_unet_up_combine's resampling half)."""
        o, n = int(self.sample_rate), int(self.out_sample_rate)
        if o == n:
            return x
        if self._rs_kernel is None:
            k, w = sinc_resample_kernel(o, n)
            g = math.gcd(o, n)
            self._rs_kernel = (k.to(self.device), w, o // g, n // g)
        k, w, o, n = self._rs_kernel
        if self.hip and o == 1 and x.is_cuda:
            out = torch.empty(x.shape[0], 1, n * x.shape[-1], dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().ntm_unet_upsample(_lib.ptr(x.float().contiguous()), _lib.ptr(k), x.shape[0], x.shape[-1], n, w,
                                                    k.shape[-1], _lib.ptr(out), _lib.current_stream()), "ntm_unet_upsample")
            return out.squeeze(1)
        return apply_resample_kernel(x, k, o, n, w)


# ---- training ----------------------------------------------------------------------------------------------------------------------------

class EDMTrainer:
    """The EDM training step of the reference (code/train-diffusion.py: the diffusion parameters of class EDM, :44-221, and
    Trainer.train_step / update_ema, :377-430) on a UNet1D of this module.
    backend "hip": the network runs UNet1D.forward_train (HIP device only); "torch": forward_torch, any device and dtype.
    draws = (a, noise) stands in for the step's torch.rand(B) and torch.randn(B, T), so that a recorded run can be replayed.
    With an optim.FusedAdam the gradient clip, the Adam step and the EMA run as launches over lists of tensors (optim.py);
    with any other optimizer they are torch's, as in the reference.
    Either the caller hands train_step its batch (B, T) and counts with `iteration`, or dset= supplies the batches and
    training_loop runs the reference's loop (:431-443) with its checkpoints (:277-364).  dset is what the reference's Trainer
    takes -- an iterator of (B, seg_len) segments at the dataset's rate, which get_batch moves to the device and resamples (:366-375)
    -- or an object with next_batch() (datasets_diffusion.DeviceSegmentFeeder) that returns the finished batch.
    load_state_dict builds attempts 1 and 2 of utilities/training_utils.load_state_dict (strict; then strict=False without the
    optimizer); its attempts 3 to 7 and the last resort, which serve the checkpoint layouts of other projects, are not built: a
    checkpoint that both attempts refuse raises.
    The reference's prints and its hydra and logging code are not here; the command line is tools/train_diffusion.py."""

    def __init__(self, args, network, optimizer, device, backend="hip", scheduler=None, dset=None):
        if backend not in ("hip", "torch"):
            raise ValueError(f"EDMTrainer: backend {backend!r}; built: 'hip' and 'torch'")
        self.args, self.network, self.optimizer, self.device, self.backend = args, network, optimizer, device, backend
        self.scheduler, self.dset = scheduler, dset
        self.latest_checkpoint = None
        self._resample = None
        dp = args.diff_params
        self.sigma_min, self.sigma_max, self.ro, self.sigma_data = dp.sigma_min, dp.sigma_max, dp.ro, dp.sigma_data
        network._packed, network._plans = None, {}        # caches of bound launches: not state, and not copyable
        self.ema = copy.deepcopy(network).eval().requires_grad_(False)
        self.it = 0

    # -- the diffusion parameters --
    def sample_ptrain_safe(self, N, a=None):
        if a is None:
            a = torch.rand(N)
        return (self.sigma_max ** (1 / self.ro) + a * (self.sigma_min ** (1 / self.ro) - self.sigma_max ** (1 / self.ro))) ** self.ro

    def cskip(self, sigma):
        return self.sigma_data ** 2 * (sigma ** 2 + self.sigma_data ** 2) ** -1

    def cout(self, sigma):
        return sigma * self.sigma_data * (self.sigma_data ** 2 + sigma ** 2) ** (-0.5)

    def cin(self, sigma):
        return (self.sigma_data ** 2 + sigma ** 2) ** (-0.5)

    def cnoise(self, sigma):
        return (1 / 4) * torch.log(sigma)

    def prepare_train_preconditioning(self, x, sigma, noise=None):
        noise = (torch.randn(x.shape) if noise is None else noise).to(sigma.device) * sigma
        cskip, cout, cin, cnoise = self.cskip(sigma), self.cout(sigma), self.cin(sigma), self.cnoise(sigma)
        target = (1 / cout) * (x - cskip * (x + noise))
        return cin * (x + noise), target, cnoise

    def _net(self, inputs, cnoise):
        if self.backend == "hip":
            return self.network.forward_train(inputs, cnoise)
        return self.network.forward_torch(inputs, cnoise)

    def loss_fn(self, x, draws=None):
        """-> (error ** 2 (B, T), sigma (B, 1))."""
        a, noise = (None, None) if draws is None else draws
        sigma = self.sample_ptrain_safe(x.shape[0], a).unsqueeze(-1).to(x.device)
        inputs, target, cnoise = self.prepare_train_preconditioning(x, sigma, noise)
        error = self._net(inputs, cnoise) - target
        return error ** 2, sigma

    # -- the loop's steps --
    def train_step(self, x, draws=None):
        """One optimiser step on the batch x (B, T) -> the loss (detached).  self.lr and self.grad_norm: what the step used."""
        train = self.args.train
        self.optimizer.zero_grad()
        error, _ = self.loss_fn(x, draws)
        loss = error.mean()
        loss.backward()
        if self.it <= train.lr_rampup_it:
            for g in self.optimizer.param_groups:
                g["lr"] = train.lr * min(self.it / max(train.lr_rampup_it, 1e-8), 1)
        self.lr = self.optimizer.param_groups[0]["lr"]
        self.grad_norm = None
        if isinstance(self.optimizer, optim.FusedAdam):      # the norm, the clip and the step as launches over lists of tensors
            self.grad_norm = self.optimizer.step(max_grad_norm=train.max_grad_norm if train.use_grad_clip else None)
        else:
            if train.use_grad_clip:
                self.grad_norm = torch.nn.utils.clip_grad_norm_(self.network.parameters(), train.max_grad_norm)
            self.optimizer.step()
        if self.scheduler is not None:
            self.scheduler.step()
        return loss.detach()

    def update_ema(self):
        train = self.args.train
        t = self.it * train.batch
        with torch.no_grad():
            s = np.clip(t / train.ema_rampup, 0.0, train.ema_rate) if t < train.ema_rampup else train.ema_rate
            if isinstance(self.optimizer, optim.FusedAdam):
                optim.ema_update_(self.ema.parameters(), self.network.parameters(), s)
                return
            for dst, src in zip(self.ema.parameters(), self.network.parameters()):
                dst.copy_(dst * s + src * (1 - s))

    def iteration(self, x, draws=None):
        """What the reference's training_loop does per pass, without the checkpoint: train_step, update_ema, it += 1."""
        loss = self.train_step(x, draws)
        self.update_ema()
        self.it += 1
        return loss

    def state_dict(self):
        """The reference's checkpoint: DiffusionGenerator loads its "ema"."""
        return {"it": self.it, "network": self.network.state_dict(), "optimizer": self.optimizer.state_dict(),
                "ema": self.ema.state_dict(), "args": self.args}

    # -- the loop, its batches and its checkpoints --
    def get_batch(self):
        """The next batch (B, T) float32 on the device: next(dset), moved and resampled from args.dset.fs to args.exp.sample_rate
        by torchaudio's rule (the filter is built once here; torchaudio rebuilds it per call), or dset.next_batch()."""
        if self.dset is None:
            raise RuntimeError("EDMTrainer.get_batch: no dset= was given")
        if hasattr(self.dset, "next_batch"):
            return self.dset.next_batch()
        audio = torch.as_tensor(next(self.dset)).to(self.device).to(torch.float32)
        o, n = int(self.args.dset.fs), int(self.args.exp.sample_rate)
        if o == n:
            return audio
        if self._resample is None:
            k, w = sinc_resample_kernel(o, n)
            g = math.gcd(o, n)
            self._resample = (k.to(self.device), w, o // g, n // g)
        k, w, o, n = self._resample
        return apply_resample_kernel(audio, k, o, n, w)

    def training_loop(self, max_it=None, log=None):
        """The reference's loop: train_step, update_ema, the checkpoint condition, it += 1.  The reference never returns; here
        max_it is the last iteration number that runs (None: for ever), so that a checkpoint due at max_it is still written.
        log(it, loss), if given, is called after every step with the detached loss (reading it synchronises)."""
        train = self.args.train
        while max_it is None or self.it <= max_it:
            loss = self.train_step(self.get_batch())
            self.update_ema()
            if log is not None:
                log(self.it, loss)
            if self.it > 0 and self.it % train.save_interval == 0 and train.save_model:
                self.save_checkpoint()
            self.it += 1

    def save_checkpoint(self):
        """{model_dir}/{exp_name}-{it}.pt; with args.logging.remove_last_checkpoint the file this trainer wrote before goes.
        (The reference's configurations have no `logging` section, and its save_checkpoint fails on them after the file is
        written; here a missing section reads as "keep".)"""
        save_name = f"{self.args.model_dir}/{self.args.exp.exp_name}-{self.it}.pt"
        torch.save(self.state_dict(), save_name)
        if (self.args.get("logging") or {}).get("remove_last_checkpoint"):
            try:
                os.remove(self.latest_checkpoint)
            except (OSError, TypeError):          # nothing written yet (None), or already gone: as the reference, go on
                pass
        self.latest_checkpoint = save_name
        return save_name

    def load_state_dict(self, sd):
        """Attempts 1 and 2 of the reference's training_utils.load_state_dict -> True; raises what attempt 2 raised otherwise."""
        try:
            self.network.load_state_dict(sd["network"])
            self.optimizer.load_state_dict(sd["optimizer"])
            self.ema.load_state_dict(sd["ema"])
            return True
        except Exception:                         # noqa: BLE001 -- the reference's rule: whatever fails, try the next way
            pass
        self.network.load_state_dict(sd["network"], strict=False)
        self.ema.load_state_dict(sd["ema"], strict=False)
        return True

    def resume_from_checkpoint(self, checkpoint_path=None, checkpoint_id=None):
        """The reference's: a path, or {model_dir}/{exp_name}-{checkpoint_id}.pt with the largest id on disk by default.  Sets
        `it` from the checkpoint (157007 / 159000 where it holds none, as there) -> True; on any failure False, and with a path
        given `it` = 0."""
        try:
            if checkpoint_path is None:
                if checkpoint_id is None:
                    name = self.args.exp.exp_name
                    id_regex = re.compile(f"{name}-(\\d*)\\.pt")
                    checkpoint_id = max(int(id_regex.search(p).groups()[0]) for p in glob.glob(f"{self.args.model_dir}/{name}-*.pt"))
                path = f"{self.args.model_dir}/{self.args.exp.exp_name}-{checkpoint_id}.pt"
            else:
                path = checkpoint_path
            checkpoint = torch.load(path, map_location=self.device, pickle_module=_tolerant_pickle, weights_only=False)
            try:
                self.it = checkpoint["it"]
            except KeyError:
                self.it = 157007 if checkpoint_path is not None else 159000
            self.load_state_dict(checkpoint)
            return True
        except Exception as e:                    # noqa: BLE001 -- the reference's rule: report and train from scratch
            print(f"Could not resume from checkpoint: {e}")
            if checkpoint_path is not None:
                self.it = 0
            return False
