"""What tests/test_gpu_tiled_block.py builds on: one ResnetBlock's operands under the module's default initialisation, the torch
module's arithmetic on the CPU under autograd as the reference (computed once per case and dtype, shared and never changed),
the tiled HIP node on the same operands, and the noise-shaped network of the network-level tests.

The bar is diffusion_train_cases': per tensor, 3 x the reference's own float32-against-float64 distance in max norm relative to
max |ref64| -- from the two references, never from the code under test."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from ntm_amd import diffusion
from ntm_amd.training import ResBlockTiledFn
from diffusion_train_cases import bar_of, hold      # noqa: F401  (re-exported)

DEV = "cuda"
R2 = 2 ** 0.5
CHANNELS = {"identity 8-8": dict(c0=8, c1=0, cout=8), "16+16-16 cropped": dict(c0=16, c1=16, cout=16, off0=3, extra=4),
            "5+3-12": dict(c0=5, c1=3, cout=12, off0=1, extra=2), "init 8-16 cropped": dict(c0=8, c1=0, cout=16, init=True, off0=2)}


@functools.lru_cache(None)
def make_case(name, T, n=8, B=2, seed=0):
    """Float32 operands of one block on the CPU: src0 (B, c0, T0) -- with init the waveform (B, 1, T0) --, src1, film (B, cin),
    the weights under ResnetBlock's default initialisation, init_w, gout.  -> (operands, meta); shared, never written."""
    kw = CHANNELS[name]
    c0, c1, cout, off0, extra, init = kw["c0"], kw["c1"], kw["cout"], kw.get("off0", 0), kw.get("extra", 0), kw.get("init", False)
    g = torch.Generator().manual_seed(1000 + seed)
    cin, T0 = c0 + c1, T + off0 + extra
    torch.manual_seed(2000 + seed)
    blk = diffusion.ResnetBlock(cin, cout, 16, num_dils=n)
    op = {"src0": torch.randn(B, 1 if init else c0, T0, generator=g),
          "src1": torch.randn(B, c1, T, generator=g) if c1 else None,
          "film": 1 + 0.5 * torch.randn(B, cin, generator=g),
          "w_first": blk.first_conv[1].weight.detach().clone(),
          "w_gated": torch.stack([h.conv.weight.detach() for h in blk.H]).clone(),
          "w_res": None if cin == cout else blk.res_conv.weight.detach().clone(),
          "init_w": 0.5 * torch.randn(c0, 1, 5, generator=g) if init else None,
          "gout": torch.randn(B, cout, T, generator=g)}
    return op, dict(off0=off0, T=T, n=n, c0=c0)


def _leaves(op, dev, dt, skip=()):
    return {k: None if v is None else v.detach().to(dev, dt).clone().requires_grad_(
        k != "gout" and k not in skip and not (k == "src0" and op["init_w"] is not None)) for k, v in op.items()}


def _named(t, n):
    grads = {k: v.grad.detach() for k, v in t.items() if v is not None and v.requires_grad}
    for l in range(n):
        grads[f"w_gated.{l}"] = grads["w_gated"][l]
    del grads["w_gated"]
    return grads


def torch_block(op, meta, dt):
    """The module's arithmetic on the CPU under autograd -> (out, [y_0 .. y_{n-1}], gradients by operand name; dW_l per layer)."""
    t = _leaves(op, "cpu", dt)
    x0 = t["src0"] if t["init_w"] is None else F.conv1d(t["src0"], t["init_w"], padding="same")
    x = x0[:, :, meta["off0"]:meta["off0"] + meta["T"]]
    if t["src1"] is not None:
        x = torch.cat((x, t["src1"]), 1)
    x = x * t["film"].unsqueeze(-1)
    y, ys = F.conv1d(F.gelu(x), t["w_first"]), []
    for l in range(meta["n"]):
        ys.append(y)
        y = (y + F.conv1d(F.gelu(y), t["w_gated"][l], dilation=2 ** l, padding="same")) / R2
    out = (y + (x if t["w_res"] is None else F.conv1d(x, t["w_res"]))) / R2
    out.backward(t["gout"])
    return out.detach(), [v.detach() for v in ys], _named(t, meta["n"])


@functools.lru_cache(None)
def reference(name, T, n=8, B=2, seed=0):
    """-> ((out, ys, grads) in float64, the same in float32) of make_case's operands."""
    op, meta = make_case(name, T, n, B, seed)
    return torch_block(op, meta, torch.float64), torch_block(op, meta, torch.float32)


def hip_block(op, meta, skip=()):
    """The tiled node on the device -> (out, ysave (B, n, cout, T), gradients as torch_block names them); skip: operands that
    take no gradient."""
    t = _leaves(op, DEV, torch.float32, skip)
    out = ResBlockTiledFn.apply(t["src0"], t["src1"], t["film"], t["w_first"], t["w_gated"], t["w_res"], t["init_w"], meta["off0"])
    B, cout = out.shape[:2]
    ysave = out.grad_fn.saved_tensors[-1][:B * meta["n"] * cout * meta["T"]].view(B, meta["n"], cout, meta["T"])
    out.backward(t["gout"])
    return out.detach(), ysave.detach(), _named(t, meta["n"])


def integer_gout(shape, gen):
    """gout whose product with the kernel's float32 1 / sqrt 2 rounds to a small integer exactly -> (gout, the integers)."""
    c = np.float32(0.70710678118654752440)
    table = {}
    for k in range(-4, 5):
        g = np.float32(k * R2)
        for cand in (g, np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf))):
            if np.float32(cand * c) == np.float32(k):
                table[k] = cand
                break
    have = sorted(table)
    assert len(have) >= 5 and have[0] < 0 < have[-1], have
    ks = torch.tensor(have)[torch.randint(0, len(have), shape, generator=gen)]
    return torch.from_numpy(np.vectorize(table.get, otypes=[np.float32])(ks.numpy())), ks


# ---- the noise-shaped network ----
NET_DEPTH = 6


def noise_config():
    args = diffusion.load_config("noise")
    args.network.depth = NET_DEPTH
    return args


@functools.lru_cache(None)
def noise_net():
    """The noise configuration at depth 6 on the CPU in float32, the CombinerUp 1x1s (zero by default) redrawn.  Copy before use."""
    torch.manual_seed(31)
    net = diffusion.UNet1D(noise_config(), "cpu")
    for m in net.modules():
        if isinstance(m, diffusion.CombinerUp):
            torch.nn.init.kaiming_uniform_(m.conv1x1.weight, a=5 ** 0.5)
    return net
