#!/usr/bin/env python3
"""Times one EDM training step of the trajectory net at the reference's shape (B = 4 x 512 samples, configs/conf_trajectories.yaml)
on the HIP backend (UNet1D.forward_train: training.ResBlockFn on csrc/unet_train.hip) against the torch backend (the same modules
under torch autograd) on the same device, splits the HIP step into the ResBlockFn forwards, their backwards, the weight-gradient
reductions inside those and the torch-op remainder, and times one block forward + backward at each level's frame count both ways.
Warm-up, then device-event times, medians; one JSON line at the end.

Usage:  python tools/diffusion_train_probe.py [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ntm_amd import _lib, diffusion, training  # noqa: E402

B, T = 4, 512


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def trainer(backend):
    args = diffusion.load_config("trajectories")
    torch.manual_seed(11)
    net = diffusion.UNet1D(args, "cuda")
    for m in net.modules():           # the reference starts these at zero, which would leave the blocks without a gradient
        if isinstance(m, diffusion.CombinerUp):
            torch.nn.init.kaiming_uniform_(m.conv1x1.weight, a=5 ** 0.5)
    opt = torch.optim.Adam(net.parameters(), lr=args.train.lr, betas=(args.train.optimizer.beta1, args.train.optimizer.beta2),
                           eps=args.train.optimizer.eps)
    tr = diffusion.EDMTrainer(args, net, opt, "cuda", backend=backend)
    tr.it = 500                       # inside the ramp-up, a non-zero learning rate
    return tr


class Spans:
    """Device time between pairs of events, summed per name over one step."""

    def __init__(self):
        self.open = []

    def wrap(self, name, fn):
        def inner(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            try:
                return fn(*a, **k)
            finally:
                e1.record()
                self.open.append((name, e0, e1))
        return inner

    def take(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.open:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        self.open = []
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    x = 1e-4 * torch.randn(B, T, device="cuda")
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "B": B, "T": T}
    hip, ref = trainer("hip"), trainer("torch")
    out["train_step_ms"] = {"hip": round(timed(lambda: hip.train_step(x), args.reps), 4),
                            "torch": round(timed(lambda: ref.train_step(x), args.reps), 4)}
    print(f"train_step  HIP {out['train_step_ms']['hip']:.3f} ms   torch {out['train_step_ms']['torch']:.3f} ms", flush=True)

    # the split of the HIP step
    spans, L, F = Spans(), _lib.lib(), training.ResBlockFn
    saved = (F.forward, F.backward, L.ntm_unet_wgrad_reduce)
    F.forward, F.backward = staticmethod(spans.wrap("forward", saved[0])), staticmethod(spans.wrap("backward", saved[1]))
    L.ntm_unet_wgrad_reduce = spans.wrap("reduce", saved[2])
    try:
        rows = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip.train_step(x)
            e1.record()
            row = spans.take()
            row["step"] = e0.elapsed_time(e1)
            rows.append(row)
    finally:
        F.forward, F.backward, L.ntm_unet_wgrad_reduce = staticmethod(saved[0]), staticmethod(saved[1]), saved[2]
    med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    med["torch_ops"] = med["step"] - med["forward"] - med["backward"]
    out["hip_step_split_ms"] = {k: round(v, 4) for k, v in med.items()}
    print("split of the HIP step (with the events' own cost):", out["hip_step_split_ms"], flush=True)

    # one block, forward + backward, at each level's frames
    out["block_ms"] = {}
    for frames in (512, 256, 128, 32):
        torch.manual_seed(frames)
        blk = diffusion.ResnetBlock(32, 16, 16).cuda()
        x0, x1 = (torch.randn(B, 16, frames, device="cuda", requires_grad=True) for _ in range(2))
        emb, gout = torch.randn(B, 16, device="cuda"), torch.randn(B, 16, frames, device="cuda")

        def node():
            w = torch.stack([h.conv.weight for h in blk.H])
            y = training.ResBlockFn.apply(x0, x1, blk.film.output_layer(emb), blk.first_conv[1].weight, w, blk.res_conv.weight, None, 0)
            y.backward(gout)

        def module():
            blk(torch.cat((x0, x1), 1), emb).backward(gout)

        a, b = timed(node, args.reps), timed(module, args.reps)
        out["block_ms"][frames] = {"hip": round(a, 4), "torch": round(b, 4), "speedup": round(b / a, 2)}
        print(f"block 16+16->16, {frames:4d} frames, forward + backward  HIP {a:.3f} ms   torch {b:.3f} ms   x{b / a:.2f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
