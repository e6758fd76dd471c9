#!/usr/bin/env python3
"""Times the diffusion generators' HIP path (csrc/unet_kernels.hip) against this project's torch path (UNet1D.forward_torch and the
reference's sampler expressions) on the same device: the shipped trajectory configuration (512 samples at 100 Hz, 8 steps) and the
noise configuration at 65 536 samples (16 steps, the checkpoint's depth), each for one network evaluation, one sample(),
sample_long(10.0) and sample_batch(16).  Warm-up, then device-event times of whole calls, medians; one JSON line at the end.

Usage:  python tools/diffusion_probe.py [--reps 7] [--golden tests/golden]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ntm_amd import diffusion  # noqa: E402


def timed(fn, reps, warmup=2):
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


def launches_per_evaluation(gen, T):
    """Kernel launches of one network evaluation on the HIP path: the calls of the bound plan, a tiled block counting two."""
    return gen.network._plan_for(1, T, False, torch.device("cuda")).launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--golden", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": {}}
    for name, depth in (("trajectories", None), ("noise", 6)):
        cfg = diffusion.load_config(name)
        cfg.network.checkpoint = os.path.join(args.golden, f"g29_diffusion_weights_{name}.npz")
        if depth:
            cfg.network.depth = depth
        hip = diffusion.DiffusionGenerator(cfg, "cuda")
        ref = diffusion.DiffusionGenerator(cfg, "cuda", hip=False)
        T = hip.seg_len
        x, s = torch.randn(1, T, device="cuda"), torch.tensor([[-1.5]], device="cuda")
        case = {"seg_len": T, "steps": len(hip.schedule) - 1, "launches_per_evaluation": launches_per_evaluation(hip, T)}
        with torch.no_grad():
            work = {"evaluation": (lambda: hip.network(x, s), lambda: ref.network.forward_torch(x, s)),
                    "sample": (hip.sample, ref.sample),
                    "sample_long_10s": (lambda: hip.sample_long(10.0), lambda: ref.sample_long(10.0)),
                    "sample_batch_16": (lambda: hip.sample_batch(16), lambda: ref.sample_batch(16))}
            for what, (f_hip, f_ref) in work.items():
                reps = args.reps if what != "sample_long_10s" or name != "noise" else max(3, args.reps // 2)
                a, b = timed(f_hip, reps), timed(f_ref, reps, warmup=1)
                case[what] = {"hip_ms": round(a, 4), "torch_ms": round(b, 4), "speedup": round(b / a, 2)}
                print(f"{name:13s} {what:16s} HIP {a:10.3f} ms   torch {b:10.3f} ms   x{b / a:.1f}", flush=True)
        out["cases"][name] = case
    print(json.dumps(out))


if __name__ == "__main__":
    main()
