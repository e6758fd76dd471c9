#!/usr/bin/env python3
"""Times the diffusion generators' HIP path (csrc/unet_kernels.hip) against this project's torch path (UNet1D.forward_torch and the
reference's sampler expressions) on the same device: the shipped trajectory configuration (512 samples at 100 Hz, 8 steps) and the
noise configuration at 65 536 samples (16 steps, the checkpoint's depth), each for one network evaluation, one sample(),
sample_long(10.0) and sample_batch(16).  Warm-up, then device-event times of whole calls, medians; one JSON line at the end.

--sampler steps | one_launch chooses the sampler mode of the HIP generators (DiffusionGenerator(sampler=)).  "one_launch" runs
where it can: the two shipped trajectory checkpoints (the noise net's levels do not fit a workgroup and are refused), and the
evaluation row is left out (the mode does not change it).  Either way the trajectory nets' sample() and sample_batch(16) are
then timed in BOTH modes on one generator, the modes taking turns repetition by repetition ("sampler_ab": median, min, max and
this project's launches per call).

Usage:  python tools/diffusion_probe.py [--reps 7] [--golden tests/golden] [--sampler steps|one_launch]
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


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median([once(fn) for _ in range(reps)])


def sampler_ab(gen, reps, warmup=3):
    """sample() and sample_batch(16) of one generator in both sampler modes, the modes taking turns so that a drift of the
    clocks falls on both: per mode the median, min and max in ms and the launches of a call."""
    out, keep = {}, gen.sampler
    try:
        for what, fn in (("sample", gen.sample), ("sample_batch_16", lambda: gen.sample_batch(16))):
            ms = {m: [] for m in diffusion.SAMPLERS}
            for i in range(warmup + reps):
                for m in diffusion.SAMPLERS:
                    gen.sampler = m
                    t = once(fn)
                    if i >= warmup:
                        ms[m].append(t)
                    out.setdefault(what, {}).setdefault(m, {})["launches"] = gen.last_launches
            for m, v in ms.items():
                out[what][m].update(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
                print(f"{what:16s} {m:11s} median {statistics.median(v):8.3f} ms   min {min(v):8.3f}   max {max(v):8.3f}   "
                      f"launches {out[what][m]['launches']}", flush=True)
    finally:
        gen.sampler = keep
    return out


def launches_per_evaluation(gen, T):
    """Kernel launches of one network evaluation on the HIP path: the calls of the bound plan, a tiled block counting two."""
    return gen.network._plan_for(1, T, False, torch.device("cuda")).launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--golden", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--sampler", choices=diffusion.SAMPLERS, default="steps")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "sampler": args.sampler, "cases": {}}
    nets = (("trajectories", None), ("noise", 6)) if args.sampler == "steps" else (("trajectories", None), ("toytrajectories", None))
    for name, depth in nets:
        cfg = diffusion.load_config(name)
        cfg.network.checkpoint = os.path.join(args.golden, f"g29_diffusion_weights_{name}.npz")
        if depth:
            cfg.network.depth = depth
        hip = diffusion.DiffusionGenerator(cfg, "cuda", sampler=args.sampler)
        ref = diffusion.DiffusionGenerator(cfg, "cuda", hip=False)
        T = hip.seg_len
        x, s = torch.randn(1, T, device="cuda"), torch.tensor([[-1.5]], device="cuda")
        case = {"seg_len": T, "steps": len(hip.schedule) - 1, "launches_per_evaluation": launches_per_evaluation(hip, T)}
        with torch.no_grad():
            work = {"evaluation": (lambda: hip.network(x, s), lambda: ref.network.forward_torch(x, s)),
                    "sample": (hip.sample, ref.sample),
                    "sample_long_10s": (lambda: hip.sample_long(10.0), lambda: ref.sample_long(10.0)),
                    "sample_batch_16": (lambda: hip.sample_batch(16), lambda: ref.sample_batch(16))}
            if args.sampler != "steps":
                del work["evaluation"]
            for what, (f_hip, f_ref) in work.items():
                reps = args.reps if what != "sample_long_10s" or name != "noise" else max(3, args.reps // 2)
                a, b = timed(f_hip, reps), timed(f_ref, reps, warmup=1)
                case[what] = {"hip_ms": round(a, 4), "torch_ms": round(b, 4), "speedup": round(b / a, 2)}
                print(f"{name:13s} {what:16s} HIP {a:10.3f} ms   torch {b:10.3f} ms   x{b / a:.1f}", flush=True)
            if name != "noise":
                print(f"{name}: both sampler modes", flush=True)
                case["sampler_ab"] = sampler_ab(hip, max(args.reps, 15))
        out["cases"][name] = case
    print(json.dumps(out))


if __name__ == "__main__":
    main()
