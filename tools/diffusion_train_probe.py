#!/usr/bin/env python3
"""Times one EDM training step of the trajectory net at the reference's shape (B = 4 x 512 samples, configs/conf_trajectories.yaml)
on the HIP backend (UNet1D.forward_train: training.ResBlockFn on csrc/unet_train.hip, training.DownCombineFn / UpCombineFn on
csrc/unet_resample_train.hip) against the torch backend (the same modules under torch autograd) on the same device and against
the PARENT-STYLE step (the same HIP trainer with the resample + combine steps of _TrainWalk bypassed to _TorchWalk's torch ops:
what the step was before those nodes), the two alternating in one process and the pair measured twice to show the spread; counts
the device kernels of a step both ways (torch.profiler, where it works); splits the HIP step into the ResBlockFn forwards and
backwards, the resample + combine nodes' forwards and backwards, the weight-gradient reductions inside the backwards and the
torch-op remainder; and times one block forward + backward at each level's frame count both ways.
Warm-up, then device-event times, medians; one JSON line at the end.

--net noise: the same for the tape-hiss net at the reference's operating point (configs/conf_noise.yaml at the checkpoint's
depth 6, B = 4 x 65 536 samples), whose three levels above 1024 frames run training.ResBlockTiledFn.  The parent-style step is
then the HIP trainer with those levels as torch modules (_TrainWalk.tiled_blocks = False: what the step was before the tiled
node); the split counts both block nodes, and where the profiler gives device times it adds the kernels of the tiled adjoint by
name (its fixed-order sums run inside the C call, where no event of this script reaches); the block table is at 4 096, 16 384
and 65 536 frames.

--optimizer fused|torch: the optimiser of the HIP trainer in the sections above (torch.optim.Adam as in the reference, or
optim.FusedAdam: the clip, the Adam step and the EMA as launches over lists of tensors, csrc/multi_tensor.hip).  Whatever it
says, the optimiser section times train_step and iteration() (train_step + update_ema) with FusedAdam against torch.optim.Adam
on the same EDMTrainer(backend="hip"), alternating in one process, the pair twice; counts the device kernels of both both ways
and the fused optimiser's own launches against the formula 2 L + 1 (+ L for the EMA), L = ceil(tensors / NTM_MULTI_MAX_TENSORS);
and reports whether one iteration leaves the weights and the EMA torch.equal to torch's own device ops, with and without the
clip.  --only-optimizer: that section alone.

Usage:  python tools/diffusion_train_probe.py [--reps 9] [--net trajectories|noise] [--optimizer fused|torch] [--only-optimizer]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ntm_amd import _lib, diffusion, optim, training  # noqa: E402

B, T = 4, 512
NET = "trajectories"
OPTIMIZER = "torch"


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


def trainer(backend, optimizer=None, clip=True):
    args = diffusion.load_config(NET)
    args.train.use_grad_clip = clip
    if NET == "noise":
        args.network.depth = 6        # the checkpoint's (weights/83)
    torch.manual_seed(11)
    net = diffusion.UNet1D(args, "cuda")
    for m in net.modules():           # the reference starts these at zero, which would leave the blocks without a gradient
        if isinstance(m, diffusion.CombinerUp):
            torch.nn.init.kaiming_uniform_(m.conv1x1.weight, a=5 ** 0.5)
    adam = optim.FusedAdam if (optimizer or OPTIMIZER) == "fused" and backend == "hip" else torch.optim.Adam
    opt = adam(net.parameters(), lr=args.train.lr, betas=(args.train.optimizer.beta1, args.train.optimizer.beta2),
               eps=args.train.optimizer.eps)
    tr = diffusion.EDMTrainer(args, net, opt, "cuda", backend=backend)
    tr.it = 500                       # inside the ramp-up, a non-zero learning rate
    return tr


class parent_style:
    """Inside, _TrainWalk runs its resample + combine steps as _TorchWalk does: torch ops under autograd.  For the noise net:
    inside, its blocks above 1024 frames are the torch modules."""
    NAMES = ("down", "up", "final")

    def __enter__(self):
        W = diffusion._TrainWalk
        if NET == "noise":
            W.tiled_blocks = False
            return
        self.saved = {n: W.__dict__[n] for n in self.NAMES}
        for n in self.NAMES:
            setattr(W, n, getattr(diffusion._TorchWalk, n))

    def __exit__(self, *exc):
        if NET == "noise":
            diffusion._TrainWalk.tiled_blocks = True
            return
        for n, f in self.saved.items():
            setattr(diffusion._TrainWalk, n, f)


def parent_step(tr, x):
    with parent_style():
        tr.train_step(x)


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(new, old, reps, warmup=3):
    """-> medians (new, old) of `reps` steps each, one of each in turn."""
    for _ in range(warmup):
        new(), old()
    torch.cuda.synchronize()
    rows = [(one(new), one(old)) for _ in range(reps)]
    return statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)


def kernels_of(fn):
    """Device kernels one call of fn starts, or None where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as e:                                    # noqa: BLE001 -- a count, not a result
        print(f"kernel count: {type(e).__name__}: {e}", flush=True)
        return None


def launches_of(fn, word="multi_"):
    """Launches of the kernels whose name holds `word` in one call of fn, by name, or None where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if str(e.device_type).endswith("CUDA") and word in e.name:
                name = e.name.split("(")[0].split("::")[-1]
                out[name] = out.get(name, 0) + 1
        return out or None
    except Exception as e:                                    # noqa: BLE001 -- a count, not a result
        print(f"launch count: {type(e).__name__}: {e}", flush=True)
        return None


def optimizer_section(out, x, reps):
    """FusedAdam against torch.optim.Adam on the same HIP trainer: times, kernel counts, launch formula, bit equality."""
    fused, ref = trainer("hip", "fused"), trainer("hip", "torch")
    tensors = sum(1 for p in fused.network.parameters() if p.requires_grad and p.numel())
    L = -(-tensors // _lib.MULTI_MAX_TENSORS)
    ema_tensors = sum(1 for p in fused.ema.parameters() if p.numel())
    Le = -(-ema_tensors // _lib.MULTI_MAX_TENSORS)
    res = {"tensors": tensors, "floats": sum(p.numel() for p in fused.network.parameters()), "L": L, "L_ema": Le}
    for what in ("train_step", "iteration"):
        pairs = [alternating(lambda: getattr(fused, what)(x), lambda: getattr(ref, what)(x), reps) for _ in range(2)]
        spread = max(abs(pairs[0][0] - pairs[1][0]), abs(pairs[0][1] - pairs[1][1]))
        gain = statistics.mean(p[1] for p in pairs) - statistics.mean(p[0] for p in pairs)
        res[what + "_ms"] = {"pairs": [{"fused": round(a, 4), "torch": round(b, 4)} for a, b in pairs], "spread": round(spread, 4),
                             "gain": round(gain, 4), "beyond_the_spread": bool(abs(gain) > spread)}
        print(f"{what}: FusedAdam vs torch.optim.Adam, two alternating runs:", res[what + "_ms"], flush=True)
        res[what + "_kernels"] = {"fused": kernels_of(lambda: getattr(fused, what)(x)), "torch": kernels_of(lambda: getattr(ref, what)(x))}
        print(f"device kernels per {what}:", res[what + "_kernels"], flush=True)
    res["fused_launches_per_iteration"] = launches_of(lambda: fused.iteration(x))
    res["formula"] = {"clip + adam": 2 * L + 1, "ema": Le}
    got = res["fused_launches_per_iteration"]
    if got is None:
        print("the profiler gives no device events here: the fused optimiser's launches are not counted", flush=True)
    else:
        res["formula_holds"] = sum(v for k, v in got.items() if "ema" not in k) == 2 * L + 1 and got.get("multi_ema_kernel", 0) == Le
        print(f"fused optimiser launches per iteration: {got}; formula 2 L + 1 = {2 * L + 1}, EMA {Le}: "
              f"{'holds' if res['formula_holds'] else 'DOES NOT HOLD'}", flush=True)
    # one iteration from equal weights on equal draws: are the results torch.equal to torch's own device ops?
    res["equal_to_torch"] = {}
    for clip in (True, False):
        a, b = trainer("hip", "fused", clip), trainer("hip", "torch", clip)
        g = torch.Generator().manual_seed(5)
        draws = (torch.rand(B, generator=g), torch.randn(B, T, generator=g))
        for tr in (a, b):
            tr.it = 1000                  # behind the EMA's ramp: s = ema_rate
            tr.iteration(x, draws)
        pa, pb = list(a.network.parameters()), list(b.network.parameters())
        ea, eb = list(a.ema.parameters()), list(b.ema.parameters())
        res["equal_to_torch"]["clip" if clip else "no clip"] = {
            "weights": f"{sum(torch.equal(p, q) for p, q in zip(pa, pb))} of {len(pa)} tensors",
            "ema": f"{sum(torch.equal(p, q) for p, q in zip(ea, eb))} of {len(ea)} tensors"}
        # the EMA alone, on equal inputs
        d1, d2 = [p.detach().clone() for p in eb], [p.detach().clone() for p in eb]
        optim.ema_update_(d1, pb, 0.999)
        with torch.no_grad():
            for d, q in zip(d2, pb):
                d.copy_(d * 0.999 + q * (1 - 0.999))
        res["equal_to_torch"]["ema_update_ alone"] = f"{sum(torch.equal(p, q) for p, q in zip(d1, d2))} of {len(d1)} tensors"
    print("torch.equal to torch's own device ops after one iteration:", res["equal_to_torch"], flush=True)
    out["fused_vs_torch"] = res


def kernel_ms_of(fn, word="unet_"):
    """Device milliseconds of one call of fn per kernel whose name holds `word`, or None where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
            if word in e.key and t:
                out[e.key.split("(")[0]] = round(t / 1000.0, 4)
        return out or None
    except Exception as e:                                    # noqa: BLE001 -- a table, not a result
        print(f"kernel times: {type(e).__name__}: {e}", flush=True)
        return None


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
    ap.add_argument("--net", choices=("trajectories", "noise"), default="trajectories")
    ap.add_argument("--optimizer", choices=("fused", "torch"), default="torch")
    ap.add_argument("--only-optimizer", action="store_true")
    args = ap.parse_args()
    global NET, T, OPTIMIZER
    NET, T, OPTIMIZER = args.net, 65536 if args.net == "noise" else T, args.optimizer
    x = 1e-4 * torch.randn(B, T, device="cuda")
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "net": NET, "B": B, "T": T, "optimizer": OPTIMIZER}
    optimizer_section(out, x, args.reps)
    if args.only_optimizer:
        print(json.dumps(out))
        return
    hip, ref = trainer("hip"), trainer("torch")
    out["train_step_ms"] = {"hip": round(timed(lambda: hip.train_step(x), args.reps), 4),
                            "torch": round(timed(lambda: ref.train_step(x), args.reps), 4)}
    print(f"train_step  HIP {out['train_step_ms']['hip']:.3f} ms   torch {out['train_step_ms']['torch']:.3f} ms", flush=True)

    # the new step against the parent-style step, alternating, the pair twice
    old = trainer("hip")
    pairs = [alternating(lambda: hip.train_step(x), lambda: parent_step(old, x), args.reps) for _ in range(2)]
    out["new_vs_parent_style_ms"] = [{"new": round(a, 4), "parent_style": round(b, 4)} for a, b in pairs]
    out["spread_ms"] = {"new": round(abs(pairs[0][0] - pairs[1][0]), 4), "parent_style": round(abs(pairs[0][1] - pairs[1][1]), 4)}
    print("new vs parent-style step, two alternating runs:", out["new_vs_parent_style_ms"], "spread", out["spread_ms"], flush=True)
    out["kernels_per_step"] = {"new": kernels_of(lambda: hip.train_step(x)), "parent_style": kernels_of(lambda: parent_step(old, x))}
    print("device kernels per step:", out["kernels_per_step"], flush=True)

    # the split of the HIP step
    spans, L = Spans(), _lib.lib()
    saved_reduce = L.ntm_unet_wgrad_reduce
    L.ntm_unet_wgrad_reduce = spans.wrap("reduce", saved_reduce)
    blocks, resamples = (training.ResBlockFn, training.ResBlockTiledFn), (training.DownCombineFn, training.UpCombineFn)
    nodes = blocks + resamples
    saved_nodes = [(N.forward, N.backward) for N in nodes]
    for N, (fw, bw) in zip(nodes, saved_nodes):
        pre = "" if N in blocks else "resample_"
        N.forward, N.backward = staticmethod(spans.wrap(pre + "forward", fw)), staticmethod(spans.wrap(pre + "backward", bw))
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
        L.ntm_unet_wgrad_reduce = saved_reduce
        for N, (fw, bw) in zip(nodes, saved_nodes):
            N.forward, N.backward = staticmethod(fw), staticmethod(bw)
    med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    med["torch_ops"] = med["step"] - med["forward"] - med["backward"] - med["resample_forward"] - med["resample_backward"]
    out["hip_step_split_ms"] = {k: round(v, 4) for k, v in med.items()}
    print("split of the HIP step (with the events' own cost):", out["hip_step_split_ms"], flush=True)

    if NET == "noise":
        out["unet_kernel_ms_per_step"] = kernel_ms_of(lambda: hip.train_step(x))
        print("device time of the step's unet kernels, by name:", out["unet_kernel_ms_per_step"], flush=True)

    # one block, forward + backward, at each level's frames
    out["block_ms"] = {}
    for frames in ((4096, 16384, 65536) if NET == "noise" else (512, 256, 128, 32)):
        torch.manual_seed(frames)
        blk = diffusion.ResnetBlock(32, 16, 16).cuda()
        x0, x1 = (torch.randn(B, 16, frames, device="cuda", requires_grad=True) for _ in range(2))
        emb, gout = torch.randn(B, 16, device="cuda"), torch.randn(B, 16, frames, device="cuda")

        def node():
            w = torch.stack([h.conv.weight for h in blk.H])
            fn = training.ResBlockTiledFn if frames > diffusion.WHOLE_MAX_T else training.ResBlockFn
            y = fn.apply(x0, x1, blk.film.output_layer(emb), blk.first_conv[1].weight, w, blk.res_conv.weight, None, 0)
            y.backward(gout)

        def module():
            blk(torch.cat((x0, x1), 1), emb).backward(gout)

        a, b = timed(node, args.reps), timed(module, args.reps)
        out["block_ms"][frames] = {"hip": round(a, 4), "torch": round(b, 4), "speedup": round(b / a, 2)}
        print(f"block 16+16->16, {frames:5d} frames, forward + backward  HIP {a:.3f} ms   torch {b:.3f} ms   x{b / a:.2f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
