#!/usr/bin/env python3
"""Times the batch path of the diffusion trainers on the device, for the three configurations of the reference (the noise net:
44.1 kHz, 4 x 65 536 samples as they are; the toy trajectories: 44.1 kHz -> 100 Hz, 4 x 225 792 -> 4 x 512; the trajectories:
192 kHz -> 100 Hz, 4 x 983 040 -> 4 x 512), on the synthetic files of tests/diffusion_feed_cases.py:

  feeder        DeviceSegmentFeeder.next_batch(): the picks on the host, two launches of csrc/segment_feed.hip
  torch         the same crops the reference's way on the device: the rows gathered from the bank, minus their means, then
                torchaudio's rule in torch ops with the filter rebuilt on every call (sinc_resample_kernel on the host, uploaded,
                apply_resample_kernel's pad + conv1d)
  host          the reference's loader: next() of a DataLoader(num_workers=0) over the dataset class (files cached after their first
                read; the reference reads the whole file again per pick), then EDMTrainer.get_batch: upload + resample, filter cached
  loop          iterations per second of EDMTrainer.training_loop (hip backend, FusedAdam) with the feeder and with the host loader

feeder and torch: device-event times around the call; host and loop: a host clock around work that ends in a synchronise.  Warm-up,
then `--reps` repetitions: the median, and the smallest and largest as the spread.  One JSON line at the end (also written to
--json).  `--design DESIGN.md` writes the table between the markers `<!-- feed_probe:begin -->` and `<!-- feed_probe:end -->` of
that file, from this run or, with --from-json, from a recorded one.

Usage:  python tools/feed_probe.py [--reps 30] [--iters 40] [--json out.json] [--design DESIGN.md] [--from-json recorded.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BEGIN, END = "<!-- feed_probe:begin -->", "<!-- feed_probe:end -->"
CONFIG = {"hiss": "noise", "toy": "toytrajectories", "traj": "trajectories"}
LABEL = {"hiss": "noise, 44.1 kHz, 4 x 65 536", "toy": "toy trajectories, 441 : 1, 4 x 225 792 -> 512",
         "traj": "trajectories, 1920 : 1, 4 x 983 040 -> 512"}


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def table(res):
    f = lambda s: f"{s['median']:.3f} ({s['min']:.3f} - {s['max']:.3f})"      # noqa: E731
    rows = ["| configuration | feeder `next_batch()` [ms] | torch ops, filter rebuilt [ms] | host loader + `get_batch` [ms] | "
            "`iteration()` alone [ms] | loop, feeder [it/s] | loop, host loader [it/s] |", "|---|---|---|---|---|---|---|"]
    for case, r in res["cases"].items():
        rows.append(f"| {LABEL[case]} | {f(r['feeder_ms'])} | {f(r['torch_ms'])} | {f(r['host_ms'])} | {f(r['iteration_ms'])} | "
                    f"{r['loop_it_per_s']['device']:.1f} | {r['loop_it_per_s']['host']:.1f} |")
    rows.append("")
    rows.append(f"Medians with (smallest - largest) of {res['reps']} repetitions; loops of {res['iters']} iterations; {res['device']}.")
    return "\n".join(rows)


def write_design(path, res):
    with open(path) as fh:
        text = fh.read()
    a, b = text.index(BEGIN) + len(BEGIN), text.index(END)
    with open(path, "w") as fh:
        fh.write(text[:a] + "\n" + table(res) + "\n" + text[b:])


def measure(reps, iters):
    import torch

    import diffusion_feed_cases as C
    from ntm_amd import datasets_diffusion, diffusion, optim

    def events(fn, warmup=5):
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
        return stats(ms)

    def clock(fn, warmup=3):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        return stats(ms)

    def trainer(case, folder, feed):
        args = diffusion.load_config(CONFIG[case])
        args.dset = C.dset_args(folder, case)
        args.train.save_model = False
        if case == "hiss":
            args.network.depth = 6                      # the checkpoint's (weights/83)
        ds = getattr(datasets_diffusion, C.CASES[case][0])(args.dset)
        torch.manual_seed(11)
        net = diffusion.UNet1D(args, "cuda")
        for m in net.modules():                         # the reference starts these at zero: the blocks would get no gradient
            if isinstance(m, diffusion.CombinerUp):
                torch.nn.init.kaiming_uniform_(m.conv1x1.weight, a=5 ** 0.5)
        opt = optim.FusedAdam(net.parameters(), lr=args.train.lr, betas=(args.train.optimizer.beta1, args.train.optimizer.beta2),
                              eps=args.train.optimizer.eps)
        if feed == "device":
            dset = datasets_diffusion.DeviceSegmentFeeder(ds, args.train.batch, args.exp.sample_rate, "cuda")
        else:
            dset = iter(torch.utils.data.DataLoader(dataset=ds, batch_size=args.train.batch, num_workers=0))
        tr = diffusion.EDMTrainer(args, net, opt, "cuda", backend="hip", dset=dset)
        tr.it = 500                                     # inside the ramp-up, a non-zero learning rate
        return tr

    out = {"device": torch.cuda.get_device_name(0), "reps": reps, "iters": iters, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        folders = {which: C.write_wavs(os.path.join(tmp, which), which) for which in C.SETS}
        for case, (cls, which, seg_len, fs_out) in C.CASES.items():
            folder, r = folders[which], {}
            dev, host = trainer(case, folder, "device"), trainer(case, folder, "host")
            feeder = dev.dset
            r["feeder_ms"] = events(feeder.next_batch)
            starts = [feeder.offsets[num] + int(idx) for num, idx in feeder.last_picks]

            def torch_way():
                x = torch.stack([feeder.bank[s:s + seg_len] for s in starts])
                x = x - x.mean(-1, keepdim=True)
                if feeder.orig == feeder.new:
                    return x
                k, w = diffusion.sinc_resample_kernel(feeder.orig, feeder.new)
                return diffusion.apply_resample_kernel(x, k.to(x.device), feeder.orig, feeder.new, w)

            r["torch_ms"] = events(torch_way)
            r["host_ms"] = clock(host.get_batch)
            x = feeder.next_batch()
            r["iteration_ms"] = events(lambda: dev.iteration(x))
            r["loop_it_per_s"] = {}
            for name, tr in (("device", dev), ("host", host)):
                tr.training_loop(max_it=tr.it + 4)      # warm-up
                torch.cuda.synchronize()
                t = time.perf_counter()
                tr.training_loop(max_it=tr.it + iters - 1)
                torch.cuda.synchronize()
                r["loop_it_per_s"][name] = round(iters / (time.perf_counter() - t), 2)
            print(case, json.dumps(r), flush=True)
            out["cases"][case] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--json", default=None)
    ap.add_argument("--design", default=None)
    ap.add_argument("--from-json", default=None)
    a = ap.parse_args()
    if a.from_json:
        with open(a.from_json) as fh:
            res = json.load(fh)
    else:
        res = measure(a.reps, a.iters)
        if a.json:
            with open(a.json, "w") as fh:
                json.dump(res, fh)
    print(table(res))
    if a.design:
        write_design(a.design, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
