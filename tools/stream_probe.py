#!/usr/bin/env python3
"""Per-block cost of real-time style inference on the MI355X, state on the device: harness.BlockStreamer on the GRU model, on
DiffDelRNN (one launch per block, the delay line on a ring: csrc/diffdel_stream.hip), and the per-block DiffDelRNN.forward loop
that was the only way to stream that model before (GRU launch + delay pass with its shifted buffer, fresh outputs per call).

    python3 tools/stream_probe.py [--rounds 7] [--window 0.2] [--json FILE]

Each path is warmed up, then timed over `rounds` windows of about `window` seconds of back-to-back blocks; the three paths take
turns round by round, so that whatever else the host is doing falls on all of them.  A window is bracketed by device events and
by a host clock that stops after a synchronise: the table gives the median of the event time per block and its spread (min ..
max over the rounds); the JSON has the host figures too.  D is the delay line's length (model.max_delay + 1).  DESIGN.md 3
carries the recorded table."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ntm_amd  # noqa: E402
from ntm_amd import harness, weights  # noqa: E402

SHAPES = [(1, 64, 11001), (16, 128, 11001), (256, 512, 11001), (1, 64, 256)]


def diffdel_model(D):
    m = ntm_amd.DiffDelRNN(1, 64, 1, skip=False, max_delay=D - 1)
    m.load_state_dict(weights.load_state_dict(weights.W_DIFFDEL))
    m = m.to("cuda").eval()
    m.warm_cache = True
    m.diffdel.defer_check = True
    return m


def paths(B, block, D):
    """-> {name: function that runs one block}, on resident inputs."""
    x = torch.rand(B, 1, block, device="cuda") - 0.5
    n = torch.arange(block, device="cuda", dtype=torch.float32)
    d = (0.5 * D + 0.4 * D * torch.sin(n / 37.0)).expand(B, 1, block).contiguous()
    rnn = harness.BlockStreamer(harness.build_model(weights.W_GRU), B, block)
    dd = harness.BlockStreamer(diffdel_model(D), B, block)
    assert dd.one_launch and dd.D == D
    m = diffdel_model(D)
    m._predict_start(B)

    def forward_loop():
        with torch.no_grad():
            m(x, d)

    return {"rnn_streamer": lambda: rnn.process(x), "diffdel_streamer": lambda: dd.process(x, d), "forward_loop": forward_loop}, (dd, m)


def window(fn, n):
    """n blocks back to back -> (event us per block, host us per block)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, (time.perf_counter() - t0) * 1e6 / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of blocks per timed window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stream_probe measures on the GPU; there is nothing to report without one"
    rows = []
    for B, block, D in SHAPES:
        fns, state = paths(B, block, D)
        counts = {}
        for name, fn in fns.items():                      # warm up, then size the window from a first look
            window(fn, 50)
            counts[name] = max(100, min(20000, int(a.window * 1e6 / window(fn, 100)[1])))
        res = {name: [] for name in fns}
        for _ in range(a.rounds):
            for name, fn in fns.items():
                res[name].append(window(fn, counts[name]))
        state[0].raise_if_violated()
        state[1].diffdel.raise_if_violated()
        row = {"B": B, "block": block, "D": D, "audio_us_per_block_44k1": block / 44100 * 1e6}
        for name, r in res.items():
            ev, host = [v[0] for v in r], [v[1] for v in r]
            row[name] = {"blocks_per_window": counts[name], "event_us": {"median": statistics.median(ev), "min": min(ev), "max": max(ev)},
                         "host_us": {"median": statistics.median(host), "min": min(host), "max": max(host)}}
        rows.append(row)
    print(f"us per block, median of {a.rounds} windows of ~{a.window} s (min .. max); device events")
    print("| B | block | D | RNN streamer | DiffDelRNN streamer | per-block model.forward | forward / streamer |")
    print("|---|---|---|---|---|---|---|")
    cell = lambda e: f"{e['median']:.1f} ({e['min']:.1f} .. {e['max']:.1f})"     # noqa: E731
    for r in rows:
        s, f = r["diffdel_streamer"]["event_us"], r["forward_loop"]["event_us"]
        print(f"| {r['B']} | {r['block']} | {r['D']} | {cell(r['rnn_streamer']['event_us'])} | {cell(s)} | {cell(f)} | {f['median'] / s['median']:.2f} |")
    if a.json:
        with open(a.json, "w") as fjson:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_s": a.window, "rows": rows}, fjson, indent=1)


if __name__ == "__main__":
    main()
