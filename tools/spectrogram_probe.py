"""Timing of the differentiable device spectrogram (ntm_spectrogram / ntm_spectrogram_grad through training.SpectrogramFn) at
the adversarial run's window: B = 16 streams x T = 16 384 samples (configs/AdversarialConfig.py), one row per scale of the
reference's spectral critics (n_fft 128 ... 2048, hop n_fft / 4, window n_fft).  Beside it the only route the library offered
before: torch.stft(...) -> abs() ** 2 and its autograd backward, same device, same inputs, same upstream gradient.

Event-timed windows of CALLS calls after WARMUP warm-up calls of every variant; the four variants alternate inside each of ROUNDS
rounds, and the line gives the median over the rounds with the extremes (us per call).  Prints one JSON line.

    python3 tools/spectrogram_probe.py [B] [T]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ntm_amd                                                                           # noqa: E402
from ntm_amd.training import SpectrogramFn                                               # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
WARMUP, CALLS, ROUNDS = 10, 100, 7
SCALES = (128, 256, 512, 1024, 2048)

if not torch.cuda.is_available():
    sys.exit("spectrogram_probe: no HIP device (timings are taken on the device only)")
gen = torch.Generator(device="cuda").manual_seed(1)
y = (0.3 * torch.randn(B, T, device="cuda", generator=gen)).requires_grad_(True)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def window(fn, n):
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / n                                           # us per call


out = {"B": B, "T": T, "calls": CALLS, "rounds": ROUNDS, "unit": "us per call: median [min, max] over the rounds", "scales": {}}
for n_fft in SCALES:
    hop = n_fft // 4
    win = torch.hann_window(n_fft, device="cuda")
    up = torch.randn(B, n_fft // 2 + 1, 1 + T // hop, device="cuda", generator=gen)

    def ours(grad):
        if not grad:
            with torch.no_grad():
                return SpectrogramFn.apply(y, n_fft, hop, n_fft)
        y.grad = None
        SpectrogramFn.apply(y, n_fft, hop, n_fft).backward(up)

    def stft(grad):
        if not grad:
            with torch.no_grad():
                return torch.stft(y, n_fft, hop, n_fft, win, return_complex=True).abs() ** 2
        y.grad = None
        (torch.stft(y, n_fft, hop, n_fft, win, return_complex=True).abs() ** 2).backward(up)

    variants = {"device_forward": lambda: ours(False), "device_forward_backward": lambda: ours(True),
                "torch_stft_forward": lambda: stft(False), "torch_stft_forward_backward": lambda: stft(True)}
    # same numbers before they are compared: the two routes agree to fp32 roundoff
    with torch.no_grad():
        a, b = ours(False), stft(False)
    ours(True)
    ga = y.grad.clone()
    stft(True)
    row = {"frames": 1 + T // hop, "forward_max_rel_diff": float((a - b).abs().max() / b.abs().max()),
           "backward_max_rel_diff": float((ga - y.grad).abs().max() / y.grad.abs().max())}
    for fn in variants.values():
        window(fn, WARMUP)
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(window(fn, CALLS))
    for k, v in times.items():
        row[k] = [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]
    out["scales"][str(n_fft)] = row
print(json.dumps(out))
