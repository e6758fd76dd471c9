"""Timing of the time-domain critic on the device (ntm_amd.critics.DilatedConvDisc: training.ConvStackFn on the kernels of
csrc/convstack_kernels.hip) at the adversarial run's window: B = 16 streams x T = 16 384 samples, the default critic (critic 3
of configs/AdversarialConfig.py: twelve layers, k = 5, dilations 1 .. 1024, 1).  Beside it the same architecture as plain torch
modules on the same device, with the same inputs and the same parameters: the reference's forward -- the weight_norm(nn.Conv1d)
/ nn.LeakyReLU modules of the very same critic object called one after the other.

Calls timed: forward (no graph), a train_crit-shaped call (two forwards of detached inputs, hinge loss, backward into the
parameters, Adam(lr = 0) step) and a train_gen-shaped call (forward of an input that requires grad, -mean, backward to the input
and the parameters, SGD(lr = 0) step on the input).  Then one layer of every kind alone -- the first (1 -> 64), the dilated
64 -> 64 at d = 1, 32 and 1024, the last (64 -> 1) -- as a one-layer stack through the C ABI against torch's own kernels on
the same tensors:
    forward          ntm_convstack_forward (weight preparation + conv + bias)       | torch._weight_norm + F.conv1d
    data gradient    ntm_convstack_backward(gx, dg = NULL)                          | aten.convolution_backward, input only
    weight gradient  ntm_convstack_backward(gx = NULL, dg) (+ weight-norm adjoint)  | aten.convolution_backward, weight + bias
with the 64 -> 64 layers' rate given against the 157.3 TFLOP/s fp32 matrix peak.

Event-timed windows of CALLS calls after WARMUP warm-up calls of every variant; the variants alternate inside each of ROUNDS
rounds, and every entry is the median over the rounds with the extremes (us per call).  Prints one JSON line.

    python3 tools/convstack_probe.py [B] [T]"""
import contextlib
import io
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ntm_amd                                                                           # noqa: E402,F401
from ntm_amd import _lib, critics                                                        # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
WARMUP, CALLS, ROUNDS = 10, 100, 7
PEAK_TF = 157.3
SLOPE = 0.2

if not torch.cuda.is_available():
    sys.exit("convstack_probe: no HIP device (timings are taken on the device only)")
gen = torch.Generator(device="cuda").manual_seed(1)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def window(fn, n):
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / n                                           # us per call


def measure(variants):
    """{name: fn} -> {name: [median, min, max]} us per call, the variants alternating inside each round."""
    for fn in variants.values():
        window(fn, WARMUP)
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(window(fn, CALLS))
    return {k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in times.items()}


class TorchTwin(torch.nn.Module):
    """The reference's forward on a DilatedConvDisc's own modules: same parameters, torch's kernels."""

    def __init__(self, crit):
        super().__init__()
        self.crit = crit

    def forward(self, x):
        for layer in self.crit.layers:
            x = layer(x)
        return x

    train_crit = critics.DilatedConvDisc.train_crit
    train_gen = critics.DilatedConvDisc.train_gen


out = {"B": B, "T": T, "calls": CALLS, "rounds": ROUNDS, "unit": "us per call: median [min, max] over the rounds", "layers": {}}
fake = 0.3 * torch.randn(B, 1, T, device="cuda", generator=gen)
real = 0.3 * torch.randn(B, 1, T, device="cuda", generator=gen)
y = (0.3 * torch.randn(B, 1, T, device="cuda", generator=gen)).requires_grad_(True)

torch.manual_seed(0)
with contextlib.redirect_stdout(io.StringIO()):
    crit = critics.DilatedConvDisc(test_in_len=T).cuda()
twin = TorchTwin(crit)
optC = torch.optim.Adam(crit.parameters(), lr=0, betas=(0.5, 0.9))
optY = torch.optim.SGD([y], lr=0.0)


def forward(model):
    with torch.no_grad():
        return model(fake)


def train_crit(model):
    crit.zero_grad(set_to_none=True)
    model.train_crit(fake, real, optC)


def train_gen(model):
    crit.zero_grad(set_to_none=True)
    y.grad = None
    model.train_gen(y, optY)


# same numbers before they are compared
a, b = forward(crit), forward(twin)
row = {"mflop_forward": round(2e-6 * B * sum(co * ci * k * (T - sum((kk - 1) * dd for _, _, kk, _, dd in crit.spec()[:l + 1]))
                                              for l, (ci, co, k, _, _) in enumerate(crit.spec())), 1),
       "forward_max_rel_diff": float((a - b).abs().max() / b.abs().max())}
train_gen(crit)
ga = y.grad.clone()
train_gen(twin)
row["train_gen_input_grad_max_rel_diff"] = float((ga - y.grad).abs().max() / y.grad.abs().max())
row.update(measure({f"{who}_{what}": (lambda m=model, f=fn: f(m)) for what, fn in (("forward", forward), ("train_crit", train_crit), ("train_gen", train_gen))
                    for who, model in (("device", crit), ("torch", twin))}))
out["critic"] = row
print(f"critic: {json.dumps(row)}", file=sys.stderr)

# ---- one layer of every kind alone
L, p = _lib.lib(), _lib.ptr
KINDS = {"first": (1, 64, 1), "d1": (64, 64, 1), "d32": (64, 64, 32), "d1024": (64, 64, 1024), "last": (64, 1, 1)}
K = 5
for name, (ci, co, d) in KINDS.items():
    frames = T - 4 * 2047 if name == "last" else T - 4 * (d - 1)                  # as it stands in the stack
    Fo = frames - (K - 1) * d
    x = torch.randn(B, ci, frames, device="cuda", generator=gen)
    v = torch.randn(co, ci, K, device="cuda", generator=gen) / (ci * K) ** 0.5
    gg = v.flatten(1).norm(dim=1).view(-1, 1, 1).clone()
    bias = torch.zeros(co, device="cuda")
    gout = torch.randn(B, co, Fo, device="cuda", generator=gen)
    lay = _lib.conv_layers_d(((ci, co, K, 1, d),))
    saved = torch.empty(int(L.ntm_convstack_saved_floats(B, ci, frames, 1, lay)), device="cuda")
    ws = torch.empty(int(L.ntm_convstack_workspace_floats(B, ci, frames, 1, lay)), device="cuda")
    o, gx, dg, dv, db = torch.empty_like(gout), torch.empty_like(x), torch.empty_like(gg), torch.empty_like(v), torch.empty_like(bias)
    A = lambda t: _lib.ptr_array([t])
    st = _lib.current_stream()

    def dev_forward():
        _lib.check(L.ntm_convstack_forward(p(x), B, ci, frames, SLOPE, 1, lay, A(gg), A(v), A(bias), p(saved), p(o), st), "forward")

    def dev_dgrad():
        _lib.check(L.ntm_convstack_backward(p(x), B, ci, frames, SLOPE, 1, lay, A(gg), A(v), p(saved), p(gout), p(gx), None, None, None, p(ws), st), "dgrad")

    def dev_wgrad():
        _lib.check(L.ntm_convstack_backward(p(x), B, ci, frames, SLOPE, 1, lay, A(gg), A(v), p(saved), p(gout), None, A(dg), A(dv), A(db), p(ws), st), "wgrad")

    w = torch._weight_norm(v, gg, 0)

    def torch_forward():
        return F.conv1d(x, torch._weight_norm(v, gg, 0), bias, dilation=d)

    def torch_dgrad():
        return torch.ops.aten.convolution_backward(gout, x, w, [co], [1], [0], [d], False, [0], 1, [True, False, False])

    def torch_wgrad():
        return torch.ops.aten.convolution_backward(gout, x, w, [co], [1], [0], [d], False, [0], 1, [False, True, True])

    dev_forward()
    dev_dgrad()
    dev_wgrad()
    tg = torch.ops.aten.convolution_backward(gout, x, w, [co], [1], [0], [d], False, [0], 1, [True, True, True])
    row = {"c_in": ci, "c_out": co, "dilation": d, "frames_out": Fo, "mflop": round(2e-6 * B * co * ci * K * Fo, 1),
           "forward_max_rel_diff": float((o - torch_forward()).abs().max() / torch_forward().abs().max()),
           "dgrad_max_rel_diff": float((gx - tg[0]).abs().max() / tg[0].abs().max()),
           "dbias_max_rel_diff": float((db - tg[2]).abs().max() / tg[2].abs().max())}
    row.update(measure({"device_forward": dev_forward, "torch_forward": torch_forward, "device_dgrad": dev_dgrad,
                        "torch_dgrad": torch_dgrad, "device_wgrad": dev_wgrad, "torch_wgrad": torch_wgrad}))
    if (ci, co) == (64, 64):
        row["device_fraction_of_fp32_matrix_peak"] = {kind: round(row["mflop"] / row["device_" + kind][0] / PEAK_TF, 3)   # MFLOP / us = TFLOP/s
                                                      for kind in ("forward", "dgrad", "wgrad")}
    out["layers"][name] = row
    print(f"layer {name}: {json.dumps(row)}", file=sys.stderr)
print(json.dumps(out))
