"""Timing of the spectral critics on the device (ntm_amd.critics.MultiSpecCrit: training.SpecCritFn on the kernels of
csrc/critic_kernels.hip) at the adversarial run's window: B = 16 streams x T = 16 384 samples, the MultiSpecCrit configurations
1, 2 and 5 of configs/AdversarialConfig.py.  Beside it the same architecture as plain torch modules on the same device, with the
same inputs and the same parameters: the reference's forward -- the front end (TimeFreqConverter, shared), log10(clamp), then the
weight_norm(nn.Conv1d) / nn.LeakyReLU modules of the very same critic object called one after the other.

Calls timed per configuration: forward (no graph), a train_crit-shaped call (two forwards of detached inputs, hinge loss,
backward into the parameters, Adam(lr = 0) step) and a train_gen-shaped call (forward of an input that requires grad, -mean,
backward to the input and the parameters, SGD(lr = 0) step on the input).  Then every layer of configuration 1 alone, per
scale, as a one-layer stack through the C ABI against torch's own kernels on the same tensors:
    forward          ntm_speccrit_forward (weight preparation + conv + bias)       | torch._weight_norm + F.conv1d
    data gradient    ntm_speccrit_backward(gx, dg = NULL)                          | aten.convolution_backward, input only
    weight gradient  ntm_speccrit_backward(gx = NULL, dg) (+ weight-norm adjoint)  | aten.convolution_backward, weight + bias
with the dense 256 -> 256, k = 5 layer's rate given against the 157.3 TFLOP/s fp32 matrix peak.

Event-timed windows of CALLS calls after WARMUP warm-up calls of every variant; the variants alternate inside each of ROUNDS
rounds, and every entry is the median over the rounds with the extremes (us per call).  Prints one JSON line.

    python3 tools/critic_probe.py [B] [T]"""
import contextlib
import io
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ntm_amd                                                                           # noqa: E402
from ntm_amd import _lib, critics                                                        # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
WARMUP, CALLS, ROUNDS = 10, 100, 7
PEAK_TF = 157.3
COMMON = dict(layers=4, chan_in=16, chan_fac=4, stride=1, g_fac=16, log=True, test_in_len=T)
CONFIGS = {
    "1": dict(scales=[128, 256, 512, 1024], kernel_sizes=[21, 21, 21, 17], hop_sizes=[32, 64, 128, 128], tf_rep="spec", **COMMON),
    "2": dict(scales=[128, 256, 512, 1024], kernel_sizes=[21, 21, 21, 17], hop_sizes=[32, 64, 128, 128], tf_rep="mel", **COMMON),
    "5": dict(scales=[512, 1024, 2048], kernel_sizes=[21, 17, 7], hop_sizes=[64, 64, 64], tf_rep="spec", **COMMON),
}

if not torch.cuda.is_available():
    sys.exit("critic_probe: no HIP device (timings are taken on the device only)")
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
    """The reference's forward on a MultiSpecCrit's own modules: same parameters, torch's kernels behind the front end."""

    def __init__(self, crit):
        super().__init__()
        self.crit = crit

    def forward(self, x):
        outs = []
        for m in self.crit.models:
            if m.tf_rep == "spec":
                h = m.layers[0](x).squeeze()
            else:
                h = m.layers[0](x, mel=True)[1].squeeze()
            if m.log:
                h = torch.log10(torch.clamp(h, min=m.log_eps))
            for layer in m.layers[1:]:
                h = layer(h)
            outs.append(h)
        return outs

    train_crit = critics.MultiSpecCrit.train_crit
    train_gen = critics.MultiSpecCrit.train_gen


out = {"B": B, "T": T, "calls": CALLS, "rounds": ROUNDS, "unit": "us per call: median [min, max] over the rounds", "configs": {}, "layers": {}}
fake = 0.3 * torch.randn(B, 1, T, device="cuda", generator=gen)
real = 0.3 * torch.randn(B, 1, T, device="cuda", generator=gen)
y = (0.3 * torch.randn(B, 1, T, device="cuda", generator=gen)).requires_grad_(True)

for name, pars in CONFIGS.items():
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        crit = critics.MultiSpecCrit(**pars).cuda()
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
    row = {"forward_max_rel_diff": max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(a, b))}
    train_gen(crit)
    ga = y.grad.clone()
    train_gen(twin)
    row["train_gen_input_grad_max_rel_diff"] = float((ga - y.grad).abs().max() / y.grad.abs().max())
    row.update(measure({f"{who}_{what}": (lambda m=model, f=fn: f(m)) for what, fn in (("forward", forward), ("train_crit", train_crit), ("train_gen", train_gen))
                        for who, model in (("device", crit), ("torch", twin))}))
    out["configs"][name] = row
    print(f"config {name}: {json.dumps(row)}", file=sys.stderr)

# ---- every layer of configuration 1 alone, per scale
L, p = _lib.lib(), _lib.ptr
for scale, ks in zip(CONFIGS["1"]["scales"], CONFIGS["1"]["kernel_sizes"]):
    C0, frames = scale // 2 + 1, 1 + T // (scale // 4)
    spec = ((C0, 16, 10, 1), (16, 64, ks, 4), (64, 256, ks, 16), (256, 256, 5, 1), (256, 1, 3, 1))
    rows = {}
    for l, (ci, co, k, g) in enumerate(spec):
        Fo = frames - k + 1
        head = l == 0
        x = torch.randn(B, ci, frames, device="cuda", generator=gen)
        x = x * x + 1e-3 if head else x
        floor = 1e-5 if head else 0.0
        v = torch.randn(co, ci // g, k, device="cuda", generator=gen) / (ci // g * k) ** 0.5
        gg = v.flatten(1).norm(dim=1).view(-1, 1, 1).clone()
        bias = torch.zeros(co, device="cuda")
        gout = torch.randn(B, co, Fo, device="cuda", generator=gen)
        lay = _lib.conv_layers(((ci, co, k, g),))
        saved = torch.empty(int(L.ntm_speccrit_saved_floats(B, ci, frames, 1, lay)), device="cuda")
        ws = torch.empty(int(L.ntm_speccrit_workspace_floats(B, ci, frames, 1, lay)), device="cuda")
        o, gx, dg, dv, db = torch.empty_like(gout), torch.empty_like(x), torch.empty_like(gg), torch.empty_like(v), torch.empty_like(bias)
        A = lambda t: _lib.ptr_array([t])
        st = _lib.current_stream()

        def dev_forward():
            _lib.check(L.ntm_speccrit_forward(p(x), B, ci, frames, floor, 1, lay, A(gg), A(v), A(bias), p(saved), p(o), st), "forward")

        def dev_dgrad():
            _lib.check(L.ntm_speccrit_backward(p(x), B, ci, frames, floor, 1, lay, A(gg), A(v), p(saved), p(gout), p(gx), None, None, None, p(ws), st), "dgrad")

        def dev_wgrad():
            _lib.check(L.ntm_speccrit_backward(p(x), B, ci, frames, floor, 1, lay, A(gg), A(v), p(saved), p(gout), None, A(dg), A(dv), A(db), p(ws), st), "wgrad")

        xin = torch.log10(torch.clamp(x, min=floor)) if head else x
        w = torch._weight_norm(v, gg, 0)

        def torch_forward():
            return F.conv1d(xin, torch._weight_norm(v, gg, 0), bias, groups=g)

        def torch_dgrad():
            return torch.ops.aten.convolution_backward(gout, xin, w, [co], [1], [0], [1], False, [0], g, [True, False, False])

        def torch_wgrad():
            return torch.ops.aten.convolution_backward(gout, xin, w, [co], [1], [0], [1], False, [0], g, [False, True, True])

        dev_forward()
        row = {"c_in": ci, "c_out": co, "k": k, "groups": g, "frames_out": Fo, "mflop": round(2e-6 * B * co * (ci // g) * k * Fo, 1),
               "forward_max_rel_diff": float((o - torch_forward()).abs().max() / torch_forward().abs().max())}
        row.update(measure({"device_forward": dev_forward, "torch_forward": torch_forward, "device_dgrad": dev_dgrad,
                            "torch_dgrad": torch_dgrad, "device_wgrad": dev_wgrad, "torch_wgrad": torch_wgrad}))
        if (ci, co, g) == (256, 256, 1):
            row["device_fraction_of_fp32_matrix_peak"] = {kind: round(row["mflop"] / row["device_" + kind][0] / PEAK_TF, 3)   # MFLOP / us = TFLOP/s
                                                          for kind in ("forward", "dgrad", "wgrad")}
        rows[f"L{l + 1}"] = row
    out["layers"][str(scale)] = rows
    print(f"scale {scale}: {json.dumps(rows)}", file=sys.stderr)
print(json.dumps(out))
