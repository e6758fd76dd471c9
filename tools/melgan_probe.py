"""Timing of the MelGAN critic on the device (ntm_amd.critics.MelGCrit: training.StridedConvStackFn on the kernels of
csrc/sconv_kernels.hip) at the adversarial run's window: B = 16 streams x T = 16 384 samples, configuration 0 of
configs/AdversarialConfig.py (num_D = 3, ndf = 16, n_layers = 4, downsampling_factor = 4: three discriminators of seven layers).
Beside it the same architecture as plain torch modules on the same device, with the same inputs and the same parameters: the
reference's forward -- the nn.Sequential / weight_norm(nn.Conv1d) modules of the very same critic object called layer by layer.

Calls timed: forward (no graph), a train_crit-shaped call (two forwards of detached inputs, hinge loss on scale[-1], backward
into the parameters, Adam(lr = 0) step) and a train_gen-shaped call (forward of an input that requires grad, -mean of scale[-1],
backward to the input and the parameters, SGD(lr = 0) step on the input).  Then every layer of one discriminator alone, at the
frames it has in the stack, as a one-layer stack through the C ABI against torch's own kernels on the same tensors:
    forward          ntm_sconvstack_forward (weight preparation + conv + bias)       | torch._weight_norm + (F.pad +) F.conv1d
    data gradient    ntm_sconvstack_backward(gx, dg = NULL)                          | aten.convolution_backward, input only (the
                                                                                       reflected layer: of the padded input, no fold)
    weight gradient  ntm_sconvstack_backward(gx = NULL, dg) (+ weight-norm adjoint)  | aten.convolution_backward, weight + bias
with every rate given against the 157.3 TFLOP/s fp32 matrix peak.

Event-timed windows of CALLS calls after WARMUP warm-up calls of every variant; the variants alternate inside each of ROUNDS
rounds, and every entry is the median over the rounds with the extremes (us per call).  Prints one JSON line.

    python3 tools/melgan_probe.py [B] [T]"""
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
WARMUP, CALLS, ROUNDS = 3, 10, 7
PEAK_TF = 157.3
SLOPE = 0.2

if not torch.cuda.is_available():
    sys.exit("melgan_probe: no HIP device (timings are taken on the device only)")
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
    """The reference's forward on a MelGCrit's own modules: same parameters, torch's kernels, layer by layer."""

    def __init__(self, crit):
        super().__init__()
        self.crit = crit

    def forward(self, x):
        results = []
        for disc in self.crit.model.values():
            h, feats = x, []
            for layer in disc.model.values():
                h = layer(h)
                feats.append(h)
            results.append(feats)
        return results

    train_crit = critics.MelGCrit.train_crit
    train_gen = critics.MelGCrit.train_gen


out = {"B": B, "T": T, "calls": CALLS, "rounds": ROUNDS, "unit": "us per call: median [min, max] over the rounds", "layers": {}}
fake = 0.3 * torch.randn(B, 1, T, device="cuda", generator=gen)
real = 0.3 * torch.randn(B, 1, T, device="cuda", generator=gen)
y = (0.3 * torch.randn(B, 1, T, device="cuda", generator=gen)).requires_grad_(True)

torch.manual_seed(0)
crit = critics.MelGCrit(num_D=3, ndf=16, n_layers=4, downsampling_factor=4).cuda()
twin = TorchTwin(crit)
optC = torch.optim.Adam(crit.parameters(), lr=0, betas=(0.5, 0.9))
optY = torch.optim.SGD([y], lr=0.0)
SPEC = crit.model["disc_0"].spec()
FR = crit.model["disc_0"].output_frames(T)


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
row = {"mflop_forward": round(2e-6 * B * 3 * sum(co * (ci // g) * k * f for (ci, co, k, g, *_), f in zip(SPEC, FR)), 1),
       "forward_max_rel_diff": max(float((p - q).abs().max() / q.abs().max()) for sa, sb in zip(a, b) for p, q in zip(sa, sb))}
del a, b
train_gen(crit)
ga = y.grad.clone()
gp = [p.grad.clone() for p in crit.parameters()]
train_gen(twin)
row["train_gen_input_grad_max_rel_diff"] = float((ga - y.grad).abs().max() / y.grad.abs().max())
row["train_gen_parameter_grad_max_rel_diff"] = max(float((p - q.grad).abs().max() / q.grad.abs().max()) for p, q in zip(gp, crit.parameters()))
del ga, gp
row.update(measure({f"{who}_{what}": (lambda m=model, f=fn: f(m)) for what, fn in (("forward", forward), ("train_crit", train_crit), ("train_gen", train_gen))
                    for who, model in (("device", crit), ("torch", twin))}))
out["critic"] = row
print(f"critic: {json.dumps(row)}", file=sys.stderr)

# ---- every layer of one discriminator alone
L, p = _lib.lib(), _lib.ptr
frames_in = [T] + FR[:-1]
for l, ((ci, co, K, groups, stride, pad, mode), Fi, Fo) in enumerate(zip(SPEC, frames_in, FR)):
    x = torch.randn(B, ci, Fi, device="cuda", generator=gen)
    v = torch.randn(co, ci // groups, K, device="cuda", generator=gen) / (ci // groups * K) ** 0.5
    gg = v.flatten(1).norm(dim=1).view(-1, 1, 1).clone()
    bias = torch.zeros(co, device="cuda")
    gout = torch.randn(B, co, Fo, device="cuda", generator=gen)
    lay = _lib.conv_layers_s(((ci, co, K, groups, stride, pad, mode),))
    saved = torch.empty(int(L.ntm_sconvstack_saved_floats(B, ci, Fi, 1, lay)), device="cuda")
    ws = torch.empty(int(L.ntm_sconvstack_workspace_floats(B, ci, Fi, 1, lay)), device="cuda")
    o, gx, dg, dv, db = torch.empty_like(gout), torch.empty_like(x), torch.empty_like(gg), torch.empty_like(v), torch.empty_like(bias)
    A = lambda t: _lib.ptr_array([t])
    st = _lib.current_stream()

    def dev_forward():
        _lib.check(L.ntm_sconvstack_forward(p(x), B, ci, Fi, SLOPE, 1, lay, A(gg), A(v), A(bias), p(saved), A(o), st), "forward")

    def dev_dgrad():
        _lib.check(L.ntm_sconvstack_backward(p(x), B, ci, Fi, SLOPE, 1, lay, A(gg), A(v), p(saved), A(o), A(gout), p(gx), None, None, None, p(ws), st), "dgrad")

    def dev_wgrad():
        _lib.check(L.ntm_sconvstack_backward(p(x), B, ci, Fi, SLOPE, 1, lay, A(gg), A(v), p(saved), A(o), A(gout), None, A(dg), A(dv), A(db), p(ws), st), "wgrad")

    w = torch._weight_norm(v, gg, 0)
    xin, tpad = (F.pad(x, (pad, pad), mode="reflect"), 0) if mode == 1 else (x, pad)

    def torch_forward():
        xp = F.pad(x, (pad, pad), mode="reflect") if mode == 1 else x
        return F.conv1d(xp, torch._weight_norm(v, gg, 0), bias, stride=stride, padding=tpad, groups=groups)

    def torch_dgrad():
        return torch.ops.aten.convolution_backward(gout, xin, w, [co], [stride], [tpad], [1], False, [0], groups, [True, False, False])

    def torch_wgrad():
        return torch.ops.aten.convolution_backward(gout, xin, w, [co], [stride], [tpad], [1], False, [0], groups, [False, True, True])

    dev_forward()
    dev_dgrad()
    dev_wgrad()
    tg = torch.ops.aten.convolution_backward(gout, xin, w, [co], [stride], [tpad], [1], False, [0], groups, [True, True, True])
    tgx = tg[0]
    if mode == 1:                                                                     # fold the mirrored borders back
        tgx = tgx[:, :, pad:pad + Fi].clone()
        tgx[:, :, 1:pad + 1] += tg[0][:, :, :pad].flip(-1)
        tgx[:, :, Fi - 1 - pad:Fi - 1] += tg[0][:, :, pad + Fi:].flip(-1)
    mflop = 2e-6 * B * co * (ci // groups) * K * Fo
    row = {"c_in": ci, "c_out": co, "k": K, "groups": groups, "stride": stride, "frames_out": Fo, "mflop": round(mflop, 1),
           "forward_max_rel_diff": float((o - torch_forward()).abs().max() / torch_forward().abs().max()),
           "dgrad_max_rel_diff": float((gx - tgx).abs().max() / tgx.abs().max()),
           "dweight_max_rel_diff": float((dv - torch.ops.aten._weight_norm_interface_backward(tg[1], v, gg, v.flatten(1).norm(dim=1).view(-1, 1, 1), 0)[0]).abs().max()
                                         / tg[1].abs().max()),
           "dbias_max_rel_diff": float((db - tg[2]).abs().max() / tg[2].abs().max())}
    row.update(measure({"device_forward": dev_forward, "torch_forward": torch_forward, "device_dgrad": dev_dgrad,
                        "torch_dgrad": torch_dgrad, "device_wgrad": dev_wgrad, "torch_wgrad": torch_wgrad}))
    row["device_fraction_of_fp32_matrix_peak"] = {kind: round(mflop / row["device_" + kind][0] / PEAK_TF, 4)   # MFLOP / us = TFLOP/s
                                                  for kind in ("forward", "dgrad", "wgrad")}
    out["layers"][f"layer_{l}"] = row
    print(f"layer {l}: {json.dumps(row)}", file=sys.stderr)
print(json.dumps(out))
