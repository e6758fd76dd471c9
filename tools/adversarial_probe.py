"""Timing of the adversarial loop's two steps on the device (ntm_amd.adversarial.Trainer) at the run's own shape:
B = 16 streams, windows of 16 384 samples, configurations 10 (three-scale MultiSpecCrit), 3 (DilatedConvDisc) and 0 (MelGCrit) of
ntm_amd.adversarial.load_config, the generator DiffDelRNN(hidden_size=64, skip=False).  Per configuration, us per call:

    critic_step stacked / two_call     Trainer.critic_step on fixed fake / real windows: one critic pass over cat([fake, real]) or two
    train_crit (modules' own)          critic.train_crit(fake, real, optC): what a user's hand-written loop called before
    generator_step                     Trainer.generator_step: grad-mode generator, critic, head, backward, optG.step, detach, zero_grad
    generator_step (hand-written)      the same window through generator(x, d), critic.train_gen(out.float(), optG), detach_hidden,
                                       zero_grad -- the reference's statements on the modules, before there was a Trainer
    generator forward / fwd+BPTT       generator(x, d) in grad mode alone, and with a backward from a fixed gradient at its output
    fakes                              generator(x, d) under no_grad (the critic phase's fakes)
    head / torch head                  forward + backward of training.AdvHeadFn on the critic's own outputs of a stacked pass, and of
                                       the torch expression it replaces, on the same tensors

Both optimizers are Adam(lr = 0, betas = (0.5, 0.9)): the steps run, the weights stay.  Event-timed windows of CALLS calls after
WARMUP warm-up calls of every variant; the variants alternate inside each of ROUNDS rounds (ROUNDS * CALLS >= 20 calls each), and
every entry is [median, min, max] over the rounds.  Prints one JSON line.

    python3 tools/adversarial_probe.py [configurations, comma separated] [B] [T]"""
import contextlib
import io
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ntm_amd                                                                           # noqa: E402
from ntm_amd import adversarial, critics, training                                       # noqa: E402

CONFIGS = [int(c) for c in sys.argv[1].split(",")] if len(sys.argv) > 1 else [10, 3, 0]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 16
T = int(sys.argv[3]) if len(sys.argv) > 3 else 16384
WARMUP, CALLS, ROUNDS = 2, 5, 5
FS, D_MIN_S, D_MAX_S = 44100, 400.25 / 44100, 700.75 / 44100

if not torch.cuda.is_available():
    sys.exit("adversarial_probe: no HIP device (timings are taken on the device only)")
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


def torch_head(n_fake, outs):
    loss = 0
    for scale in outs:
        loss += F.relu(1 + scale[:n_fake]).mean()
    for scale in outs:
        loss += F.relu(1 - scale[n_fake:]).mean()
    return loss


def probe(n):
    cfg = adversarial.load_config(n)
    torch.manual_seed(n)
    gen = ntm_amd.DiffDelRNN(hidden_size=cfg["hid_size"], skip=False).cuda()
    gen.load_state_dict({k: torch.as_tensor(v) for k, v in ntm_amd.weights.load_state_dict(ntm_amd.weights.W_DIFFDEL).items()})
    with contextlib.redirect_stdout(io.StringIO()):
        crit, _ = critics.get_critic(cfg["crit"], cfg["crit_pars"], "cuda", 0.0, T)
    optG = torch.optim.Adam(gen.parameters(), lr=0.0, betas=(0.5, 0.9))
    optC = torch.optim.Adam(crit.parameters(), lr=0.0, betas=(0.5, 0.9))
    tr = {s: adversarial.Trainer(gen, crit, optG, optC, T, FS, D_MIN_S, D_MAX_S, stacked=s) for s in (True, False)}
    init = tr[True].train_init
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(B, 1, init + T, device="cuda", generator=g) - 0.5
    real = 0.6 * torch.tanh(2.0 * x[:, :, init:]) + 0.01 * torch.randn(B, 1, T, device="cuda", generator=g)
    t = torch.arange(init + T, device="cuda", dtype=torch.float32)
    d = (150.0 + 140.0 * torch.sin(2 * math.pi * t / 9000.0 + torch.rand(B, 1, 1, device="cuda", generator=g) * 6.0)).expand(B, 1, -1).contiguous()
    xw, dw = x[:, :, init:].contiguous(), d[:, :, init:].contiguous()

    def restart(grad):
        with torch.enable_grad() if grad else torch.no_grad():
            gen.initialize_hidden(B, init)
            gen(x[:, :, :init], d[:, :, :init], warmup=True)
        gen.detach_hidden()
        gen.zero_grad()

    restart(False)
    with torch.no_grad():
        fake, _ = gen(xw, dw)
    gy = torch.randn(B, 1, T, device="cuda", generator=g) / (B * T)

    def hand_written():
        out, _ = gen(xw, dw)
        crit.train_gen(out.float(), optG)
        gen.detach_hidden()
        gen.zero_grad()

    def gen_forward():
        gen(xw, dw)
        gen.detach_hidden()

    def gen_fwd_bptt():
        out, _ = gen(xw, dw)
        out.backward(gy)
        gen.detach_hidden()
        gen.zero_grad()

    def fakes():
        with torch.no_grad():
            gen(xw, dw)

    with torch.no_grad():
        outs = [o.detach() for o in adversarial.critic_heads(crit, crit(torch.cat([fake, real])))]
    leaves = [o.clone().requires_grad_(True) for o in outs]

    def head():
        training.AdvHeadFn.apply("crit", B, *leaves).backward()
        for leaf in leaves:
            leaf.grad = None

    def head_torch():
        torch_head(B, leaves).backward()
        for leaf in leaves:
            leaf.grad = None

    res = {"critic": cfg["crit"], "train_init": init, "head_outputs": [list(o.shape) for o in outs]}
    res.update(measure({"critic_step stacked": lambda: (crit.zero_grad(), tr[True].critic_step(fake, real)),
                        "critic_step two_call": lambda: (crit.zero_grad(), tr[False].critic_step(fake, real)),
                        "train_crit (modules' own)": lambda: (crit.zero_grad(), crit.train_crit(fake, real, optC))}))
    crit.zero_grad()
    restart(True)
    res.update(measure({"generator_step": lambda: tr[True].generator_step(xw, dw), "generator_step (hand-written)": hand_written,
                        "generator forward": gen_forward, "generator fwd+BPTT": gen_fwd_bptt, "fakes": fakes}))
    res.update(measure({"head": head, "torch head": head_torch}))
    return res


if __name__ == "__main__":
    print(json.dumps({"B": B, "T": T, "calls": [WARMUP, CALLS, ROUNDS], "us_per_call": {str(n): probe(n) for n in CONFIGS}}))
