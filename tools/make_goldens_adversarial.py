#!/usr/bin/env python3
"""Golden g28: the reference's adversarial run on the CPU, by importing the reference as the other makers do (torchaudio /
soundfile / librosa as empty stand-ins; wandb as a stand-in that drops what it is handed).

  tests/golden/g28_adversarial_configs.json   configs/AdversarialConfig.py: main(n) for n in 0-7 and 10.
  tests/golden/g28_adversarial.npz            the loop of code/train-adversarial.py on a small case.

The loop is not restated here: the lines 232-317 (one epoch of training) and 136-169 (one validation pass) of the reference's
script are read from the checkout at run time and executed as they stand, in a namespace that holds what the script has built
by then.  Generator: the reference's DiffDelRNN(hidden_size=64, skip=False) from the shipped DiffDelGRU-HS[64] weights;
critic: the reference's get_critic('DilatedConvDisc', {'layers': 6, 'conv_channels': 16}, 'cpu', lr, tbptt_len) under
torch.manual_seed(28) (receptive field 129 samples); both optimizers Adam(lr=1e-4, betas=(0.5, 0.9)) that record every p.grad
just before step().  B = 2, fs = 44100, tbptt_len = 1024, segments of train_init + 2 * 1024 samples, two iterations of three
different batches each (generator input, critic input, critic target; of each only the half the loop reads is stored).  The delay trajectories are float64 seconds between
d_min = 400.25 / fs and d_max = 700.75 / fs, so train_init = 1024 and d_traj_offset = 398; they are piecewise linear between
knots every 64 samples, and only the knots are stored (np.interp gives them back bit for bit).  The audio is float64 tensors of
float32 values, as VADataset(double=True) hands them over.

The loop runs twice:
  ref32   as the reference runs it (float32 modules; code/model.py:403 casts the input down; the delay line returns float64);
  ref64   the modules in double, the generator's forward called piecewise without that cast, and -- in the executed text only --
          `.float()` read as `.double()` and torch.inference_mode() as torch.no_grad() (an inference tensor of the critic's own
          dtype could not be saved for backward).
Recorded per pass: the critic's and the generator's loss of every window, the gradients at every optimizer step, the final
state dicts, and (pred, pre_d) of one validation batch of 2 x 3000 samples (made with the initial weights, as the script validates
before it trains).  ref64 is what the tests compare with; it is stored rounded to float32 (half an ulp of each element, far
below any bar), ref32 only where a test needs it (the losses, the critic's final weights).  E32 per kind of tensor -- the worst
max|ref32 - ref64| / max|ref64| over the tensors of that kind -- is computed here and stored beside them.  Nothing of the
reference travels: only inputs and recorded results.

usage: python tools/make_goldens_adversarial.py <reference checkout>"""
import contextlib
import io
import json
import os
import sys
import textwrap
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("NTM_REFERENCE", "")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
SCRIPT = os.path.join(REF, "code", "train-adversarial.py")
if not os.path.isfile(SCRIPT):
    sys.exit(__doc__)
for name in ("torchaudio", "soundfile", "librosa", "librosa.filters"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["librosa.filters"].mel = lambda *a, **k: None
sys.modules["librosa"].filters = sys.modules["librosa.filters"]
sys.path.insert(0, os.path.join(REF, "code"))
sys.path.insert(0, os.path.join(REF, "configs"))
sys.path.insert(0, ROOT)
import AdversarialConfig  # noqa: E402
import critics as ref_critics  # noqa: E402
import model as ref_model  # noqa: E402

from ntm_amd import weights  # noqa: E402

SEED, ITERS, B, FS, WIN, NWIN, T_VAL = 28, 2, 2, 44100, 1024, 2, 3000
D_MIN_S, D_MAX_S = 400.25 / FS, 700.75 / FS
LR = 1e-4
KNOT = 64
CRIT_PARS = {"layers": 6, "conv_channels": 16}
CONFIGS = (0, 1, 2, 3, 4, 5, 6, 7, 10)


class RecordingAdam(torch.optim.Adam):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.grads = []

    def step(self, closure=None):
        self.grads.append([p.grad.detach().clone() for g in self.param_groups for p in g["params"]])
        return super().step(closure)


class PiecewiseGenerator(ref_model.DiffDelRNN):
    """The reference's generator with forward() called piece by piece, so that the input keeps its dtype."""

    def forward(self, x, del_traj, warmup=False):
        h, self.hidden = self.GRU(x.reshape(x.shape[0], x.shape[2], x.shape[1]), self.hidden)
        pre_d = self.output(h)
        pre_d = pre_d.reshape(pre_d.shape[0], pre_d.shape[2], pre_d.shape[1])
        return self.diffdel(pre_d, del_traj, warmup), pre_d


def script_lines(first, last, double):
    with open(SCRIPT) as f:
        text = textwrap.dedent("".join(f.readlines()[first - 1:last]))
    if double:
        text = text.replace(".float()", ".double()").replace("torch.inference_mode()", "torch.no_grad()")
    return compile(text, f"{SCRIPT}:{first}-{last}", "exec")


def knots_to_traj(knots, T):
    """(..., K) float64 knots every KNOT samples -> (..., T) float64 seconds."""
    flat = knots.reshape(-1, knots.shape[-1])
    n = np.arange(T, dtype=np.float64)
    kn = np.arange(knots.shape[-1], dtype=np.float64) * KNOT
    return np.stack([np.interp(n, kn, row) for row in flat]).reshape(knots.shape[:-1] + (T,))


def make_knots(rng, shape, T):
    K = (T + KNOT - 1) // KNOT + 1
    n = np.arange(K) * KNOT
    ph = rng.uniform(0, 2 * np.pi, shape + (2, 1))
    mid, half = 0.5 * (D_MIN_S + D_MAX_S) * FS, 0.5 * (D_MAX_S - D_MIN_S) * FS - 1.0
    samples = mid + half * (0.8 * np.sin(2 * np.pi * n / 2300 + ph[..., 0, :]) + 0.2 * np.sin(2 * np.pi * n / 310 + ph[..., 1, :]))
    return samples / FS


def audio(rng, shape):
    x = rng.uniform(-0.5, 0.5, shape).astype(np.float32)
    t = (0.6 * np.tanh(2.0 * x) + 0.05 * np.roll(x, 3, axis=-1) + 0.01 * rng.standard_normal(shape)).astype(np.float32)
    return x, t


def run(double, inp, crit_sd0):
    dt = torch.float64 if double else torch.float32
    train_d_min, train_d_max = D_MIN_S * FS - 1, D_MAX_S * FS + 1
    train_init = max(int(train_d_max - train_d_min) + 2, 1024)
    d_traj_offset = int(train_d_min) - 1
    assert (train_init, d_traj_offset) == (1024, 398)
    T = train_init + NWIN * WIN
    Generator = (PiecewiseGenerator if double else ref_model.DiffDelRNN)(hidden_size=64, skip=False)
    Generator.load_state_dict(weights.load_state_dict(weights.W_DIFFDEL))
    Generator = Generator.to(dt)
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        Critic, _ = ref_critics.get_critic("DilatedConvDisc", dict(CRIT_PARS), "cpu", LR, WIN)
    if crit_sd0 is not None:
        assert all(torch.equal(v, crit_sd0[k]) for k, v in Critic.state_dict().items())
    sd0 = {k: v.clone() for k, v in Critic.state_dict().items()}
    Critic = Critic.to(dt)
    optG = RecordingAdam(Generator.parameters(), lr=LR, betas=(0.5, 0.9))
    optC = RecordingAdam(Critic.parameters(), lr=LR, betas=(0.5, 0.9))
    logged = {"loss/critic": [], "loss/gen": []}

    def log(values, step=None):
        for k, v in values.items():
            if k in logged:
                logged[k].append(float(v))

    as_t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))     # noqa: E731  float64 tensors of float32 values
    traj = knots_to_traj(inp["traj_knots"], T)                              # (ITERS, 2, B, T): generator input, critic input
    no_t = torch.zeros(0)                                                   # the halves of a batch that the loop drops
    inp_iter_gen = [(as_t(inp["x_gen"][i]), no_t, {"delay_trajectory": torch.from_numpy(traj[i, 0])}) for i in range(ITERS)]
    inp_iter_crit = [(as_t(inp["x_crit"][i]), no_t, {"delay_trajectory": torch.from_numpy(traj[i, 1])}) for i in range(ITERS)]
    tgt_iter_crit = [(no_t, as_t(inp["t_real"][i]), {}) for i in range(ITERS)]
    ns = {"torch": torch, "Generator": Generator, "Critic": Critic, "optG": optG, "optC": optC, "device": torch.device("cpu"),
          "wandb": types.SimpleNamespace(log=log), "dataset_train": types.SimpleNamespace(fs=FS),
          "dataset_val": types.SimpleNamespace(fs=FS), "train_init": train_init, "d_traj_offset": d_traj_offset,
          "tbptt_len": WIN, "crit_step": 0, "gen_step": 0, "epoch": 0, "val_d_max": D_MAX_S * FS + 1,
          "evaluator": types.SimpleNamespace(add_loss=lambda o, t: None),
          "val_iter": [(as_t(inp["val_x"]), as_t(inp["val_t"]), {"delay_trajectory": torch.from_numpy(knots_to_traj(inp["val_knots"], T_VAL))})],
          "inp_iter_gen": inp_iter_gen, "inp_iter_crit": inp_iter_crit, "tgt_iter_crit": tgt_iter_crit}
    torch.set_default_dtype(dt)          # the validation pass collects its chunks in torch.empty(target.shape)
    try:
        exec(script_lines(136, 169, double), ns)
    finally:
        torch.set_default_dtype(torch.float32)
    out = {"val_pred": ns["pred"].detach().double().numpy().copy(), "val_pre_d": ns["pre_d"].detach().double().numpy().copy()}
    exec(script_lines(232, 317, double), ns)
    assert ns["crit_step"] == ITERS * NWIN == ns["gen_step"] == len(optC.grads) == len(optG.grads)
    out["crit_losses"], out["gen_losses"] = np.array(logged["loss/critic"]), np.array(logged["loss/gen"])
    for tag, module, opt in (("gen", Generator, optG), ("crit", Critic, optC)):
        keys = [k for k, _ in module.named_parameters()]
        out[f"{tag}_keys"] = keys
        for j, k in enumerate(keys):
            out[f"{tag}_grad__{k}"] = np.stack([g[j].double().numpy() for g in opt.grads])
        for k, v in module.state_dict().items():
            out[f"{tag}_final__{k}"] = v.double().numpy().copy()
    return out, sd0


def e32(a, b, keys):
    """Worst max|ref32 - ref64| / max|ref64| over the named tensors (per optimizer step where they are stacked)."""
    worst = 0.0
    for k in keys:
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        rows = zip(x, y) if k.split("__")[0].endswith("grad") else [(x, y)]
        for r32, r64 in rows:
            if np.abs(r64).max() > 0:             # a tensor that is zero in both passes says nothing
                worst = max(worst, float(np.abs(r32 - r64).max() / np.abs(r64).max()))
            else:
                assert np.abs(r32).max() == 0, k
    return worst


def main():
    with open(os.path.join(GDIR, "g28_adversarial_configs.json"), "w") as f:
        json.dump({str(n): AdversarialConfig.main(n) for n in CONFIGS}, f, indent=1, sort_keys=True)
        f.write("\n")
    torch.set_num_threads(4)
    rng = np.random.default_rng(SEED)
    T = 1024 + NWIN * WIN
    x, t = audio(rng, (3, ITERS, B, 1, T))
    vx, vt = audio(rng, (B, 1, T_VAL))
    inp = {"x_gen": x[0], "x_crit": x[1], "t_real": t[2], "traj_knots": make_knots(rng, (ITERS, 2, B), T), "val_x": vx, "val_t": vt,
           "val_knots": make_knots(rng, (B,), T_VAL)}
    r32, sd0 = run(False, inp, None)
    r64, _ = run(True, inp, sd0)
    kinds = {"crit_loss": ["crit_losses"], "gen_loss": ["gen_losses"], "val": ["val_pred", "val_pre_d"],
             "crit_grad": [k for k in r64 if k.startswith("crit_grad__")], "gen_grad": [k for k in r64 if k.startswith("gen_grad__")]}
    out = {"meta": np.array([SEED, ITERS, B, FS, WIN, NWIN, T_VAL, KNOT]), "d_min_s": np.array(D_MIN_S), "d_max_s": np.array(D_MAX_S),
           "lr": np.array(LR), "crit_layers": np.array(CRIT_PARS["layers"]), "crit_channels": np.array(CRIT_PARS["conv_channels"]),
           **inp}
    for k, v in sd0.items():
        out[f"crit_init__{k}"] = v.numpy().copy()
    for kind, keys in kinds.items():
        out[f"e32__{kind}"] = np.array(e32(r32, r64, keys))
        print(f"E32[{kind}] = {float(out[f'e32__{kind}']):.3e}   (4 E32 must stay far below 1)")
        assert 4 * float(out[f"e32__{kind}"]) < 0.05, kind
    out["gen_keys"], out["crit_keys"] = np.array(r64["gen_keys"]), np.array(r64["crit_keys"])
    for k, v in r64.items():
        if k.endswith("_keys"):
            continue
        out[f"ref64__{k}"] = v if k.endswith("_losses") else v.astype(np.float32)
    for k in ["crit_losses", "gen_losses"] + [k for k in r32 if k.startswith("crit_final__")]:
        out[f"ref32__{k}"] = r32[k] if k.endswith("_losses") else r32[k].astype(np.float32)
    path = os.path.join(GDIR, "g28_adversarial.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    print("critic losses  ref32", r32["crit_losses"], "\n               ref64", r64["crit_losses"])
    print("generator losses ref32", r32["gen_losses"], "\n                 ref64", r64["gen_losses"])


if __name__ == "__main__":
    main()
