#!/usr/bin/env python3
"""Goldens g29: the reference's own `UNet1D` (code/networks/unet_1d.py) and `DiffusionGenerator` (code/model.py:656-891) on the
CPU with the three shipped checkpoints (weights/83, 90, 91).

Dev-only script: it imports the reference's modules at run time from a checkout given on the command line and never travels.
torchaudio is not installed where this runs, so it gets a stand-in: `transforms.Resample` holds a `kernel` buffer and applies
torchaudio's pad / strided-conv / trim rule, `functional.resample` is the same.  The checkpoints carry torchaudio's OWN filters in
those buffers; this script asserts that the restated rule reproduces every one of them to <= 1 ulp of float32 and stops if not.
The checkpoints pickle OmegaConf objects: they are read through ntm_amd.diffusion's tolerant unpickler.

Random draws: np.random.RandomState(seed).standard_normal(shape).astype(float32), one call per torch.randn of the reference, in
its order.  Every case runs twice: in float32 as the reference stands (`<case>_ref32`) and with the module and the inputs in
float64 holding the same float32 parameter values (`<case>_ref64`); the samplers' float64 runs keep the float32 schedule and gamma
(cast), so that both runs integrate the same problem.

Files (tests/golden/, each below 1 MiB):
  g29_diffusion_weights_{noise,trajectories,toytrajectories}.npz   the three `ema` dicts
  g29_diffusion_configs.json    the three YAMLs as data
  g29_diffusion.npz             trajectory net: one evaluation B = 2, T = 512 with every block's and combiner's output
                                (ev_<module name>), sample() (traj_sample), sample_long(9.3) at 100 Hz (traj_long, 3 segments),
                                schedules and gammas; toy net: one evaluation (toy_ev)
  g29_diffusion_noise.npz       noise net (at the checkpoint's depth, 6): evaluations at T = 1 024 (a bottom level of one frame), 16 384 and 32 768, sample() and outpaint_sample with seg_len = 16 384,
                                T = 3 (the epsilon branch) and a 2 048-sample mask
  g29_diffusion_long32.npz, g29_diffusion_long64.npz   the first 88 200 samples of sample_long(9.3) at 44.1 kHz

Usage:  python tools/make_goldens_diffusion.py <reference checkout>
"""
import json
import os
import sys
import types

import numpy as np
import torch
import yaml

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("NTM_REFERENCE", "")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
if not os.path.isfile(os.path.join(REF, "code", "networks", "unet_1d.py")):
    sys.exit(__doc__)
sys.path.insert(0, ROOT)
from ntm_amd import diffusion as D  # noqa: E402

NAMES = ("noise", "trajectories", "toytrajectories")
SEEDS = {"ev": 2901, "toy_ev": 2902, "traj_sample": 2903, "traj_long": 2904, "noise_ev1k": 2910, "noise_ev16k": 2905, "noise_ev32k": 2906,
         "noise_sample": 2907, "noise_outpaint": 2908, "noise_outpaint_x": 2909}


# ---- stand-ins ----
class Resample(torch.nn.Module):
    def __init__(self, orig_freq, new_freq):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        g = np.gcd(self.orig_freq, self.new_freq)
        self.o, self.n = self.orig_freq // g, self.new_freq // g
        kernel, self.width = D.sinc_resample_kernel(self.o, self.n)
        self.register_buffer("kernel", kernel)

    def forward(self, x):
        return D.apply_resample_kernel(x, self.kernel, self.o, self.n, self.width)


def functional_resample(x, orig_freq, new_freq):
    if int(orig_freq) == int(new_freq):
        return x
    return Resample(orig_freq, new_freq).to(x.device)(x)


ta = types.ModuleType("torchaudio")
ta.transforms = types.ModuleType("torchaudio.transforms")
ta.functional = types.ModuleType("torchaudio.functional")
ta.transforms.Resample, ta.functional.resample = Resample, functional_resample
sys.modules.update({"torchaudio": ta, "torchaudio.transforms": ta.transforms, "torchaudio.functional": ta.functional})
for m in ["soundfile", "librosa", "librosa.filters"]:      # imported by the reference's utilities, never used here
    sys.modules[m] = types.ModuleType(m)
sys.modules["librosa.filters"].mel = lambda *a, **k: None
sys.modules["librosa"].filters = sys.modules["librosa.filters"]
sys.path.insert(0, os.path.join(REF, "code"))
import model as refmodel  # noqa: E402  (the reference's code/model.py)
from networks import unet_1d as refunet  # noqa: E402

torch.set_num_threads(8)
REAL_RANDN = torch.randn      # the reference's `torch` IS this module's: the stand-in below is put in and taken out again


class Draws:
    """The frozen stream that stands in for torch.randn."""

    def __init__(self, seed, dtype):
        self.rs, self.dtype = np.random.RandomState(seed), dtype

    def __call__(self, *shape, device=None, **kw):
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else shape
        return torch.from_numpy(self.rs.standard_normal(shape).astype(np.float32)).to(self.dtype)


def ulp_diff(a, b):
    a, b = a.numpy().ravel(), b.numpy().ravel()
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))))


# ---- configurations and weights ----
configs, emas = {}, {}
for n in NAMES:
    with open(os.path.join(REF, "configs", f"conf_{n}.yaml")) as f:
        configs[n] = json.loads(json.dumps(D._wrap(yaml.safe_load(f))))     # `8e-4` as the float OmegaConf reads
    emas[n] = D.load_checkpoint(os.path.join(REF, "code", configs[n]["network"]["checkpoint"]))
    worst = 0.0
    for k, v in emas[n].items():
        if k.endswith("resample.kernel"):
            new, _, taps = v.shape
            orig = 1 if new > 1 else taps - 2 * {54: 25, 28: 13}[taps]
            mine, _ = D.sinc_resample_kernel(orig, new)
            assert mine.shape == v.shape, (k, mine.shape, v.shape)
            worst = max(worst, ulp_diff(mine, v.cpu()))
    print(f"{n}: {len(emas[n])} tensors, {sum(v.numel() for k, v in emas[n].items() if not k.endswith('kernel'))} parameters, "
          f"restated filters within {worst:.3f} ulp of the checkpoint's")
    if worst > 1.0:
        sys.exit(f"FINDING: the restated torchaudio filter rule is {worst} ulp from the buffers of checkpoint {n}")
    path = os.path.join(GDIR, f"g29_diffusion_weights_{n}.npz")
    np.savez_compressed(path, **{k: v.cpu().numpy() for k, v in emas[n].items()})
    print(f"  {path}: {os.path.getsize(path)} bytes")
with open(os.path.join(GDIR, "g29_diffusion_configs.json"), "w") as f:
    json.dump(configs, f, indent=1, sort_keys=True)
    f.write("\n")

# the reference calls torch.load(path, map_location=device): hand it the dict read above
# FINDING: conf_noise.yaml says depth 8, the checkpoint it names holds downs.0 .. downs.5: as shipped, the reference's strict
# load_state_dict refuses it.  Every noise case here runs the reference's class at the checkpoint's depth
NOISE_DEPTH = 1 + max(int(k.split(".")[1]) for k in emas["noise"] if k.startswith("downs."))
print(f"noise checkpoint: depth {NOISE_DEPTH}, conf_noise.yaml: depth {configs['noise']['network']['depth']}")
refmodel.torch.load = lambda path, map_location=None: {"ema": emas[[n for n in NAMES if os.path.basename(path).startswith(n + "-")][0]]}


def args_of(name, **over):
    a = D._wrap(configs[name])
    if name == "noise":
        a.network.depth = NOISE_DEPTH
    a.network.checkpoint = os.path.join(REF, "code", a.network.checkpoint)
    for k, v in over.items():
        sec, key = k.split("__")
        a[sec][key] = v
    return a


def generator(name, dtype, **over):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        g = refmodel.DiffusionGenerator(args_of(name, **over), "cpu")
    if dtype == torch.float64:
        g.network.double()
        g.schedule, g.gamma = g.schedule.double(), g.gamma.double()
    return g


def both(fn):
    """fn(dtype) -> array or dict of arrays, run in float32 and float64."""
    out = {}
    for tag, dt in (("ref32", torch.float32), ("ref64", torch.float64)):
        with torch.no_grad():
            r = fn(dt)
        for k, v in (r.items() if isinstance(r, dict) else [("", r)]):
            out[(k + "_" if k else "") + tag] = v.detach().numpy().copy()
    return out


def evaluation(name, seed, B, T, sigma, record=False):
    def run(dt):
        g = generator(name, dt)
        rs = np.random.RandomState(seed)
        x = torch.from_numpy(rs.standard_normal((B, T)).astype(np.float32)).to(dt)
        s = torch.tensor(sigma, dtype=torch.float32).reshape(-1, 1).to(dt)
        got, hooks = {}, []
        if record:
            for mn, m in g.network.named_modules():
                if isinstance(m, (refunet.ResnetBlock, refunet.CombinerDown)):
                    hooks.append(m.register_forward_hook(lambda _m, _i, o, mn=mn: got.__setitem__(mn, o)))
            # CombinerUp of the level before the last runs twice (the last level reuses it): keep the calls in order
            ups = []
            for mn, m in g.network.named_modules():
                if isinstance(m, refunet.CombinerUp):
                    hooks.append(m.register_forward_hook(lambda _m, _i, o, mn=mn: ups.append((mn, o))))
        got["out"] = g.network(x, s)
        if record:
            for mn, o in ups[:-1]:
                got[mn] = o
            got["final"] = ups[-1][1].squeeze(1)
        for h in hooks:
            h.remove()
        return got
    return run


def sampler(name, seed, what, **over):
    def run(dt):
        g = generator(name, dt, **over)
        refmodel.torch.randn = Draws(seed, dt)
        try:
            if what == "sample":
                return g.sample()
            if what == "outpaint":
                rs = np.random.RandomState(SEEDS["noise_outpaint_x"])
                xo = torch.from_numpy((rs.standard_normal((1, g.seg_len)) * g.sigma_data).astype(np.float32)).to(dt)
                mask = torch.zeros(1, g.seg_len, dtype=dt)
                mask[..., :2048] = 1
                return g.outpaint_sample(xo, mask)
            if what == "long":
                runs = []
                orig = g.resampler
                g.resampler = lambda x: (runs.append(x.clone()), orig(x))[1]
                torch.set_default_dtype(dt)     # sample_long's own buffer is torch.zeros of the default dtype
                try:
                    y = g.sample_long(9.3)
                finally:
                    torch.set_default_dtype(torch.float32)
                return {"100": runs[0], "44k": y[..., :88200]}
        finally:
            refmodel.torch.randn = REAL_RANDN
    return run


main, noise, long32, long64 = {}, {}, {}, {}
for n in NAMES:
    g = generator(n, torch.float32)
    main[f"schedule_{n}"], main[f"gamma_{n}"] = g.schedule.numpy(), g.gamma.numpy()
    main[f"keys_{n}"] = np.array(";".join(g.network.state_dict()))
    main[f"shapes_{n}"] = np.array(";".join(",".join(str(d) for d in v.shape) for v in g.network.state_dict().values()))
g = generator("noise", torch.float32, exp__seg_len=16384, diff_params__T=3)
main["schedule_noise_T3"], main["gamma_noise_T3"] = g.schedule.numpy(), g.gamma.numpy()
main["seeds"] = np.array(json.dumps(SEEDS))

EV_SIGMA = [[-1.2], [-2.1]]     # cnoise = log(sigma) / 4 of sigma = 8.2e-3 and 2.2e-4: inside the trajectory schedule
for k, v in both(evaluation("trajectories", SEEDS["ev"], 2, 512, EV_SIGMA, record=True)).items():
    main["ev_" + k] = v
main["ev_sigma"] = np.array(EV_SIGMA, np.float32)
for k, v in both(evaluation("toytrajectories", SEEDS["toy_ev"], 1, 512, [[-0.9]])).items():
    main["toy_ev_" + k] = v
for k, v in both(sampler("trajectories", SEEDS["traj_sample"], "sample")).items():
    main["traj_sample_" + k] = v
for k, v in both(sampler("trajectories", SEEDS["traj_long"], "long")).items():
    if k.startswith("100"):
        main["traj_long_" + k] = v
    else:
        (long32 if k.endswith("32") else long64)["traj_long_" + k] = v
for T, tag in ((1024, "1k"), (16384, "16k"), (32768, "32k")):      # 1 024: the bottom level of the depth-6 net is ONE frame
    for k, v in both(evaluation("noise", SEEDS[f"noise_ev{tag}"], 1, T, [[-1.5]])).items():
        noise[f"noise_ev{tag}_" + k] = v
for what in ("sample", "outpaint"):
    for k, v in both(sampler("noise", SEEDS[f"noise_{what}"], what, exp__seg_len=16384, diff_params__T=3)).items():
        noise[f"noise_{what}_" + k] = v

for fname, arrays in (("g29_diffusion.npz", main), ("g29_diffusion_noise.npz", noise), ("g29_diffusion_long32.npz", long32),
                      ("g29_diffusion_long64.npz", long64)):
    path = os.path.join(GDIR, fname)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes, {len(arrays)} arrays")
    assert size < (1 << 20), "a fixture must stay below 1 MiB"
for k in sorted(a for a in {**main, **noise, **long32} if a.endswith("ref32")):
    src = main if k in main else noise if k in noise else long32
    r64 = {**main, **noise, **long64}[k[:-2] + "64"]
    print(f"  {k[:-6]:28s} {src[k].shape}  |ref32 - ref64| / max|ref64| = {np.max(np.abs(src[k] - r64)) / np.max(np.abs(r64)):.3e}")
