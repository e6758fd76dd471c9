"""What tests/test_diffusion_cpu.py and tests/test_gpu_diffusion.py share: the g29 goldens (tools/make_goldens_diffusion.py),
generators built on the exported checkpoints, the frozen random stream and the error bar.

The bar of a float32 result: 3 x the reference's own float32-against-float64 distance on that case, both in max norm relative
to max |ref64| -- computed here from the golden, never from the code under test."""
import functools
import os

import numpy as np
import torch

from ntm_amd import diffusion

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("noise", "trajectories", "toytrajectories")
NOISE_DEPTH = 6          # what the shipped noise checkpoint holds (conf_noise.yaml says 8)
EV_BLOCKS = ("downs.0.0", "downs.0.2", "downs.1.0", "downs.1.2", "downs.2.0", "downs.2.2", "downs.3.0", "middle.0.0", "ups.0.0",
             "ups.0.2", "ups.1.0", "ups.1.2", "ups.2.0", "ups.2.2", "ups.3.0", "final")


@functools.lru_cache(None)
def arrays():
    out = {}
    for f in ("g29_diffusion.npz", "g29_diffusion_noise.npz", "g29_diffusion_long32.npz", "g29_diffusion_long64.npz"):
        with np.load(os.path.join(GOLDEN, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def seeds():
    import json
    return json.loads(str(arrays()["seeds"]))


def weights_path(name):
    return os.path.join(GOLDEN, f"g29_diffusion_weights_{name}.npz")


def config(name, **over):
    """load_config(name) pointed at the exported checkpoint; over: section__key = value."""
    a = diffusion.load_config(name)
    a.network.checkpoint = weights_path(name)
    if name == "noise":
        a.network.depth = NOISE_DEPTH
    for k, v in over.items():
        sec, key = k.split("__")
        a[sec][key] = v
    return a


NOISE_SMALL = dict(exp__seg_len=16384, diff_params__T=3)      # the goldens' noise sampler: the epsilon branch in 3 steps


def generator(name, device="cpu", **over):
    return diffusion.DiffusionGenerator(config(name, **over), device)


def normal(seed, shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def draws(seed, B, L):
    """The frozen stream of the goldens: one RandomState(seed).standard_normal((B, L)) per draw."""
    rs = np.random.RandomState(seed)
    while True:
        yield torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32))


def rel_err(got, ref64):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    return float(np.max(np.abs(got.astype(np.float64) - ref64)) / np.max(np.abs(ref64)))


def bar(case):
    a = arrays()
    r32, r64 = a[case + "_ref32"], a[case + "_ref64"]
    return 3.0 * float(np.max(np.abs(r32.astype(np.float64) - r64)) / np.max(np.abs(r64)))


def check(case, got, what=""):
    """Print the figure, then hold it against the bar."""
    e, b = rel_err(got, arrays()[case + "_ref64"]), bar(case)
    print(f"{what or case}: error {e:.3e}, bar {b:.3e}, ratio to the reference's own float32 error {3.0 * e / b:.2f}")
    assert e <= b, (case, e, b)
    return e


def outpaint_inputs(gen):
    xo = (np.random.RandomState(seeds()["noise_outpaint_x"]).standard_normal((1, gen.seg_len)) * gen.sigma_data).astype(np.float32)
    mask = torch.zeros(1, gen.seg_len)
    mask[..., :2048] = 1
    return torch.from_numpy(xo), mask
