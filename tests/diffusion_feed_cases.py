"""What tests/test_diffusion_feed_cpu.py, tests/test_gpu_diffusion_feed.py and tools/make_goldens_diffusion_feed.py share: the
synthetic training files of golden g31, the three dataset cases on them, and the error bound of the decimating feeder kernel.

The files are 16-bit PCM written by a seeded generator in integer arithmetic only (numpy's frozen RandomState stream, sums and
integer divisions), so every platform writes the same bytes: a slow random trajectory (white integers through two box filters
with a first null at 25 Hz: content that survives the resample to 100 Hz), a DC offset per file (the mean subtraction has
something to remove) and a few LSB of white noise.  Per set three files of unequal lengths, the second one stereo; their names
match both `target*.wav` (TapeHissdset) and `*.wav` (ToyTrajectories)."""
import functools
import os

import numpy as np
import torch
from scipy.io import wavfile

from ntm_amd import datasets_diffusion, diffusion

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_diffusion_feed.npz")
SEED = 31
# set -> sampling rate and the longest segment cut from it; a file is `longest + extra` samples
SETS = {"44k": (44100, 225792), "192k": (192000, 983040)}
EXTRA = (4099, 30011, 12345)
NAMES = ("target_0_a.wav", "target_1_b.wav", "target_2_c.wav")
DC = (500, -300, 120)
# case -> (class, set, seg_len, sampling rate the trainer asks for): the noise net, the toy trajectories (441 : 1), the
# trajectories (1920 : 1)
CASES = {"hiss": ("TapeHissdset", "44k", 65536, 44100), "toy": ("ToyTrajectories", "44k", 225792, 100),
         "traj": ("ToyTrajectories", "192k", 983040, 100)}
N_PICKS, N_BATCHES, BATCH = 24, 3, 4


def _trajectory(rs, n, w):
    r = rs.randint(-30000, 30001, n + 2 * w).astype(np.int64)
    for _ in range(2):
        c = np.concatenate(([0], np.cumsum(r)))
        r = (c[w:] - c[:-w]) // w
    return r[:n]


def write_wavs(folder, which):
    """The three files of set `which` ("44k" | "192k") into `folder` -> folder."""
    fs, longest = SETS[which]
    rs = np.random.RandomState(SEED + fs)
    os.makedirs(folder, exist_ok=True)
    for i, name in enumerate(NAMES):
        n = longest + EXTRA[i]
        chans = []
        for _ in range(2 if i == 1 else 1):
            chans.append(_trajectory(rs, n, fs // 25) + DC[i] + rs.randint(-8, 9, n))
        a = np.clip(np.stack(chans, 1) if len(chans) > 1 else chans[0], -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(folder, name), fs, a)
    return folder


@functools.lru_cache(None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def dset_args(folder, case):
    _, which, seg_len, _ = CASES[case]
    return diffusion.Config(path=str(folder), fs=SETS[which][0], seg_len=seg_len, num_workers=0)


def dataset(folder, case, **kw):
    """The case's dataset on `folder`, its files in the order the reference saw them when g31 was recorded (glob.glob's order is
    the file system's)."""
    ds = getattr(datasets_diffusion, CASES[case][0])(dset_args(folder, case), **kw)
    order = str(golden()[f"{case}_order"]).split(";")
    assert sorted(os.path.basename(p) for p in ds.train_samples) == sorted(order)
    ds.train_samples = [os.path.join(str(folder), n) for n in order]
    return ds


def picks(case):
    return [tuple(int(v) for v in p) for p in golden()[f"{case}_picks"]]


def decimate_reference(x64, ker, orig, width):
    """x64 (B, L) float64 raw crops, ker (taps,) float32 -> (the fp64 result of torchaudio's rule on x - mean64, the bound of an
    fp32 evaluation of it).  bound = (n + 1) 2^-24 sum_k |ker_k xz_k| + 2^-24 |mean64| sum_k |ker_k|, n the taps inside the
    crop, sums over those taps: it holds for any summation order at fp32 or better, with one rounding of the mean."""
    x64 = torch.as_tensor(x64, dtype=torch.float64)
    k64 = torch.as_tensor(ker, dtype=torch.float64).reshape(1, 1, -1)
    mean = x64.mean(-1, keepdim=True)
    xz = x64 - mean
    ref = diffusion.apply_resample_kernel(xz, k64, orig, 1, width)
    s_abs = diffusion.apply_resample_kernel(xz.abs(), k64.abs(), orig, 1, width)
    ones = torch.ones_like(xz)
    n_in = diffusion.apply_resample_kernel(ones, torch.ones_like(k64), orig, 1, width)
    k_in = diffusion.apply_resample_kernel(ones, k64.abs(), orig, 1, width)
    bound = (n_in + 1) * 2.0 ** -24 * s_abs + 2.0 ** -24 * mean.abs() * k_in
    return ref, bound
