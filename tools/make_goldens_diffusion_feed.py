#!/usr/bin/env python3
"""Golden g31: the reference's batch path of the diffusion trainers -- code/datasets_diffusion.py and Trainer.get_batch of
code/train-diffusion.py -- on synthetic files.

Dev-only script, set up as tools/make_goldens_diffusion_train.py is: it reads the reference's two scripts from a checkout given on
the command line, executes them as they stand and never travels.  What is not installed where this runs gets stand-ins:
soundfile (a scipy reader that returns float64 like sf.read: 16-bit PCM over 32768, (N,) or (N, C)), omegaconf, the package
edm.torch_utils (training_stats.report returns its value and keeps the losses), and torchaudio.  THE RESAMPLE IS THE PROJECT'S
RESTATEMENT OF TORCHAUDIO'S RULE (ntm_amd.diffusion.sinc_resample_kernel / apply_resample_kernel), NOT TORCHAUDIO ITSELF: the rule
is pinned by the buffers of the reference's checkpoints only for the ratios 2 and 4 of the networks' resamplers; at 441 : 1 and
1920 : 1 it is the published formula, restated.  The dataset classes and Trainer.get_batch run unmodified.

The files are those of tests/diffusion_feed_cases.py (seeded 16-bit PCM, three per set, one stereo, unequal lengths), written
into a temporary folder.  Cases: hiss (TapeHissdset, 44.1 kHz, segments of 65 536), toy (ToyTrajectories, 44.1 kHz -> 100 Hz,
225 792 samples -> 512) and traj (ToyTrajectories, 192 kHz -> 100 Hz, 983 040 -> 512).

Recorded in tests/golden/g31_diffusion_feed.npz, per case:
  <case>_order      the base names of train_samples in the order the reference saw them (glob.glob's: the file system's)
  <case>_picks      the first 24 (file index, crop index) pairs, from the reference's own calls of random.randint and
                    np.random.randint, recorded while its __iter__ runs
  <case>_mean, _head, _tail, _sum64   of each of those 24 segments as yielded: np.mean (float32), the first and last 64 samples,
                    the sum in float64
  <case>_batch32, _batch64 (toy, traj)   three batches of get_batch (4, 512) through a DataLoader with num_workers=0, in _main's
                    order (the dataset seeds, the Trainer draws torch's seed from np.random, the batches draw): as returned, and
                    the same segments with the resample run in float64; <case>_batch_picks: their 12 picks
  toy_loss32, toy_loss64   the losses of three iterations of the reference's Trainer (train_step, update_ema, it += 1) on the toy
                    case with num_workers=0, on the network g30 exports; in float32 as the reference stands, and with the
                    network and the batch in float64

usage: python tools/make_goldens_diffusion_feed.py <reference checkout>"""
import contextlib
import io
import math
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from scipy.io import wavfile

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("NTM_REFERENCE", "")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REF, "code", "train-diffusion.py")
if not os.path.isfile(SCRIPT):
    sys.exit(__doc__)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ntm_amd import diffusion as D  # noqa: E402
import diffusion_feed_cases as C  # noqa: E402
import diffusion_train_cases as T  # noqa: E402


def resample(x, o, n):
    if int(o) == int(n):
        return x
    g = math.gcd(int(o), int(n))
    kernel, width = D.sinc_resample_kernel(o, n)
    return D.apply_resample_kernel(x, kernel, int(o) // g, int(n) // g, width)


def sf_read(file):
    fs, a = wavfile.read(file)
    assert a.dtype == np.int16
    return a.astype(np.float64) / 32768.0, fs


def module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample as the reference's UNet1D uses it: the filter as a buffer."""

    def __init__(self, orig_freq, new_freq):
        super().__init__()
        g = math.gcd(int(orig_freq), int(new_freq))
        self.o, self.n = int(orig_freq) // g, int(new_freq) // g
        kernel, self.width = D.sinc_resample_kernel(self.o, self.n)
        self.register_buffer("kernel", kernel)

    def forward(self, x):
        return D.apply_resample_kernel(x, self.kernel, self.o, self.n, self.width)


losses = []
module("torchaudio", transforms=module("torchaudio.transforms", Resample=Resample),
       functional=module("torchaudio.functional", resample=resample))
module("soundfile", read=sf_read)
module("omegaconf", OmegaConf=type("OmegaConf", (), {"load": staticmethod(D.load_config)}))
module("edm", torch_utils=module("edm.torch_utils", training_stats=module(
    "edm.torch_utils.training_stats", report=lambda name, value: (losses.append(value) if name == "loss" else None, value)[1])))
sys.path.insert(0, os.path.join(REF, "code"))
import datasets_diffusion as ref_ds  # noqa: E402  -- the reference's, unmodified
ref = types.ModuleType("ref_train_diffusion")
ref.__file__ = SCRIPT
with open(SCRIPT) as f:
    exec(compile(f.read(), SCRIPT, "exec"), ref.__dict__)      # __name__ is not "__main__": nothing runs

torch.set_num_threads(8)
quiet = lambda: contextlib.redirect_stdout(io.StringIO())      # noqa: E731


def config(case, folder):
    args = D.load_config("noise" if case == "hiss" else "toytrajectories")
    args.dset = C.dset_args(folder, case)
    args.exp.sample_rate = C.CASES[case][3]
    return args


@contextlib.contextmanager
def recording():
    """The calls of random.randint(a, b) and np.random.randint(a, b) -- the dataset's; the Trainer's has one argument -- while
    the block runs, as ("file" | "idx", value)."""
    calls, real = [], (random.randint, np.random.randint)

    def wrap(kind, fn):
        def f(*a):
            v = fn(*a)
            if len(a) == 2:
                calls.append((kind, v))
            return v
        return f

    random.randint, np.random.randint = wrap("file", real[0]), wrap("idx", real[1])
    try:
        yield calls
    finally:
        random.randint, np.random.randint = real


def picks_of(calls):
    picks, num = [], None
    for kind, v in calls:
        if kind == "file":
            num = v
        else:
            picks.append((num, v))
    return picks


def loader(ds):
    return iter(torch.utils.data.DataLoader(dataset=ds, batch_size=C.BATCH, num_workers=0))


out = {}
with tempfile.TemporaryDirectory() as tmp:
    folders = {which: C.write_wavs(os.path.join(tmp, which), which) for which in C.SETS}
    for case, (cls, which, seg_len, fs_out) in C.CASES.items():
        folder = folders[which]
        args = config(case, folder)
        # the picks and the segments: the reference's __iter__ with its two generator calls recorded
        ds = getattr(ref_ds, cls)(args.dset)
        out[f"{case}_order"] = np.array(";".join(os.path.basename(p) for p in ds.train_samples))
        with recording() as calls:
            it = iter(ds)
            segs = [next(it) for _ in range(C.N_PICKS)]
        picks = picks_of(calls)
        out[f"{case}_picks"] = np.array(picks[:C.N_PICKS], np.int64)
        assert all(s.dtype == np.float32 and s.shape == (seg_len,) for s in segs)
        out[f"{case}_mean"] = np.array([np.mean(s) for s in segs], np.float32)
        out[f"{case}_head"] = np.stack([s[:64] for s in segs])
        out[f"{case}_tail"] = np.stack([s[-64:] for s in segs])
        out[f"{case}_sum64"] = np.array([s.astype(np.float64).sum() for s in segs])
        if case == "hiss":
            continue
        # three batches of the unmodified get_batch
        kept = []
        ds = getattr(ref_ds, cls)(args.dset)
        batches = loader(ds)
        feed = iter(lambda: (kept.append(next(batches)), kept[-1])[1], None)
        net = torch.nn.Linear(1, 1)
        with quiet(), recording() as calls:
            tr = ref.Trainer(args, feed, net, torch.optim.Adam(net.parameters()), ref.EDM(args), "cpu")      # draws torch's seed
            b32 = [tr.get_batch() for _ in range(C.N_BATCHES)]
        out[f"{case}_batch_picks"] = np.array(picks_of(calls)[:C.N_BATCHES * C.BATCH], np.int64)
        out[f"{case}_batch32"] = torch.stack(b32).numpy()
        out[f"{case}_batch64"] = torch.stack([resample(torch.Tensor(a).double(), args.dset.fs, fs_out) for a in kept]).numpy()
        assert out[f"{case}_batch32"].shape == (C.N_BATCHES, C.BATCH, 512) and out[f"{case}_batch32"].dtype == np.float32

    # three iterations of the reference's trainer on the toy case, num_workers=0, on g30's exported network
    class Trainer64(ref.Trainer):
        def get_batch(self):
            return super().get_batch().double()

    for tag, dt, cls in (("32", torch.float32, ref.Trainer), ("64", torch.float64, Trainer64)):
        args = config("toy", folders["44k"])
        ds = ref_ds.ToyTrajectories(args.dset)                  # _main's order: the dataset seeds ...
        with quiet():
            net = ref.UNet1D(args, "cpu")
        net.load_state_dict(T.init_state())
        net = net.to(dt)
        opt = torch.optim.Adam(net.parameters(), lr=args.train.lr, betas=(args.train.optimizer.beta1, args.train.optimizer.beta2),
                               eps=args.train.optimizer.eps)
        del losses[:]
        with quiet():
            tr = cls(args, loader(ds), net, opt, ref.EDM(args), "cpu")      # ... the Trainer draws torch's seed ...
            for _ in range(3):                                              # ... the batches draw
                tr.train_step()
                tr.update_ema()
                tr.it += 1
        out[f"toy_loss{tag}"] = np.array(losses, np.float64)

path = C.GOLDEN
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print(f"{path}: {size} bytes, {len(out)} arrays")
assert size < (1 << 20), "a fixture must stay below 1 MiB"
for case in C.CASES:
    print(case, str(out[f"{case}_order"]), out[f"{case}_picks"][:4].tolist())
print("loss32", out["toy_loss32"], "loss64", out["toy_loss64"])
for case in ("toy", "traj"):
    a, b = out[f"{case}_batch32"].astype(np.float64), out[f"{case}_batch64"]
    print(case, "batch32 against batch64, max |diff| / max |ref|:", float(np.abs(a - b).max() / np.abs(b).max()), "max |ref|", float(np.abs(b).max()))
