"""The batch feeder of the diffusion trainers on the device: the ntm_segment_* kernels (csrc/segment_feed.hip) against float64 at
their edges and operating points, datasets_diffusion.DeviceSegmentFeeder against golden g31, and tools/train_diffusion.py end
to end in child processes.

Bars.  Mean: one rounding of the float64 mean, 2^-24 |mean64|, plus the error of a float64 sum of L terms (the kernel's and the
reference's), 2^-52 sum |x|.  Crop: |out - (x - mean64)| <= 2^-24 (|mean64| + |x - mean64|): one rounding of the mean and one
of the difference.  Decimate: diffusion_feed_cases.decimate_reference -- float64 apply_resample_kernel on x - mean64 on the CPU,
|err| <= (n + 1) 2^-24 sum_k |ker_k xz_k| + 2^-24 |mean64| sum_k |ker_k| with n the taps inside the crop, which holds for any
summation order at fp32 or better.  Every case is run twice (equal bits) and one of its rows alone (equal bits again)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffusion_feed_cases as C
from ntm_amd import _lib, datasets_diffusion, diffusion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    return {which: C.write_wavs(str(tmp_path_factory.mktemp("wavs" + which)), which) for which in C.SETS}


def make_bank(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(n, generator=g) + 0.3).float()


def spread(bank_len, L, B):
    """B starts: 0, ..., the last one with start + L == bank_len."""
    last = bank_len - L
    return [(last * b) // max(B - 1, 1) for b in range(B)] if B > 1 else [last // 2]


def run(bank_d, starts, L, filt=None):
    """-> (mean (B,), out) of the raw entry points; filt = (ker (taps,) on the device, orig, width) decimates, None crops."""
    lib, B, st, stream = _lib.lib(), len(starts), _lib.i64_array(starts), _lib.current_stream()
    mean = torch.full((B,), 7.0, device="cuda")
    _lib.check(lib.ntm_segment_mean(_lib.ptr(bank_d), bank_d.numel(), st, B, L, _lib.ptr(mean), stream), "ntm_segment_mean")
    if filt is None:
        out = torch.full((B, L), 7.0, device="cuda")
        _lib.check(lib.ntm_segment_crop(_lib.ptr(bank_d), bank_d.numel(), st, _lib.ptr(mean), B, L, _lib.ptr(out), stream),
                   "ntm_segment_crop")
    else:
        ker, orig, width = filt
        out = torch.full((B, -(-L // orig)), 7.0, device="cuda")
        _lib.check(lib.ntm_segment_decimate(_lib.ptr(bank_d), bank_d.numel(), st, _lib.ptr(mean), B, L, _lib.ptr(ker), orig, width,
                                            ker.numel(), _lib.ptr(out), stream), "ntm_segment_decimate")
    return mean, out


def repeat_and_alone(bank_d, starts, L, filt, mean, out):
    mean2, out2 = run(bank_d, starts, L, filt)
    assert torch.equal(mean2, mean) and torch.equal(out2, out), "a second call gives other bits"
    for b in sorted({0, len(starts) // 2, len(starts) - 1}):
        m1, o1 = run(bank_d, [starts[b]], L, filt)
        assert torch.equal(m1[0], mean[b]) and torch.equal(o1[0], out[b]), f"row {b} alone gives other bits"


def crops64(bank, starts, L):
    return torch.stack([bank[s:s + L] for s in starts]).double()


def check_crop(bank, starts, L, mean, out):
    x = crops64(bank, starts, L)
    m64 = x.mean(-1, keepdim=True)
    e_mean = (mean.double().cpu()[:, None] - m64).abs()
    assert bool((e_mean <= 2.0 ** -24 * m64.abs() + 2.0 ** -52 * x.abs().sum(-1, keepdim=True)).all()), float(e_mean.max())
    err, bound = (out.double().cpu() - (x - m64)).abs(), 2.0 ** -24 * (m64.abs() + (x - m64).abs())
    ratio = float((err / bound).max())
    print(f"crop L = {L}: worst ratio to the bound {ratio:.3f}")
    WORST["crop"] = max(WORST.get("crop", 0.0), ratio)
    assert bool((err <= bound).all()), ratio


def check_decimate(x64, ker, orig, width, out, what, ref=None):
    want, bound = C.decimate_reference(x64, ker, orig, width)
    want = want if ref is None else ref
    assert out.shape == want.shape == (x64.shape[0], -(-x64.shape[1] // orig)), (out.shape, want.shape)
    err = (out.double().cpu() - want).abs()
    ratio = float((err / bound).max())
    print(f"decimate {what}: worst ratio to the bound {ratio:.2e}, max |err| {float(err.max()):.3e}, max |ref| {float(want.abs().max()):.3e}")
    WORST["decimate"] = max(WORST.get("decimate", 0.0), ratio)
    assert bool((err <= bound).all()), ratio


def filter_of(orig):
    ker, width = diffusion.sinc_resample_kernel(orig, 1)
    ker = ker.reshape(-1)
    assert ker.numel() == 2 * width + orig
    return ker, width


@pytest.mark.parametrize("L", [1, 2, 255, 256, 257, 65536])
def test_mean_and_crop_against_float64(L):
    bank = make_bank(3 * L + 17, L)
    starts = spread(bank.numel(), L, 3)
    assert starts[0] == 0 and starts[-1] + L == bank.numel()
    bank_d = bank.cuda()
    mean, out = run(bank_d, starts, L)
    check_crop(bank, starts, L, mean, out)
    repeat_and_alone(bank_d, starts, L, None, mean, out)


@pytest.mark.parametrize("orig,L,B", [(2, 1, 3), (2, 7, 3), (3, 64, 3), (441, 440, 3), (441, 441, 3), (441, 442, 3), (441, 4411, 3),
                                      (1920, 5765, 3), (441, 225792, 4), (1920, 983040, 2), (3, 64, 65)])
def test_decimate_against_float64(orig, L, B):
    ker, width = filter_of(orig)
    bank = make_bank(L + 4099 if L > 100000 else B * L + 29, orig + L + B)
    starts = spread(bank.numel(), L, B) if B <= 4 else [(7 * b) % (bank.numel() - L) for b in range(B - 1)] + [bank.numel() - L]
    assert min(starts) == 0 and max(starts) + L == bank.numel()
    bank_d = bank.cuda()
    filt = (ker.cuda(), orig, width)
    mean, out = run(bank_d, starts, L, filt)
    check_decimate(crops64(bank, starts, L), ker, orig, width, out, f"orig = {orig}, L = {L}, B = {B}")
    repeat_and_alone(bank_d, starts, L, filt, mean, out)


def test_the_raw_entry_points_refuse_and_write_nothing():
    lib, stream = _lib.lib(), _lib.current_stream()
    bank = make_bank(100, 1).cuda()
    ker, width = filter_of(3)
    ker = ker.cuda()
    mean, out = torch.full((2,), 7.0, device="cuda"), torch.full((2, 10), 7.0, device="cuda")
    ok, past, neg = _lib.i64_array([0, 90]), _lib.i64_array([0, 91]), _lib.i64_array([-1, 0])
    p = _lib.ptr
    calls = [("ntm_segment_mean", lambda: lib.ntm_segment_mean(p(bank), 100, past, 2, 10, p(mean), stream)),
             ("ntm_segment_mean", lambda: lib.ntm_segment_mean(p(bank), 100, neg, 2, 10, p(mean), stream)),
             ("ntm_segment_mean", lambda: lib.ntm_segment_mean(p(bank), 100, ok, 2, 0, p(mean), stream)),
             ("ntm_segment_mean", lambda: lib.ntm_segment_mean(None, 100, ok, 2, 10, p(mean), stream)),
             ("ntm_segment_crop", lambda: lib.ntm_segment_crop(p(bank), 100, past, p(mean), 2, 10, p(out), stream)),
             ("ntm_segment_crop", lambda: lib.ntm_segment_crop(p(bank), 100, ok, None, 2, 10, p(out), stream)),
             ("ntm_segment_crop", lambda: lib.ntm_segment_crop(p(bank), 9, ok, p(mean), 2, 10, p(out), stream)),
             ("ntm_segment_decimate", lambda: lib.ntm_segment_decimate(p(bank), 100, past, p(mean), 2, 10, p(ker), 3, width, ker.numel(), p(out), stream)),
             ("ntm_segment_decimate", lambda: lib.ntm_segment_decimate(p(bank), 100, ok, p(mean), 2, 10, p(ker), 3, width, ker.numel() - 1, p(out), stream)),
             ("ntm_segment_decimate", lambda: lib.ntm_segment_decimate(p(bank), 100, ok, p(mean), 2, 10, p(ker), 0, width, 2 * width, p(out), stream)),
             ("ntm_segment_decimate", lambda: lib.ntm_segment_decimate(p(bank), 100, ok, p(mean), 2, 10, None, 3, width, ker.numel(), p(out), stream)),
             ("ntm_segment_decimate", lambda: lib.ntm_segment_decimate(p(bank), 100, ok, p(mean), 2, 0, p(ker), 3, width, ker.numel(), p(out), stream))]
    for name, call in calls:
        rc, msg = call(), lib.ntm_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":"), (name, rc, msg)
    torch.cuda.synchronize()
    assert bool((mean == 7.0).all()) and bool((out == 7.0).all())


@pytest.mark.parametrize("case", list(C.CASES))
def test_feeder_draws_the_references_picks(folders, case):
    ds = C.dataset(folders[C.CASES[case][1]], case)
    feeder = datasets_diffusion.DeviceSegmentFeeder(ds, C.BATCH, C.CASES[case][3], "cuda")
    assert feeder.bank.dtype == torch.float32 and feeder.bank.numel() == sum(C.SETS[C.CASES[case][1]][1] + e for e in C.EXTRA)
    got = []
    for _ in range(C.N_PICKS // C.BATCH):
        x = feeder.next_batch()
        got += [tuple(int(v) for v in pk) for pk in feeder.last_picks]
        assert x.shape == (C.BATCH, feeder.out_len) and x.dtype == torch.float32 and x.is_cuda
    assert got == C.picks(case)
    # the bank holds what the host classes cut their segments from
    host = iter(C.dataset(folders[C.CASES[case][1]], case))
    bank = feeder.bank.cpu()
    for (num, idx) in got[:4]:
        seg, s = next(host), feeder.offsets[num] + idx
        raw = bank[s:s + feeder.seg_len].numpy()
        assert np.array_equal(raw - np.mean(raw), seg)
    if case == "hiss":          # equal rates: the batch is the crop
        starts = [feeder.offsets[num] + idx for num, idx in got[-C.BATCH:]]
        mean, out = run(feeder.bank, starts, feeder.seg_len)
        assert torch.equal(out, x)
        check_crop(bank, starts, feeder.seg_len, mean, x)


@pytest.mark.parametrize("case", ["toy", "traj"])
def test_feeder_batches_against_the_references_float64_batches(folders, case):
    g = C.golden()
    ds = C.dataset(folders[C.CASES[case][1]], case)
    np.random.randint(1 << 31)              # the trainer's draw of torch's seed comes between the seeding and the batches
    feeder = datasets_diffusion.DeviceSegmentFeeder(ds, C.BATCH, C.CASES[case][3], "cuda")
    ker, bank = feeder.kernel.reshape(-1).cpu(), feeder.bank.cpu()
    for i in range(C.N_BATCHES):
        x = feeder.next_batch()
        assert [tuple(int(v) for v in pk) for pk in feeder.last_picks] == [tuple(int(v) for v in pk) for pk in g[f"{case}_batch_picks"][C.BATCH * i:C.BATCH * (i + 1)]]
        starts = [feeder.offsets[num] + int(idx) for num, idx in feeder.last_picks]
        check_decimate(crops64(bank, starts, feeder.seg_len), ker, feeder.orig, feeder.width, x, f"{case} batch {i} against g31",
                       ref=torch.from_numpy(g[f"{case}_batch64"][i]))


def _drive(args, limit=240):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "tools", "train_diffusion.py")] + args,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_the_driver_trains_checkpoints_repeats_and_resumes(folders, tmp_path):
    import yaml
    cfg = json.loads(json.dumps(diffusion.load_config("toytrajectories")))
    cfg["train"]["save_interval"] = 2
    with open(tmp_path / "conf.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    base = ["--MODE", "toy_trajectories", "--CONFIG", str(tmp_path / "conf.yaml"), "--DSET_PATH", folders["44k"]]
    runs = []
    for tag in ("a", "b"):
        lines = _drive(base + ["--MODEL_DIR", str(tmp_path / tag), "--MAX_IT", "4"])
        assert [ln["it"] for ln in lines] == [0, 1, 2, 3, 4] and all(np.isfinite(ln["loss"]) for ln in lines), lines
        assert sorted(os.listdir(tmp_path / tag)) == ["toytrajectories-2.pt", "toytrajectories-4.pt"]
        runs.append(lines)
    assert runs[0] == runs[1]
    for name in ("toytrajectories-2.pt", "toytrajectories-4.pt"):
        a, b = (torch.load(tmp_path / tag / name, map_location="cpu", weights_only=False) for tag in ("a", "b"))
        assert a["it"] == b["it"] == int(name[-4])
        for part in ("network", "ema"):
            assert list(a[part]) == list(b[part]) and all(torch.equal(a[part][k], b[part][k]) for k in a[part]), (name, part)
        sa, sb = a["optimizer"]["state"], b["optimizer"]["state"]
        assert list(sa) == list(sb) and len(sa) > 0 and a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"]
        assert all(torch.equal(sa[k][n], sb[k][n]) for k in sa for n in ("step", "exp_avg", "exp_avg_sq")), name
    cfg["train"]["resume"] = True
    with open(tmp_path / "conf.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    lines = _drive(base + ["--MODEL_DIR", str(tmp_path / "a"), "--MAX_IT", "5"])
    assert [ln["it"] for ln in lines] == [4, 5] and all(np.isfinite(ln["loss"]) for ln in lines), lines


def test_print_the_worst_ratios():
    print("worst ratios to the bounds over this module's cases:", json.dumps(WORST))
