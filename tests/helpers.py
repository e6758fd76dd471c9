"""Shared helpers for the test-suite: exported-weight loading for the ORACLE side."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WDIR = os.path.join(ROOT, "neural-tape-modeling_amd", "weights")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def state_dict_np(name):
    """Exported checkpoint -> {key: np.ndarray} in the reference's state_dict layout."""
    with open(os.path.join(WDIR, "manifest.json")) as f:
        man = json.load(f)[str(name)]
    blob = np.fromfile(os.path.join(WDIR, man["file"]), dtype="<f4")
    return {t["key"]: blob[t["offset"]:t["offset"] + t["count"]].reshape(t["shape"]).copy()
            for t in man["tensors"]}


def oracle_weights(name):
    import oracle
    return oracle.Weights.from_state_dict(state_dict_np(name))


def load(npz):
    return np.load(os.path.join(GOLDEN, npz), allow_pickle=False)


def validate_batches(seed, n_batches, b, t, fs):
    """The synthetic validation set of golden g18 (tools/make_goldens_validate.py), regenerated from its seed:
    [(input (b,2,t), target (b,2,t), delay trajectory (b,t) in seconds)] -- two channels like the dataset's stereo items
    (audio + pilot), so that the `[:, :1, :]` cut of validate() is exercised."""
    rng = np.random.default_rng(seed)
    out = []
    n = np.arange(t)
    for _ in range(n_batches):
        x = rng.uniform(-0.5, 0.5, (b, 2, t)).astype(np.float32)
        tgt = (0.7 * np.tanh(1.5 * x) + 0.01 * rng.standard_normal((b, 2, t))).astype(np.float32)
        f = rng.uniform(0.5, 3.0, (b, 1))
        ph = rng.uniform(0, 2 * np.pi, (b, 1))
        d = (100.0 + 45.0 * np.sin(2 * np.pi * f * n / fs * 40 + ph) + 5.0 * rng.uniform(-1, 1, (b, 1))) / fs
        out.append((x, tgt, d))
    return out


def _torch_power(x, n_fft, hop, win, dtype):
    """|torch.stft|^2 of a (B, L) array in `dtype` (centred, reflect padding, periodic Hann of `win` samples) -> torch
    tensor (B, bins, frames) in `dtype`."""
    import torch
    X = torch.stft(torch.from_numpy(np.ascontiguousarray(x)).to(dtype), n_fft, hop, win,
                   torch.hann_window(win, dtype=dtype), return_complex=True)
    return X.real ** 2 + X.imag ** 2


def torch_stft_sums(y, t, skip, n_fft, hop, win, eps=1e-8, dtype=None):
    """The four per-stream sums of ntm_stft_sums / oracle.stft_sums from `torch.stft` and the auraloss formula that
    tools/make_goldens_stft.py uses (mag = sqrt(clamp(re^2 + im^2, eps))), with the spectra and the per-cell terms in
    `dtype` (default float64) and the sums over the cells in float64 -> ((B, 4) float64, cells per stream)."""
    import torch
    dtype = dtype or torch.float64
    my = torch.sqrt(torch.clamp(_torch_power(y[:, skip:], n_fft, hop, win, dtype), min=eps))
    mt = torch.sqrt(torch.clamp(_torch_power(t[:, skip:], n_fft, hop, win, dtype), min=eps))
    terms = ((mt - my) ** 2, mt ** 2, (torch.log(my) - torch.log(mt)).abs(), (my - mt).abs())
    return torch.stack([c.double().sum(dim=(1, 2)) for c in terms], dim=1).numpy(), my.shape[1] * my.shape[2]


def torch_spec_sums(y, t, skip, n_fft, hop=None, win=None, floor=1e-5, dtype=None):
    """The same for ntm_spec_sums / oracle.spec_sums (power spectrogram: |P_y - P_t|, |log10 of the clamped powers|,
    P_t, P_y)."""
    import torch
    dtype = dtype or torch.float64
    hop = n_fft // 4 if hop is None else hop
    win = n_fft if win is None else win
    py = _torch_power(y[:, skip:], n_fft, hop, win, dtype)
    pt = _torch_power(t[:, skip:], n_fft, hop, win, dtype)
    terms = ((py - pt).abs(), (torch.log10(torch.clamp(py, min=floor)) - torch.log10(torch.clamp(pt, min=floor))).abs(), pt, py)
    return torch.stack([c.double().sum(dim=(1, 2)) for c in terms], dim=1).numpy(), py.shape[1] * py.shape[2]


def torch_mel_sums(y, t, skip, n_fft, hop, basis, floor=1e-5, dtype=None):
    """The same for ntm_mel_sums / oracle.mel_sums: the power spectrogram (window = n_fft) projected by `basis`
    [n_mels, 1 + n_fft/2], used as it is given."""
    import torch
    dtype = dtype or torch.float64
    hop = n_fft // 4 if hop is None else hop
    bm = torch.from_numpy(np.asarray(basis)).to(dtype)
    my = torch.matmul(bm, _torch_power(y[:, skip:], n_fft, hop, n_fft, dtype))          # (B, mels, frames)
    mt = torch.matmul(bm, _torch_power(t[:, skip:], n_fft, hop, n_fft, dtype))
    terms = ((my - mt).abs(), (torch.log10(torch.clamp(my, min=floor)) - torch.log10(torch.clamp(mt, min=floor))).abs(), mt, my)
    return torch.stack([c.double().sum(dim=(1, 2)) for c in terms], dim=1).numpy(), my.shape[1] * my.shape[2]


def noise_pair(seed, B, T, amp=0.3):
    """Two UNRELATED white-noise signals (B, T) float32: nothing cancels in the difference terms of the spectral sums."""
    rng = np.random.default_rng(seed)
    return ((amp * rng.standard_normal((B, T))).astype(np.float32), (amp * rng.standard_normal((B, T))).astype(np.float32))


# frames per workgroup and iteration of stft_sums_kernel (4 waves x 64/SUB frame slots)
STFT_FRAMES_PER_ITERATION = {64: 16, 128: 8, 256: 4, 512: 4, 1024: 4, 2048: 4}


def structural_cases(n_fft):
    """[(L, hop, win, skip, B)]: every frame count of {1, 2, F-1, F, F+1, 2F+1} twice -- with a hop that divides L = T - skip
    and one that does not -- from the hops {n_fft/4, n_fft/4+1, n_fft+3} (enlarged where L would fall below the minimum:
    two frames at the minimum length is hop = L); the minimum length and n_fft+1 with the short hops (and hop 1 for the
    frames of 64 / 128 samples: 34 ... 66 frames); one frame by hop = L+1.  Windows, skips and batch sizes rotate with
    coprime periods, so every window meets every skip and both batch sizes over the six frame sizes and three modes."""
    F, lmin = STFT_FRAMES_PER_ITERATION[n_fft], n_fft // 2 + 1
    hops = (n_fft // 4, n_fft // 4 + 1, n_fft + 3)
    lh, k = [], 0
    for nf in (1, 2, F - 1, F, F + 1, 2 * F + 1):
        for divides in (True, False):
            if nf == 1:
                L, hop = (lmin, lmin + 1) if divides else (n_fft + 1, n_fft + 3)
            else:
                hop = max(hops[k % 3], -(-lmin // (nf - 1)))
                k += 1
                L = (nf - 1) * hop + (0 if divides else hop // 2)
            assert 1 + L // hop == nf and L >= lmin and (nf == 1 or (L % hop == 0) == divides)
            lh.append((L, hop))
    lh += [(lmin, n_fft // 4), (lmin, n_fft // 4 + 1), (n_fft + 1, n_fft // 4), (n_fft + 1, n_fft // 4 + 1), (n_fft + 1, n_fft + 2)]
    if n_fft <= 128:
        lh += [(lmin, 1)] + ([(n_fft + 1, 1)] if n_fft == 64 else [])
    wins, skips, Bs = (2, 3, n_fft // 2 - 1, n_fft - 1, n_fft), (0, 1, 37), (1, 3)
    off = list(STFT_FRAMES_PER_ITERATION).index(n_fft)
    return [(L, hop, wins[(j + off) % 5], skips[(j + off) % 3], Bs[(j + off) % 2]) for j, (L, hop) in enumerate(lh)]


# ---- case tables and extended-precision references of the tape kernels (tests/test_gpu_tape.py; the tables are checked
# and the references pinned on the CPU by tests/test_oracle_tape.py)
TAPE_TILE = 64                                           # tape_hmag_kernel: 64 streams x 64 samples per LDS tile
TAPE_HMAG_B = (1, 63, 64, 65, 129)
TAPE_HMAG_N = (1, 2, 63, 64, 65, 127, 128, 129, 193)
TAPE_SINGLE_STREAMS = (0, 63, 64, 128)                   # of a batch of 129, each also run alone
RESAMPLE_RATIOS = ((1, 16), (16, 1), (147, 160), (160, 147), (2, 3), (3, 2))      # (orig, new)
FIR_TAPS = (1, 2, 127, 128, 129)
RECORD_SHAPES = ((1, 1), (3, 255), (2, 257))
RECORD_GRID_LIMIT = 65536 * 256                          # threads of tape_record_field_kernel's largest grid
RECORD_BIG = (3, RECORD_GRID_LIMIT // 3 + 1)             # the smallest B = 3 shape whose grid-stride loop goes round twice


def tape_walk(seed, B, N, amp=300.0):
    """Unsaturated H_mag input (B, N): the walk_small family of golden g25, amp * cumsum(randn) / 20."""
    return amp * np.cumsum(np.random.default_rng(seed).standard_normal((B, N)), axis=1) / 20.0


def tape_cut_lists(N):
    """Chunk lengths (each list sums to N) across the 64-sample tile of tape_hmag_kernel."""
    cuts = [c for c in ((1, N - 1), (63, N - 63), (64, 64, N - 128), (65, N - 65)) if min(c) > 0]
    if N == 67:
        cuts.append((1,) * 67)
    assert all(sum(c) == N for c in cuts), N
    return cuts


TAPE_CUT_N = (67, 193)


def resample_lengths(width):
    return tuple(sorted({1, 2, width - 1, width, width + 1, 255, 256, 257, 1000}))


def resample_out_lengths(N, up, down):
    """M: torchaudio's ceil(up N / down), 1, one below and one above it (ntm.h defines every i * up + p < M)."""
    full = -(-up * N // down)
    return tuple(dict.fromkeys((full, 1, max(1, full // 2), full + up + 3)))


def fir_lengths(taps):
    return tuple(sorted({1, taps - 1, taps, taps + 1, 255, 256, 257, 700} - {0}))


U53 = 2.0 ** -53


def resample_ref_ld(x, ker, width, up, down, M):
    """include/ntm.h's formula of ntm_resample_fir in numpy.longdouble:
    y[b][i*up + p] = sum_k ker[p][k] xpad[b][i*down + k], xpad[j] = x[j - width] (zero outside [0, N)), i*up + p < M
    -> (y (B, M) longdouble, s (B, M) float64 = sum_k |ker[p][k]| |xpad[i*down + k]|)."""
    x, ker = np.asarray(x, np.longdouble), np.asarray(ker, np.longdouble)
    B, N = x.shape
    taps = 2 * width + down
    assert ker.shape == (up, taps)
    o = np.arange(M)
    i, p = o // up, o % up
    j = i[:, None] * down + np.arange(taps)[None, :] - width                 # (M, taps) index into x
    ok = (j >= 0) & (j < N)
    xg = np.where(ok[None], x[:, np.clip(j, 0, N - 1)], np.longdouble(0))    # (B, M, taps)
    kg = ker[p]                                                              # (M, taps)
    return (xg * kg[None]).sum(-1), np.abs(xg * kg[None]).sum(-1).astype(np.float64)


def fir_ref_ld(x, h):
    """include/ntm.h's formula of ntm_fir_f64 without the clamp in numpy.longdouble: y[b][n] = sum_{k < taps, k <= n}
    h[k] x[b][n-k] -> (y (B, N) longdouble, s (B, N) float64 = sum |h[k]| |x[n-k]|)."""
    x, h = np.asarray(x, np.longdouble), np.asarray(h, np.longdouble)
    B, N = x.shape
    j = np.arange(N)[:, None] - np.arange(len(h))[None, :]                   # (N, taps)
    xg = np.where((j >= 0)[None], x[:, np.clip(j, 0, N - 1)], np.longdouble(0))
    return (xg * h[None, None]).sum(-1), np.abs(xg * h[None, None]).sum(-1).astype(np.float64)


def resample_input(seed, B, N):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, N))


def fir_case(taps, N, seed=0):
    """(x (2, N), h (taps,)) with outputs exactly on +-1, just inside, and far outside: h[0] = 1 passes x[0] through
    alone at n = 0, and the first samples of the rows are +-1 and +-(1 - 2^-53); the rest is noise of amplitude 3."""
    rng = np.random.default_rng(1000 * taps + N + seed)
    h = rng.uniform(-1.0, 1.0, taps) / max(1, taps) ** 0.5
    h[0] = 1.0
    x = 3.0 * rng.standard_normal((2, N))
    x[0, 0], x[1, 0] = 1.0, -1.0
    if N > taps:                      # a later sample that lands exactly on the rail: everything in its window is zero
        x[:, -taps:] = 0.0
        x[0, -1], x[1, -1] = -(1.0 - U53), 1.0 - U53
    return x, h


def bench_record(stdout, detail=True):
    """bench.py's output contract: exactly ONE JSON line on stdout, the last one, shorter than 4 KB (the driver's parser lost
    round 5's 20 KB line), naming the detail file that holds the full record.  -> (compact line dict, full record dict);
    the headline fields of the two agree."""
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and stdout.rstrip().splitlines()[-1] == lines[0], stdout[-2000:]
    assert len(lines[0]) < 4096, len(lines[0])
    c = json.loads(lines[0])
    if not detail:
        return c, None
    path = c["detail_file"] if os.path.isabs(c["detail_file"]) else os.path.join(ROOT, c["detail_file"])
    with open(path) as f:
        d = json.load(f)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "scaling", "dtype", "data"):
        assert c[k] == d[k], k
    assert c["roofline"]["frac"] == d["roofline"]["frac"] and c["roofline"]["kernel_ms"] == d["roofline"]["kernel_ms"]
    return c, d


# ---- time-domain losses (tests/test_gpu_losses.py; the references and the input conditions are pinned on the CPU by
# tests/test_oracle_losses.py)
def _loss_signals(y, t, skip):
    """(e, t) of the window [skip, T) as longdouble (2, B, n): e = t - y formed in float32, the definition the kernels and
    the oracle share."""
    y, t = np.asarray(y), np.asarray(t)
    assert y.dtype == np.float32 and t.dtype == np.float32 and y.shape == t.shape and y.ndim == 2 and 0 <= skip <= y.shape[1]
    with np.errstate(all="ignore"):
        e = t - y
    assert e.dtype == np.float32
    return np.stack([e[:, skip:], t[:, skip:]]).astype(np.longdouble)


def esr_sums_exact(y, t, skip):
    """include/ntm.h's ntm_esr_sums per stream, (B, 2) numpy.longdouble: sum (t - y)^2 | sum t^2 over [skip, T) with the
    float32 difference, squares and sums in longdouble."""
    u = _loss_signals(y, t, skip)
    return (u * u).sum(-1).T


def dcpre_sums_exact(y, t, skip, R, dtype=np.longdouble):
    """include/ntm.h's ntm_esr_dcpre_sums per stream, (B, 2) `dtype`: both e = t - y (float32) and t pass
    f[n] = (u[n] - u[n-1]) + R f[n-1] from f = 0 and u[skip-1] := 0 at sample `skip`, the pole being the float32 value of
    `R`; recursion and sums of squares in `dtype` (longdouble: 64-bit mantissa, rounding 5e-20 per operation against the
    6e-8 of the kernels' float32 filters).  A sequence of poles gives (len(R), B, 2)."""
    u = _loss_signals(y, t, skip).astype(dtype)                               # (2, B, n)
    poles = np.atleast_1d(np.asarray(R, np.float32)).astype(dtype)
    r = poles.reshape(-1, 1, 1)
    f = np.zeros((len(poles),) + u.shape[:2], dtype)
    prev, s = np.zeros(u.shape[:2], dtype), np.zeros_like(f)
    with np.errstate(all="ignore"):
        for n in range(u.shape[2]):
            cur = u[:, :, n]
            f = (cur - prev) + r * f
            s += f * f
            prev = cur
    s = np.moveaxis(s, 1, 2)                                                  # (poles, B, 2)
    return s if np.ndim(R) else s[0]


def _fam_noise_offset(rng, B, T):
    t = (rng.standard_normal((B, T)) + 0.3).astype(np.float32)
    return (t + 0.1 * rng.standard_normal((B, T))).astype(np.float32), t


def _fam_dc_small_ac(rng, B, T):
    t = (1.0 + 1e-3 * rng.standard_normal((B, T))).astype(np.float32)
    return (0.9 + 1e-3 * rng.standard_normal((B, T))).astype(np.float32), t


def _fam_step(rng, B, T):
    t = np.zeros((B, T), np.float32)
    t[:, T // 2 + 3:] = 0.7
    return (0.9 * t + 1e-3 * rng.standard_normal((B, T))).astype(np.float32), t


def _fam_slow_sine(rng, B, T):
    ph = rng.uniform(0.0, 2 * np.pi, (B, 1))
    n = np.arange(T)[None, :]
    t = (0.5 * np.sin(2e-3 * n + ph) + 0.5).astype(np.float32)
    return (0.45 * np.sin(2e-3 * n + ph + 0.1) + 0.48 + 1e-3 * rng.standard_normal((B, T))).astype(np.float32), t


def _fam_const(rng, B, T):
    lv = rng.uniform(0.2, 1.0, (B, 1))
    return np.broadcast_to(0.4 * lv, (B, T)).astype(np.float32), np.broadcast_to(lv, (B, T)).astype(np.float32)


def _fam_tight_fit(rng, B, T):
    _, t = _fam_dc_small_ac(rng, B, T)
    return (t * (1.0 + 1e-6 * rng.standard_normal((B, T)))).astype(np.float32), t


# name -> generator(rng, B, T) -> (y, t) float32 (B, T): the output / target pairs of the time-domain loss tests
LOSS_FAMILIES = {
    "noise_offset": _fam_noise_offset,     # white noise on a 0.3 offset, error 0.1 noise (test_esr_dcpre_sums_vs_oracle's inputs)
    "dc_small_ac": _fam_dc_small_ac,       # level 1.0 (output 0.9) with 1e-3 noise: the filter state stays large
    "step": _fam_step,                     # 0 -> 0.7 three samples after the middle
    "slow_sine": _fam_slow_sine,           # 0.5 sin(2e-3 n + phase) + 0.5, a phase per stream
    "const": _fam_const,                   # a level per stream: the blocker's impulse response alone
    "tight_fit": _fam_tight_fit,           # y = t (1 + 1e-6 xi) on a dc_small_ac target: t - y is a few float32 roundings
}


def loss_family(name, seed, B, T):
    y, t = LOSS_FAMILIES[name](np.random.default_rng(seed), B, T)
    return np.ascontiguousarray(y), np.ascontiguousarray(t)


R_BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))          # the largest float32 pole the entry points accept
LOSS_BAR = 2e-5                                                              # the project's bar on the DCPreESR sums
# the streaming kernel (esr_dcpre_kernel): 4 waves x 1024-sample chunks, n = T - skip
DCPRE_STRUCT_N = (0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 2048, 2049, 3073, 4095, 4096, 4097, 5121, 8192, 8193)
DCPRE_STRUCT_SKIP = (0, 7, 1024)
DCPRE_STRUCT_B, DCPRE_STRUCT_SEED = 3, 41
DCPRE_COND_N, DCPRE_COND_SKIP, DCPRE_COND_B, DCPRE_COND_SEED = (17, 1025, 4097), 5, 2, 43
DCPRE_COND_POLES = (0.0, 0.5, 0.9, 0.995)
DCPRE_GROWTH_N, DCPRE_GROWTH_B, DCPRE_GROWTH_SEED = 65536, 2, 47
DCPRE_GROWTH_FAMILIES = ("slow_sine", "dc_small_ac")
# the fused flush (gru_mfma2.hip): 64-sample tiles, skip a multiple of 4
FLUSH_FAMILIES = ("dc_small_ac", "step", "slow_sine", "const")
FLUSH_T = (1, 4, 63, 64, 65, 128, 129, 300)
FLUSH_POLES = (0.995, 0.9, 0.0)
FLUSH_SEED = 53


def flush_skips(T):
    return tuple(s for s in dict.fromkeys((0, 4, 64, 68, T // 4 * 4)) if s <= T)


def rel_err(got, want):
    """|got - want| / |want| elementwise in longdouble; 0 where both are 0, inf where only `want` is."""
    got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
    with np.errstate(all="ignore"):
        r = np.abs(got - want) / np.abs(want)
    return np.where(want == 0, np.where(got == 0, 0.0, np.inf), r).astype(np.float64)
