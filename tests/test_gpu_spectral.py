"""The spectral loss kernels (stft_sums_kernel behind ntm_stft_sums / ntm_spec_sums / ntm_mel_sums) against the fp64
oracle -- which tests/test_oracle_spectral.py pins to torch.stft float64 at these same edges -- where a hand-written FFT
with reflect padding by index arithmetic, frames side by side in one wave and a chunked frame loop can go wrong:
the minimum legal length, 1 / 2 / F-1 / F / F+1 / 2F+1 frames (F = frames per workgroup iteration), hops that do and do
not divide the length or exceed the frame, windows of 2 and 3 samples, odd windows and skips, mel band counts on either
side of the 64-lane stride, every chunk partition through the raw ABI, and inputs on which the shared complex FFT
(y + i t through one transform) is ill-conditioned.

Frame counts stay at or below 70 wherever sums are compared: ONE wrong frame then moves a sum by more than 1 %, two
orders above the 1e-4 bar.  On two unrelated noise signals nothing cancels in the difference terms: fp32 torch.stft stays
within 8.2e-7 of fp64 in every column and an fp32 simulation of the shared FFT within 3.9e-6, so rtol = 1e-4 (the
project's bar for these sums) leaves a 25x margin."""
import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import oracle
from helpers import STFT_FRAMES_PER_ITERATION as FPI, noise_pair, structural_cases, torch_stft_sums

pytestmark = pytest.mark.gpu
RTOL = 1e-4
SET = dict(deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
N_FFTS = tuple(FPI)
MEL_BANDS, MEL_RATES = (8, 64, 65, 160), (44100, 16000)
STFT_EPS, SPEC_FLOOR = 1e-8, 1e-5


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available()
    return ntm_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hip_sums(ntm, mode, y, t, skip, n_fft, hop, win, n_mels=None, sr=None):
    """Through the Python wrappers -> ((B, 4) float64 numpy, cells)."""
    yd, td = dev(y).unsqueeze(1), dev(t).unsqueeze(1)
    if mode == "stft":
        s, cells = ntm.stft_sums(yd, td, skip, n_fft, hop, win)
    elif mode == "spec":
        s, cells = ntm.spec_sums(yd, td, skip, n_fft, hop, win)
    else:
        assert win == n_fft
        s, cells = ntm.mel_sums(yd, td, skip, n_fft, hop, n_mels, sr)
    return s.cpu().numpy(), cells


def oracle_sums(mode, y, t, skip, n_fft, hop, win, n_mels=None, sr=None):
    if mode == "stft":
        return oracle.stft_sums(y, t, skip, n_fft, hop, win)
    if mode == "spec":
        return oracle.spec_sums(y, t, skip, n_fft, hop, win)
    return oracle.mel_sums(y, t, skip, n_fft, hop, n_mels, sr)


def rel_err(got, want):
    """Per-element |got - want| / |want| (0 where both are 0, inf where only `want` is)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(got - want) / np.abs(want)
    return np.where(got == want, 0.0, e)


def check_case(ntm, mode, seed, B, L, skip, n_fft, hop, win, n_mels=None, sr=None):
    y, t = noise_pair(seed, B, L + skip)
    got, cells = hip_sums(ntm, mode, y, t, skip, n_fft, hop, win, n_mels, sr)
    want, cells_o = oracle_sums(mode, y, t, skip, n_fft, hop, win, n_mels, sr)
    what = dict(mode=mode, B=B, L=L, skip=skip, n_fft=n_fft, hop=hop, win=win, n_mels=n_mels, sr=sr, frames=1 + L // hop)
    assert cells == cells_o, what
    assert np.isfinite(got).all() and (rel_err(got, want) <= RTOL).all(), (what, rel_err(got, want))


# ------------------------------------------------------------------------------------------ a. structural sweep
@pytest.mark.parametrize("n_fft", N_FFTS)
@pytest.mark.parametrize("mode", ["stft", "spec"])
def test_structural_sweep_stft_and_spec(ntm, mode, n_fft):
    """Frame counts around the workgroup iteration, edge lengths, hops, windows and skips (structural_cases) for the
    auraloss sums and the power-spectrogram sums: every column within 1e-4 of the oracle, cell counts equal."""
    shift = 0 if mode == "stft" else 2        # the two modes meet different (window, skip) pairs at the same (L, hop)
    cases = structural_cases(n_fft)
    for j, (L, hop, _, _, B) in enumerate(cases):
        _, _, win, skip, _ = cases[(j + shift) % len(cases)]
        check_case(ntm, mode, 100 * n_fft + j, B, L, skip, n_fft, hop, win)


@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_structural_sweep_mel(ntm, n_fft):
    """The same lengths, hops and skips for the mel sums (window = n_fft there); band counts and rates rotate."""
    for j, (L, hop, _, skip, B) in enumerate(structural_cases(n_fft)):
        check_case(ntm, "mel", 200 * n_fft + j, B, L, skip, n_fft, hop, n_fft, MEL_BANDS[j % 4], MEL_RATES[(j // 4) % 2])


# ------------------------------------------------------------------------------------------ b. chunk partition, raw ABI
def raw_sums(ntm, mode, y, t, skip, n_fft, hop, win, chunks, n_mels=None, sr=None):
    """ntm_stft_sums / ntm_spec_sums / ntm_mel_sums by ctypes, with `chunks` chosen by the caller -> (B, chunks, 4 waves, 4)
    float64 numpy.  The output starts as NaN: every row must be WRITTEN, also the rows of chunks without a frame."""
    L = ntm._lib
    B, T = y.shape
    yd, td = dev(y), dev(t)
    out = torch.full((B, chunks, 4, 4), float("nan"), device="cuda", dtype=torch.float64)
    if mode == "mel":
        from ntm_amd.utilities import mel_filterbank_sparse
        first, start, w = (dev(a) for a in mel_filterbank_sparse(sr, n_fft, n_mels))
        rc = L.lib().ntm_mel_sums(L.ptr(yd), L.ptr(td), B, T, skip, n_fft, hop, win, SPEC_FLOOR, chunks, n_mels,
                                  L.ptr(first), L.ptr(start), L.ptr(w), L.ptr(out), L.current_stream())
    elif mode == "spec":
        rc = L.lib().ntm_spec_sums(L.ptr(yd), L.ptr(td), B, T, skip, n_fft, hop, win, SPEC_FLOOR, chunks, L.ptr(out), L.current_stream())
    else:
        rc = L.lib().ntm_stft_sums(L.ptr(yd), L.ptr(td), B, T, skip, n_fft, hop, win, STFT_EPS, chunks, L.ptr(out), L.current_stream())
    L.check(rc, "ntm_%s_sums" % mode)
    return out.cpu().numpy()


CHUNK_SHAPES = [("stft", 64, 16, 60, 68 * 16 + 5), ("spec", 64, 16, 60, 68 * 16 + 5),
                ("stft", 1024, 120, 600, 39 * 120 + 50), ("spec", 1024, 120, 600, 39 * 120 + 50), ("mel", 1024, 120, 1024, 39 * 120 + 50),
                ("stft", 2048, 240, 1200, 19 * 240 + 100), ("spec", 2048, 240, 1200, 19 * 240 + 100), ("mel", 2048, 240, 2048, 19 * 240 + 100)]


@pytest.mark.parametrize("mode,n_fft,hop,win,L", CHUNK_SHAPES)
def test_chunk_partition_through_the_raw_abi(ntm, mode, n_fft, hop, win, L):
    """`chunks` of the C ABI on its own (the wrapper ties it to the shape): 69 / 40 / 20 frames split into 1, 2, 3, 7, n_frames
    and n_frames + 5 chunks.  The fp32 partial sums per lane and frame do not depend on the partition, only the order of the
    fp64 additions does: totals agree to 1e-12, rows of chunks past the last frame are exactly zero, and the one-chunk
    total is the oracle's."""
    skip, B, n_frames = 3, 2, 1 + L // hop
    mel = dict(n_mels=65, sr=44100) if mode == "mel" else {}
    y, t = noise_pair(n_fft + len(mode), B, L + skip)
    want, _ = oracle_sums(mode, y, t, skip, n_fft, hop, win, *mel.values())
    base = None
    for chunks in (1, 2, 3, 7, n_frames, n_frames + 5):
        out = raw_sums(ntm, mode, y, t, skip, n_fft, hop, win, chunks, **mel)
        assert np.isfinite(out).all(), (chunks, "a row was left unwritten")
        per = -(-n_frames // chunks)
        for c in range(chunks):
            if c * per >= n_frames:
                assert (out[:, c] == 0.0).all(), (chunks, c)
            else:       # only a guard against a chunk that did nothing: the values are carried by the 1e-12 agreement of the
                        # totals across partitions, the NaN pre-fill and the oracle comparison at chunks = 1
                assert (out[:, c, :, 2 if mode == "mel" else 1] > 0).any(), (chunks, c)
        total = out.sum(axis=(1, 2))
        if base is None:
            base = total
            assert (rel_err(total, want) <= RTOL).all(), rel_err(total, want)
        assert (rel_err(total, base) <= 1e-12).all(), (chunks, rel_err(total, base))


@pytest.mark.parametrize("mode,n_fft,hop,L", [("stft", 64, 16, 68 * 16 + 5), ("spec", 64, 16, 68 * 16 + 5), ("mel", 1024, 250, 64 * 250 + 100)])
def test_wrapper_chunking_threshold_and_many_streams(ntm, mode, n_fft, hop, L):
    """Through the Python wrappers, across their own threshold: 65 ... 69 frames are two chunks at B = 3 and one chunk at
    B = 2049 (the three streams tiled): the same sums to 1e-12, tiled copies bit-identical, and the oracle's values."""
    skip, win = 5, (n_fft if mode == "mel" else 60)
    mel = (65, 16000) if mode == "mel" else ()
    assert 64 <= 1 + L // hop <= 70
    y, t = noise_pair(7 * n_fft, 3, L + skip)
    s3, cells = hip_sums(ntm, mode, y, t, skip, n_fft, hop, win, *mel)
    want, cells_o = oracle_sums(mode, y, t, skip, n_fft, hop, win, *mel)
    assert cells == cells_o and (rel_err(s3, want) <= RTOL).all(), rel_err(s3, want)
    big, _ = hip_sums(ntm, mode, np.tile(y, (683, 1)), np.tile(t, (683, 1)), skip, n_fft, hop, win, *mel)
    assert big.shape == (2049, 4)
    assert (rel_err(big[:3], s3) <= 1e-12).all(), rel_err(big[:3], s3)
    assert (big.reshape(683, 3, 4) == big[:3]).all()


# ------------------------------------------------------------------------------------------ c. hypothesis sweep
@settings(max_examples=60, **SET)
@given(data=st.data(), mode=st.sampled_from(["stft", "spec", "mel"]), B=st.integers(1, 4), skip=st.integers(0, 50),
       seed=st.integers(0, 2**31 - 1))
def test_random_shapes_hops_windows_and_skips(ntm, data, mode, B, skip, seed):
    """Any mode, frame size, length n_fft/2 < L <= 6000, hop (at most 70 frames, down to one), window >= 2, skip and
    batch; mel band counts 1 ... 200 at three rates: within 1e-4 of the oracle on the independent pair."""
    n_fft = data.draw(st.sampled_from([1024, 2048] if mode == "mel" else list(N_FFTS)), label="n_fft")
    L = data.draw(st.one_of(st.integers(n_fft // 2 + 1, n_fft // 2 + 4), st.integers(n_fft // 2 + 1, 6000)), label="L")
    hop_min = L // 70 + 1                                      # 1 + L // hop <= 70
    hop = data.draw(st.one_of(st.integers(hop_min, min(hop_min + 20, L + 1)), st.integers(hop_min, L + 1)), label="hop")
    if mode == "mel":
        win = n_fft
        mel = (data.draw(st.integers(1, 200), label="n_mels"), data.draw(st.sampled_from([44100, 22050, 16000]), label="sr"))
    else:
        win = data.draw(st.one_of(st.integers(2, n_fft), st.sampled_from([2, 3, n_fft - 1, n_fft])), label="win")
        mel = ()
    assert 1 + L // hop <= 70
    check_case(ntm, mode, seed, B, L, skip, n_fft, hop, win, *mel)


# ------------------------------------------------------------------------------------------ d. conditioning families
COND_SHAPES = [(64, 16, 60), (512, 50, 240), (1024, 120, 600), (2048, 240, 1200)]      # one per FFT structure
FAMILIES = ("near", "tones", "y_small", "t_small", "y_zero_noise", "y_zero_tone", "silent", "dc")


def family_pair(family, seed, T):
    """(y, t), each (2, T) float32.  y + i t goes through ONE complex FFT and the two spectra are separated afterwards, so
    the rounding of the larger side leaks into the smaller one -- these are the pairs on which that could show."""
    rng = np.random.default_rng(seed)
    n = np.arange(T)
    noise = lambda a: a * rng.standard_normal((2, T))                                    # noqa: E731
    tone = lambda a, ph: a * np.sin(2 * np.pi * np.array([[1000.0], [3217.3]]) * n / 44100.0 + ph)    # noqa: E731
    if family == "near":                  # (i) prediction = target + 1 % noise: what the existing tests use
        t = noise(0.3); y = t + noise(0.003)
    elif family == "tones":               # (ii) the same frequency, slightly different amplitude and phase
        t = tone(0.8, 0.3); y = tone(0.808, 0.31)
    elif family == "y_small":             # (iii) 60 dB between the sides
        t = noise(0.3); y = noise(0.3e-3)
    elif family == "t_small":
        y = noise(0.3); t = noise(0.3e-3)
    elif family == "y_zero_noise":        # (iv) one side identically zero
        t = noise(0.3); y = np.zeros((2, T))
    elif family == "y_zero_tone":
        t = tone(1.0, 0.3); y = np.zeros((2, T))
    elif family == "silent":              # (v)
        t = np.zeros((2, T)); y = np.zeros((2, T))
    else:                                 # (vi) two unrelated signals, both on a 0.5 DC offset
        t = 0.5 + noise(0.3); y = 0.5 + noise(0.3)
    return y.astype(np.float32), t.astype(np.float32)


@pytest.fixture(scope="module")
def conditioning():
    """{family: [(case, y, t, fp64 sums, cells)], ...} and E_ref {family: (4,)}: per family and column the worst
    |fp32 - fp64| / |fp64| of torch.stft float32 on the CPU (spectra and per-cell terms in float32, the sum over the cells
    in float64 as on the device), POOLED over the four shapes, both lengths and both streams, so that one lucky small
    sample does not set the bar.  Computed once; the bars come from this reference, never from the kernel."""
    cases, e_ref = {}, {}
    for family in FAMILIES:
        cases[family], worst = [], np.zeros(4)
        for i, (n_fft, hop, win) in enumerate(COND_SHAPES):
            for L in (n_fft // 2 + 1, 3000):
                skip = 7
                y, t = family_pair(family, 1000 * i + L, L + skip)
                want, cells = oracle.stft_sums(y, t, skip, n_fft, hop, win)
                f32, _ = torch_stft_sums(y, t, skip, n_fft, hop, win, STFT_EPS, torch.float32)
                worst = np.maximum(worst, rel_err(f32, want).max(axis=0))
                cases[family].append(((n_fft, hop, win, L, skip), y, t, want, cells))
        e_ref[family] = worst
    return cases, e_ref


@pytest.mark.parametrize("family", FAMILIES)
def test_conditioning_of_the_shared_fft(ntm, conditioning, family):
    """ntm_stft_sums on the families above, four shapes x {minimum length, 3000 samples}: per column
    |hip - fp64| <= max(1e-4, 4 E_ref) |fp64| with E_ref from fp32 torch.stft (fixture) and the project's standing factor 4
    over an fp32 reference.  Silence is known exactly: columns 0, 2, 3 are 0 and column 1 is cells x eps.  With y = 0 the
    target's power (column 1) matches to 1e-6 and columns 0, 3 to 1e-4: rounding of t that leaked into Y above the clamp
    would show there.  Prints the kernel's worst error per column beside the reference's (DESIGN.md records them)."""
    cases, e_ref = conditioning
    bar = np.maximum(RTOL, 4.0 * e_ref[family])
    worst, failures = np.zeros(4), []
    for case, y, t, want, cells in cases[family]:
        n_fft, hop, win, L, skip = case
        got, cells_hip = hip_sums(ntm, "stft", y, t, skip, n_fft, hop, win)
        assert cells_hip == cells and np.isfinite(got).all(), case
        if family == "silent":
            assert (got[:, [0, 2, 3]] == 0.0).all(), (case, got)
            assert (np.abs(got[:, 1] / (cells * STFT_EPS) - 1) <= 1e-6).all(), (case, got[:, 1], cells * STFT_EPS)
            assert (want[:, [0, 2, 3]] == 0.0).all()
            continue
        e = rel_err(got, want)
        worst = np.maximum(worst, e.max(axis=0))
        if not (e <= bar).all():
            failures.append((case, e))
        if family.startswith("y_zero"):
            if not ((e[:, 1] <= 1e-6).all() and (e[:, [0, 3]] <= 1e-4).all()):
                failures.append((case, "y = 0", e))
    with np.errstate(divide="ignore", invalid="ignore"):
        row = lambda v: " ".join(f"{x:.2e}" for x in v)                                   # noqa: E731
        print(f"\nconditioning {family}: hip {row(worst)} | ref {row(e_ref[family])} | ratio {row(worst / e_ref[family])} | bar {row(bar)}")
    assert not failures, failures


# ------------------------------------------------------------------------------------------ e. mel specifics
@pytest.mark.parametrize("n_mels", MEL_BANDS)
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_mel_band_counts_around_the_lane_stride(ntm, n_fft, n_mels):
    """Lane m walks filters m, m + 64, ...: 8 (idle lanes), 64 (exactly one pass), 65 (one lane makes a second pass) and
    160 bands, at two sample rates (at 16 kHz the low filters of 160 bands are narrower than a bin of n_fft 1024), with one
    frame and with F + 1 = 5 frames (every wave one frame, the first wave a second one)."""
    for sr in MEL_RATES:
        for L, hop in ((n_fft // 2 + 1, n_fft), (n_fft + 77, n_fft // 4)):
            assert 1 + L // hop in (1, 5)
            check_case(ntm, "mel", n_fft + n_mels + sr, 2, L, 3, n_fft, hop, n_fft, n_mels, sr)


def test_mel_sums_refuses_small_frames(ntm):
    y, t = noise_pair(1, 1, 4000)
    with pytest.raises(ntm.NtmError):
        ntm.mel_sums(dev(y).unsqueeze(1), dev(t).unsqueeze(1), 0, 512)
    with pytest.raises(ntm.NtmError):
        raw_sums(ntm, "mel", y, t, 0, 512, 128, 512, 1, n_mels=8, sr=44100)


# ------------------------------------------------------------------------------------------ f. host wrappers
def test_mrstft_loss_other_resolutions_and_all_weights(ntm):
    """MRSTFTLoss with a resolution list of its own (n_fft 64 and 256 among it: frames side by side, the four-pass plan)
    and all three weights non-zero: per_segment (with a skip) and forward over the whole batch against the oracle's sums
    composed by the published formula."""
    res = ((64, 16, 48), (256, 50, 255), (1024, 120, 600))
    w_sc, w_log, w_lin = 0.7, 1.3, 0.4
    skip, L, B = 11, 1100, 3
    y, t = noise_pair(42, B, L + skip)
    loss = ntm.MRSTFTLoss([r[0] for r in res], [r[1] for r in res], [r[2] for r in res], w_sc=w_sc, w_log_mag=w_log, w_lin_mag=w_lin)
    yd, td = dev(y).unsqueeze(1), dev(t).unsqueeze(1)

    def composed(sk, whole):
        total = 0.0
        for n_fft, hop, win in res:
            s, cells = oracle.stft_sums(y, t, sk, n_fft, hop, win)
            assert cells // (n_fft // 2 + 1) <= 70
            if whole:
                s, cells = s.sum(axis=0), cells * B
            total = total + w_sc * np.sqrt(s[..., 0]) / np.sqrt(s[..., 1]) + w_log * s[..., 2] / cells + w_lin * s[..., 3] / cells
        return total / len(res)

    per = loss.per_segment(yd, td, skip).cpu().numpy()
    assert per.shape == (B,) and (rel_err(per, composed(skip, False)) <= RTOL).all(), rel_err(per, composed(skip, False))
    whole = float(loss(yd, td))
    assert abs(whole / composed(0, True) - 1) <= RTOL, (whole, composed(0, True))


def test_wrappers_edges_and_refusals(ntm):
    """An empty batch gives empty sums without a launch; T - skip = n_fft/2 is refused and n_fft/2 + 1 accepted; hop 0,
    window 0, a window longer than the frame and a zero floor are each refused with NtmError."""
    e = torch.zeros(0, 1, 4000, device="cuda")
    for fn in (ntm.stft_sums, ntm.spec_sums, ntm.mel_sums):
        s, _ = fn(e, e)
        assert tuple(s.shape) == (0, 4) and s.dtype == torch.float64
    torch.cuda.synchronize()
    y, t = noise_pair(3, 2, 600)
    yd, td = dev(y).unsqueeze(1), dev(t).unsqueeze(1)
    for n_fft in (64, 1024):
        with pytest.raises(ntm.NtmError):
            ntm.stft_sums(yd, td, 600 - n_fft // 2, n_fft, 16, n_fft)
        with pytest.raises(ntm.NtmError):
            ntm.spec_sums(yd, td, 600 - n_fft // 2, n_fft)
        sk = 600 - n_fft // 2 - 1
        s, cells = ntm.stft_sums(yd, td, sk, n_fft, 16, n_fft)
        so, cells_o = oracle.stft_sums(y, t, sk, n_fft, 16, n_fft)
        assert cells == cells_o and (rel_err(s.cpu().numpy(), so) <= RTOL).all()
    for kw in (dict(hop=0), dict(win_length=0), dict(win_length=1025), dict(eps=0.0)):
        with pytest.raises(ntm.NtmError):
            ntm.stft_sums(yd, td, 0, **{**dict(n_fft=1024, hop=120, win_length=600), **kw})
    for kw in (dict(hop=0), dict(win_length=0), dict(win_length=1025), dict(log_floor=0.0)):
        with pytest.raises(ntm.NtmError):
            ntm.spec_sums(yd, td, 0, 1024, **kw)
    for kw in (dict(hop=0), dict(log_floor=0.0)):
        with pytest.raises(ntm.NtmError):
            ntm.mel_sums(yd, td, 0, 1024, **kw)
    # the library's own checks (the wrappers refuse hop = 0 before it is called): hop, window and chunks through the raw ABI
    for mode in ("stft", "spec"):
        for hop, win, chunks in ((0, 600, 1), (-1, 600, 1), (120, 0, 1), (120, 1025, 1), (120, 600, 0)):
            with pytest.raises(ntm.NtmError):
                raw_sums(ntm, mode, y, t, 0, 1024, hop, win, chunks)
    with pytest.raises(ntm.NtmError):
        raw_sums(ntm, "mel", y, t, 0, 1024, 0, 1024, 1, n_mels=8, sr=44100)
    torch.cuda.synchronize()
