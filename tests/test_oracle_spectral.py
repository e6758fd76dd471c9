"""The CPU oracle of the spectral sums (oracle.stft_sums / spec_sums / mel_sums: numpy restatements that frame, window
and reflect by hand) against `torch.stft` in float64 at the EDGES of the legal parameter space: the minimum length
T - skip = n_fft/2 + 1 (one frame that reflects at both ends), lengths just around n_fft, hops that do and do not divide
the length or exceed the frame, windows of 2 and 3 samples, odd windows (the window is zero-padded to n_fft with the
SHORTER half on the left), and a non-zero skip.  Goldens g10 / g13 pin the oracle at the auraloss shapes only; the GPU
tests of tests/test_gpu_spectral.py lean on it everywhere else, so it is pinned everywhere else here.
Both sides are float64: they differ by the order of the additions only (worst observed 2e-14), the bar is 1e-10."""
import numpy as np
import pytest

import oracle
from helpers import STFT_FRAMES_PER_ITERATION, noise_pair, structural_cases, torch_mel_sums, torch_spec_sums, torch_stft_sums

RTOL = 1e-10
N_FFTS = (64, 128, 256, 512, 1024, 2048)
SKIPS = (0, 5)


@pytest.fixture(scope="module", autouse=True)
def one_torch_thread():
    """Thousands of transforms of a few hundred samples each: torch's thread pool costs ten times what it saves here."""
    import torch
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def edge_grid(n_fft):
    """(L, hop, win) over L = T - skip in {n_fft/2+1, n_fft/2+2, n_fft-1, n_fft, n_fft+1, 3 n_fft+7}, hop in {small,
    n_fft/4, n_fft/4+1, n_fft+3, L, L+1} and win in {2, 3, n_fft/2-1, n_fft-1, n_fft}; `small` is 1 for the frames of 64
    and 128 samples and n_fft/32 above (a hop of 1 at 6151 samples of n_fft 2048 is 100 MB of float64 frames)."""
    small = 1 if n_fft <= 128 else n_fft // 32
    cases = []
    for L in (n_fft // 2 + 1, n_fft // 2 + 2, n_fft - 1, n_fft, n_fft + 1, 3 * n_fft + 7):
        for hop in (small, n_fft // 4, n_fft // 4 + 1, n_fft + 3, L, L + 1):
            for win in (2, 3, n_fft // 2 - 1, n_fft - 1, n_fft):
                cases.append((L, hop, win))
    return sorted(set(cases))


def worst(a, b):
    return float(np.abs(a / b - 1).max())


@pytest.mark.parametrize("n_fft", N_FFTS)
def test_stft_sums_oracle_equals_torch_stft_float64_at_the_edges(n_fft):
    bad, seen = [], 0.0
    for i, (L, hop, win) in enumerate(edge_grid(n_fft)):
        for skip in SKIPS:
            y, t = noise_pair(1000 * n_fft + i, 2, L + skip)
            so, cells_o = oracle.stft_sums(y, t, skip, n_fft, hop, win)
            st, cells_t = torch_stft_sums(y, t, skip, n_fft, hop, win)
            assert cells_o == cells_t == (1 + L // hop) * (n_fft // 2 + 1), (L, hop, win, skip)
            e = worst(so, st)
            seen = max(seen, e)
            if not e <= RTOL:
                bad.append((L, hop, win, skip, e))
    print(f"stft_sums n_fft {n_fft}: worst relative difference {seen:.2e}")
    assert not bad, bad[:10]


@pytest.mark.parametrize("n_fft", N_FFTS)
def test_spec_sums_oracle_equals_torch_stft_float64_at_the_edges(n_fft):
    """The power-spectrogram form: with its defaults (win = n_fft, hop = n_fft/4) at every edge length, and with explicit
    hop / win_length over the same grid as above."""
    bad, seen = [], 0.0
    for i, (L, hop, win) in enumerate(edge_grid(n_fft)):
        for skip in SKIPS:
            y, t = noise_pair(2000 * n_fft + i, 2, L + skip)
            runs = [(hop, win)]
            if hop == L and win == n_fft:           # once per length: the defaults
                runs.append((None, None))
            for h, w in runs:
                so, cells_o = oracle.spec_sums(y, t, skip, n_fft, h, w)
                st, cells_t = torch_spec_sums(y, t, skip, n_fft, h, w)
                assert cells_o == cells_t == (1 + L // (h or n_fft // 4)) * (n_fft // 2 + 1), (L, h, w, skip)
                e = worst(so, st)
                seen = max(seen, e)
                if not e <= RTOL:
                    bad.append((L, h, w, skip, e))
    print(f"spec_sums n_fft {n_fft}: worst relative difference {seen:.2e}")
    assert not bad, bad[:10]


@pytest.mark.parametrize("sr", [44100, 16000])
@pytest.mark.parametrize("n_mels", [8, 64, 65, 160])
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_mel_sums_oracle_equals_torch_stft_float64_projected(n_fft, n_mels, sr):
    """oracle.mel_sums against torch.stft float64 projected by oracle.mel_filterbank as it is (the filter bank itself is
    checked by tests/test_oracle.py::test_mel_filterbank_restatement): framing, padding and the projection's layout."""
    basis = oracle.mel_filterbank(sr, n_fft, n_mels)
    assert basis.shape == (n_mels, n_fft // 2 + 1)
    for i, L in enumerate((n_fft // 2 + 1, n_fft // 2 + 2, n_fft - 1, n_fft, n_fft + 1, 3 * n_fft + 7)):
        for skip in SKIPS:
            for hop in (None, n_fft // 4 + 1, L + 1):
                y, t = noise_pair(3000 * n_fft + 10 * n_mels + i, 2, L + skip)
                so, cells_o = oracle.mel_sums(y, t, skip, n_fft, hop, n_mels, sr)
                st, cells_t = torch_mel_sums(y, t, skip, n_fft, hop, basis)
                assert cells_o == cells_t == (1 + L // (hop or n_fft // 4)) * n_mels
                assert worst(so, st) <= RTOL, (L, skip, hop, worst(so, st))


def test_structural_cases_cover_what_they_claim():
    """The case generator of the GPU structural sweep (tests/test_gpu_spectral.py), checked where no GPU is needed."""
    for n_fft in N_FFTS:
        F, cases = STFT_FRAMES_PER_ITERATION[n_fft], structural_cases(n_fft)
        frames = [1 + L // hop for L, hop, _, _, _ in cases]
        assert {1, 2, F - 1, F, F + 1, 2 * F + 1} <= set(frames) and max(frames) <= 70
        assert {n_fft // 2 + 1, n_fft + 1} <= {c[0] for c in cases} and max(c[0] for c in cases) > 2 * n_fft
        assert {n_fft // 4, n_fft // 4 + 1, n_fft + 3} <= {c[1] for c in cases}
        assert any(hop == L + 1 for L, hop, _, _, _ in cases) and any(hop == L for L, hop, _, _, _ in cases)
        assert (n_fft > 128) or any(c[1] == 1 for c in cases)
        assert {c[2] for c in cases} == {2, 3, n_fft // 2 - 1, n_fft - 1, n_fft}
        assert {c[3] for c in cases} == {0, 1, 37} and {c[4] for c in cases} == {1, 3}
        assert any(win == n_fft and skip % 2 == 1 for _, _, win, skip, _ in cases)
        assert all(L + skip <= 20000 for L, _, _, skip, _ in cases)
