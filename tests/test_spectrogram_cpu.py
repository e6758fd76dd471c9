"""CPU: the host side of the device spectrogram (ntm_spectrogram, ntm_spectrogram_grad) and of TimeFreqConverter -- symbols,
the argument checks (they run before anything touches a device, so they run here with made-up non-null pointers), and what
the module builds in its constructor."""
import ctypes
import re
import os

import numpy as np
import pytest
import torch

import ntm_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ntm_spectrogram", "ntm_spectrogram_grad")
# never dereferenced: every call below is refused (or is B == 0) before a device is touched
Y, GP, WS, OUT = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000))


def test_entry_points_are_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    L = ntm_amd._lib.lib()
    for s in SYMS:
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1]
    assert len(ntm_amd._lib._SIGNATURES["ntm_spectrogram"][1]) == 8
    assert len(ntm_amd._lib._SIGNATURES["ntm_spectrogram_grad"][1]) == 11
    assert re.search(r"#define\s+NTM_ABI_VERSION\s+9\b", header) and L.ntm_abi_version() == 9


def _forward(y=Y, B=1, T=600, n_fft=512, hop=128, win=512, P=OUT):
    return ntm_amd._lib.lib().ntm_spectrogram(y, B, T, n_fft, hop, win, P, None)


def _adjoint(y=Y, gP=GP, B=1, T=600, n_fft=512, hop=128, win=512, ws=WS, dy=OUT):
    return ntm_amd._lib.lib().ntm_spectrogram_grad(y, gP, B, T, n_fft, hop, win, ws, dy, 0, None)


SIZES = [dict(n_fft=500), dict(n_fft=32), dict(n_fft=4096), dict(win=0), dict(win=513), dict(hop=0), dict(T=256), dict(B=-1),
         dict(T=2 ** 31)]


@pytest.mark.parametrize("call,name,pointers", [
    (_forward, "ntm_spectrogram", [dict(y=None), dict(P=None), dict(P=Y)]),
    (_adjoint, "ntm_spectrogram_grad", [dict(y=None), dict(gP=None), dict(ws=None), dict(dy=None), dict(dy=Y)]),
])
def test_one_refusal_per_check_under_the_called_name(call, name, pointers):
    L = ntm_amd._lib.lib()
    for kw in SIZES + pointers:
        assert call(**kw) == -1, kw
        assert L.ntm_last_error().decode().startswith(name + ": "), (kw, L.ntm_last_error())


def test_the_messages_name_what_was_wrong():
    L = ntm_amd._lib.lib()
    for call in (_forward, _adjoint):
        for kw, word in ((dict(n_fft=500), "n_fft"), (dict(win=0), "win_length"), (dict(win=513), "win_length"), (dict(hop=0), "hop"),
                         (dict(T=256), "n_fft/2"), (dict(y=None), "null pointer"), (dict(T=2 ** 31), "2^31")):
            assert call(**kw) == -1 and word in L.ntm_last_error().decode(), (kw, L.ntm_last_error())
    assert _forward(P=Y) == -1 and "alias" in L.ntm_last_error().decode()
    assert _adjoint(dy=Y) == -1 and "alias" in L.ntm_last_error().decode()


def test_an_empty_batch_is_ok_with_null_pointers():
    assert _forward(y=None, P=None, B=0) == 0
    assert _adjoint(y=None, gP=None, ws=None, dy=None, B=0) == 0
    assert _forward(y=None, P=None, B=0, T=0) == 0                        # (no length check without a stream, as ntm_stft_sums)


@pytest.mark.parametrize("requires_grad", [False, True])
def test_a_cpu_tensor_is_refused(requires_grad):
    tf = ntm_amd.TimeFreqConverter(256)
    for mel in (False, True):
        with pytest.raises(RuntimeError, match="HIP device only"):
            tf(torch.zeros(2, 1, 1024, requires_grad=requires_grad), mel=mel)


@pytest.mark.parametrize("n_fft,n_mels,sr", [(2048, 160, 44100), (1024, 160, 44100), (256, 40, 16000), (64, 160, 44100)])
def test_the_dense_mel_basis_is_the_scatter_of_the_sparse_one(n_fft, n_mels, sr):
    tf = ntm_amd.TimeFreqConverter(n_fft, sampling_rate=sr, n_mel_channels=n_mels)
    assert tf.mel_basis.shape == (n_mels, n_fft // 2 + 1) and tf.mel_basis.dtype == torch.float32
    first, start, w = ntm_amd.utilities.mel_filterbank_sparse(sr, n_fft, n_mels)
    want = np.zeros((n_mels, n_fft // 2 + 1), np.float32)
    for m in range(n_mels):
        for q in range(start[m], start[m + 1]):
            want[m, first[m] + q - start[m]] = w[q]
    assert np.array_equal(tf.mel_basis.numpy(), want)
    assert int(np.count_nonzero(want)) == int(np.count_nonzero(w))
    lo = ntm_amd.TimeFreqConverter(n_fft, sampling_rate=sr, n_mel_channels=n_mels, mel_fmin=300.0, mel_fmax=sr / 4)
    f = ntm_amd.utilities.mel_filterbank_sparse(sr, n_fft, n_mels, 300.0, sr / 4)
    assert not np.array_equal(lo.mel_basis.numpy(), want) and np.count_nonzero(lo.mel_basis.numpy()) == np.count_nonzero(f[2])


def test_constructor_arguments_attributes_and_the_frame_count():
    tf = ntm_amd.TimeFreqConverter()
    assert (tf.n_fft, tf.hop_length, tf.win_length, tf.sampling_rate, tf.n_mel_channels) == (2048, 512, 2048, 44100, 160)
    assert set(dict(tf.named_buffers())) == {"window", "mel_basis"} and not list(tf.parameters())
    assert torch.equal(tf.window, torch.hann_window(2048))
    # hop_length and win_length are stored, `window` follows win_length -- and the transform's hop stays n_fft / 4
    odd = ntm_amd.TimeFreqConverter(1024, hop_length=100, win_length=600)
    assert (odd.hop_length, odd.win_length) == (100, 600) and odd.window.shape == (600,)
    for T in (513, 1024, 16384, 16385):
        assert odd.n_frames(T) == ntm_amd.TimeFreqConverter(1024).n_frames(T) == 1 + T // 256
    assert "TimeFreqConverter" in ntm_amd.__all__
