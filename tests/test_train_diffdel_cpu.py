"""CPU: the C entry point of the delay line's adjoint (ntm_delay_backward), the refusals of DiffDelRNN training and golden g24."""
import numpy as np
import pytest
import torch

import ntm_amd
from helpers import ROOT, load


def _trainable(m):
    for p in m.parameters():
        p.requires_grad_(True)
    return m


def test_delay_backward_is_in_the_header_and_the_binding():
    import os
    assert "ntm_delay_backward" in ntm_amd._lib._SIGNATURES
    with open(os.path.join(ROOT, "include", "ntm.h")) as f:
        h = f.read()
    assert "int ntm_delay_backward(" in h and "#define NTM_DELAY_BWD_SCAN 1" in h
    L = ntm_amd._lib.lib()
    assert L.ntm_abi_version() == 9
    assert callable(L.ntm_delay_backward)


def test_delay_backward_checks_its_arguments_on_the_host():
    L = ntm_amd._lib.lib()
    p = ntm_amd._lib.ptr
    t = torch.zeros(4)
    # negative sizes, unknown flags, null outputs / delays, aliasing: -1 before anything is enqueued
    assert L.ntm_delay_backward(None, None, None, None, None, -1, 8, 4, 0, 0, None) == -1
    assert L.ntm_delay_backward(None, None, None, None, None, 1, -8, 4, 0, 0, None) == -1
    assert L.ntm_delay_backward(None, None, None, None, None, 1, 8, -4, 0, 0, None) == -1
    assert L.ntm_delay_backward(None, None, None, None, None, 1, 8, 4, 0, 2, None) == -1
    assert L.ntm_delay_backward(p(t), p(t), None, None, None, 1, 8, 4, 0, 0, None) == -1          # null gpre
    assert L.ntm_delay_backward(p(t), None, None, p(torch.zeros(4)), None, 1, 8, 4, 0, 0, None) == -1   # null d
    assert L.ntm_delay_backward(p(t), p(t), None, p(t), None, 1, 8, 4, 0, 0, None) == -1           # gpre aliases gy
    g = torch.zeros(4)
    assert L.ntm_delay_backward(None, None, p(g), p(t), p(g), 1, 8, 4, 1, 0, None) == -1           # gbuf aliases g_newbuf
    assert L.ntm_delay_backward(None, None, None, None, None, 1, 8, 1 << 25, 0, 0, None) == -1     # D above 2^24
    assert b"ntm_delay_backward" in L.ntm_last_error()
    # nothing to do: OK without touching a device
    assert L.ntm_delay_backward(None, None, None, None, None, 0, 8, 4, 0, 0, None) == 0
    assert L.ntm_delay_backward(None, None, None, None, None, 3, 0, 0, 0, 0, None) == 0


@pytest.mark.parametrize("args,kw", [((1, 32, 1), {}), ((1, 16, 1), {}), ((1, 64, 1), {"skip": True})])
def test_unsupported_diffdel_configurations_refuse_to_train(args, kw):
    m = ntm_amd.DiffDelRNN(*args, max_delay=100, **kw)
    x = torch.zeros(2, 1, 4096)
    want = r"DiffDelRNN\(input_size=1, hidden_size=64, output_size=1, skip=False\)"

    class DS:
        fs = 44100
        max_delay = 0.001
    with pytest.raises(RuntimeError, match=want):
        m.train_epoch([(x, x, {"delay_trajectory": torch.zeros(2, 4096)})], ntm_amd.ESRLoss(),
                      torch.optim.Adam(m.parameters(), 1e-3), dataset=DS)
    with pytest.raises(RuntimeError, match=want):
        _trainable(m)(x, x)


def test_cpu_diffdel_training_names_the_device_and_the_configuration():
    m = _trainable(ntm_amd.DiffDelRNN(1, 64, 1, max_delay=100))
    x = torch.zeros(1, 1, 16)
    with pytest.raises(RuntimeError, match="DiffDelRNN training is not implemented for parameters on 'cpu'") as e:
        m(x, x)
    assert "HIP device only" in str(e.value) and "DiffDelRNN(input_size=1, hidden_size=64, output_size=1, skip=False)" in str(e.value)
    assert callable(getattr(ntm_amd.DiffDelRNN, "train_epoch", None))
    assert issubclass(ntm_amd.training.DelayLineStep, torch.autograd.Function)
    # RNN's texts are unchanged
    assert ntm_amd.training.SUPPORTED == "RNN(input_size=1, hidden_size=64, output_size=1, skip=False) on a HIP device"


def test_g24_golden_is_complete():
    inp = load("g24_train_diffdel_inputs.npz")
    assert inp["x"].shape == (2, 4, 1, 512 + 3 * 2048) and inp["t"].shape == inp["x"].shape
    assert inp["traj_s"].shape == (2, 4, 512 + 3 * 2048) and inp["traj_s"].dtype == np.float32
    seed, nb, B, T, init, win, max_delay, fs = (int(v) for v in inp["meta"])
    D = max_delay + 1
    assert (init, win, D) == (512, 2048, 552) and init < D
    from ntm_amd.utilities import nextpow2
    assert nextpow2(int(float(inp["analyser_max_delay_s"]) * fs)) == init
    d = (torch.from_numpy(inp["traj_s"]) * fs).numpy()                   # the fp32 product the reference forms
    assert d.min() >= 0 and d.max() <= D and (d[:, 3] == D).any()       # stream 3 touches d = D
    assert np.array_equal(d[:, 1], np.round(d[:, 1]))                   # stream 1: whole samples
    k = np.floor(d[:, 2])
    assert (np.diff(np.arange(d.shape[-1]) - k, axis=-1) < 0).any()     # stream 2: q = n - floor(d) not monotone
    for name in ("esr", "dcpreesr"):
        g = load(f"g24_train_diffdel_{name}.npz")
        assert len(g["losses"]) == 6 and g["grad__GRU.weight_hh_l0"].shape == (6, 192, 64)
        assert g["grad__output.weight"].shape == (6, 1, 64) and "grad__output.bias" not in g.files
        assert np.isfinite(g["epoch_loss"]) and all(np.isfinite(g["losses"]))
