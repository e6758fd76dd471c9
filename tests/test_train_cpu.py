"""CPU: the refusals of the training path (RNN.train_epoch, training.py) and the build-time checks of csrc/gru_train.hip."""
import os
import subprocess
import sys

import pytest
import torch

import ntm_amd
from helpers import ROOT


def _trainable(m):
    for p in m.parameters():
        p.requires_grad_(True)
    return m


def test_train_epoch_on_a_cpu_model_raises_hip_device_only():
    m = ntm_amd.RNN(1, 64, 1)
    x = torch.zeros(2, 1, 2048)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.train_epoch([(x, x, None)], ntm_amd.ESRLoss(), torch.optim.Adam(m.parameters(), 1e-3))


@pytest.mark.parametrize("args,kw", [((1, 32, 1), {}), ((1, 16, 1), {}), ((2, 64, 1), {}), ((1, 64, 3), {}), ((1, 64, 1), {"skip": True})])
def test_unsupported_configurations_refuse_to_train(args, kw):
    m = ntm_amd.RNN(*args, **kw)
    x = torch.zeros(2, args[0], 2048)
    with pytest.raises(RuntimeError, match=r"RNN\(input_size=1, hidden_size=64, output_size=1, skip=False\)"):
        m.train_epoch([(x, x, None)], ntm_amd.ESRLoss(), torch.optim.Adam(m.parameters(), 1e-3))
    # a forward with grad-requiring parameters is refused as well (never a silently non-differentiable result)
    with pytest.raises(RuntimeError, match="hidden_size=64"):
        _trainable(m)(x)


def test_diffdel_rnn_with_grad_requiring_parameters_refuses():
    m = _trainable(ntm_amd.DiffDelRNN(1, 64, 1, max_delay=100))
    x = torch.zeros(1, 1, 16)
    with pytest.raises(RuntimeError, match="DiffDelRNN training is not implemented"):
        m(x, x)


def test_parameters_do_not_require_grad_by_default_and_train_epoch_is_there():
    for m in (ntm_amd.RNN(1, 64, 1), ntm_amd.DiffDelRNN(1, 64, 1)):
        assert not any(p.requires_grad for p in m.parameters())
    assert callable(getattr(ntm_amd.RNN, "train_epoch", None)) and issubclass(ntm_amd.training.GRUTrainStep, torch.autograd.Function)


def test_gru_train_kernels_run_dpp_with_full_exec():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_exec.py"),
                        os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "gru_train.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_training_entry_points_are_in_the_header_and_the_binding():
    syms = set(ntm_amd._lib._SIGNATURES)
    for s in ("ntm_gru_train_workspace_floats", "ntm_gru_train_forward", "ntm_gru_train_backward", "ntm_gru_train_reduce",
              "ntm_esr_grad", "ntm_esr_dcpre_grad"):
        assert s in syms
    L = ntm_amd._lib.lib()
    assert L.ntm_abi_version() == 9
    assert L.ntm_gru_train_workspace_floats(32, 1024) == 32 * 1024 * 5 * 64
    # argument checks happen on the host, before anything touches a device
    assert L.ntm_gru_train_forward(*([None] * 8), 1, 1, 1, 1, None, None, None) == -1
    assert L.ntm_gru_train_backward(None, None, None, 1, None, None, 1, None, 1, 1, None, None, None) == -1
    assert L.ntm_gru_train_reduce(None, 1, None, None) == -1
    assert L.ntm_esr_grad(None, None, 1, 1, None, None, 1e-5, None, None) == -1
    assert L.ntm_esr_dcpre_grad(None, None, 1, 1, 1.5, None, None, 1e-5, None, None) == -1


def test_g23_golden_is_complete():
    import numpy as np
    from helpers import load
    inp = load("g23_train_inputs.npz")
    assert inp["x"].shape == (2, 4, 1, 4096) and inp["t"].shape == (2, 4, 1, 4096)
    for name in ("esr", "dcpreesr"):
        g = load(f"g23_train_{name}.npz")
        assert len(g["losses"]) == 6 and g["grad__GRU.weight_hh_l0"].shape == (6, 192, 64)
        assert np.isfinite(g["epoch_loss"]) and g["losses"][-1] < g["losses"][0]


# One bad argument for each of the ten training entry points (a single form and its `_replicas` form share one body in
# csrc/ntm_api.hip): the refusal must carry the name of the function that was called, never its sibling's.
P = 4096        # a non-null "pointer": every call below is refused before anything is dereferenced
REFUSALS = [
    ("ntm_gru_train_forward", lambda L: L.ntm_gru_train_forward(*([P] * 6), P, 2 * P, -1, 4, 4, 4, None, P, None), "negative B or T"),
    ("ntm_gru_train_forward_replicas", lambda L: L.ntm_gru_train_forward_replicas(*([P] * 6), P, 2 * P, 2, 3, -1, 4, 4, None, P, None),
     "negative T"),
    ("ntm_gru_train_forward", lambda L: L.ntm_gru_train_forward(*([P] * 6), P, P, 2, 4, 4, 4, None, P, None), "y must not alias x"),
    ("ntm_gru_train_forward_replicas", lambda L: L.ntm_gru_train_forward_replicas(*([P] * 6), P, P, 2, 3, 4, 4, 4, None, P, None),
     "y must not alias x"),
    ("ntm_gru_train_backward", lambda L: L.ntm_gru_train_backward(P, P, P, 3, P, P, 4, P, 2, 4, P, P, None), "row stride below T"),
    ("ntm_gru_train_backward_replicas", lambda L: L.ntm_gru_train_backward_replicas(P, P, P, 3, P, P, 4, P, 2, 3, 4, P, P, None),
     "row stride below T"),
    ("ntm_gru_train_reduce", lambda L: L.ntm_gru_train_reduce(P, -1, P, None), "negative B"),
    ("ntm_gru_train_reduce", lambda L: L.ntm_gru_train_reduce(None, 1, P, None), "null pointer"),
    ("ntm_gru_train_reduce_replicas", lambda L: L.ntm_gru_train_reduce_replicas(None, 2, 3, P, None), "null pointer"),
    ("ntm_gru_train_reduce_replicas", lambda L: L.ntm_gru_train_reduce_replicas(P, 0, 3, P, None), "R and Bper must be positive"),
    ("ntm_esr_grad", lambda L: L.ntm_esr_grad(P, P, 2, 4, P, P, -1.0, P, None), "bad size or eps"),
    ("ntm_esr_grad_replicas", lambda L: L.ntm_esr_grad_replicas(P, P, 2, 3, 4, P, P, -1.0, P, None), "bad size or eps"),
    ("ntm_esr_grad", lambda L: L.ntm_esr_grad(P, P, 2, 4, None, P, 1e-5, P, None), "null pointer"),
    ("ntm_esr_dcpre_grad", lambda L: L.ntm_esr_dcpre_grad(P, P, 2, 4, 1.5, P, P, 1e-5, P, None), "R must be in [0,1)"),
    ("ntm_esr_dcpre_grad_replicas", lambda L: L.ntm_esr_dcpre_grad_replicas(P, P, 2, 3, 4, 1.5, P, P, 1e-5, P, None), "R must be in [0,1)"),
    ("ntm_esr_dcpre_grad", lambda L: L.ntm_esr_dcpre_grad(P, P, 1 << 31, 4, 0.5, P, P, 1e-5, P, None), "at most 2^31 - 1 streams per call"),
    ("ntm_esr_dcpre_grad_replicas", lambda L: L.ntm_esr_dcpre_grad_replicas(P, P, 70000, 1, 4, 0.5, P, P, 1e-5, P, None),
     "at most 65535 replicas per call"),
]


@pytest.mark.parametrize("name,call,what", REFUSALS, ids=[f"{n}-{w.split()[0]}" for n, _, w in REFUSALS])
def test_every_training_entry_point_reports_its_own_name(name, call, what):
    L = ntm_amd._lib.lib()
    assert call(L) == -1
    assert L.ntm_last_error().decode() == f"{name}: {what}"
    assert set(n for n, _, _ in REFUSALS) == {e + s for e in ("ntm_gru_train_forward", "ntm_gru_train_backward", "ntm_gru_train_reduce",
                                                               "ntm_esr_grad", "ntm_esr_dcpre_grad") for s in ("", "_replicas")}


def test_single_forms_return_ok_for_an_empty_batch_without_looking_at_the_pointers():
    L = ntm_amd._lib.lib()
    assert L.ntm_gru_train_forward(*([None] * 8), 0, 4, 4, 4, None, None, None) == 0
    assert L.ntm_gru_train_forward(*([None] * 8), 3, 0, 0, 0, None, None, None) == 0
    assert L.ntm_gru_train_backward(None, None, None, 4, None, None, 4, None, 0, 4, None, None, None) == 0
    assert L.ntm_esr_grad(None, None, 0, 4, None, None, 1e-5, None, None) == 0
    assert L.ntm_esr_dcpre_grad(None, None, 3, 0, 0.5, None, None, 1e-5, None, None) == 0
    assert L.ntm_esr_grad_replicas(None, None, 2, 3, 0, None, None, 1e-5, None, None) == 0
