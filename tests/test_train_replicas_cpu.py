"""CPU: the replica training path (ntm_amd.Replicas, training.GRUTrainStep with R, the *_replicas entry points of
csrc/gru_train.hip) -- the symbols, the host-side argument checks and the refusals that need no device."""
import os
import re

import pytest
import torch

import ntm_amd
from helpers import ROOT

SYMS = ("ntm_gru_train_forward_replicas", "ntm_gru_train_backward_replicas", "ntm_gru_train_reduce_replicas",
        "ntm_loss_sums_replicas", "ntm_esr_grad_replicas", "ntm_esr_dcpre_grad_replicas")


def test_replica_entry_points_are_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    for s in SYMS:
        assert s in ntm_amd._lib._SIGNATURES
        assert re.search(rf"\bint {s}\(", header), s
    assert re.search(r"#define NTM_ABI_VERSION\s+9\b", header)
    L = ntm_amd._lib.lib()
    assert L.ntm_abi_version() == 9
    for s in SYMS:
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1]


def _calls(L, R, Bper, p=None):
    """Every replica entry point with sizes (R, Bper) and the pointer `p` for every tensor."""
    return [L.ntm_gru_train_forward_replicas(*([p] * 8), R, Bper, 4, 4, 4, p, p, None),
            L.ntm_gru_train_backward_replicas(p, p, p, 4, p, p, 4, p, R, Bper, 4, p, p, None),
            L.ntm_gru_train_reduce_replicas(p, R, Bper, p, None),
            L.ntm_loss_sums_replicas(p, R, Bper, 1, p, None),
            L.ntm_esr_grad_replicas(p, p, R, Bper, 4, p, p, 1e-5, p, None),
            L.ntm_esr_dcpre_grad_replicas(p, p, R, Bper, 4, 0.995, p, p, 1e-5, p, None)]


def test_argument_checks_return_minus_one_before_anything_touches_a_device():
    L = ntm_amd._lib.lib()
    assert _calls(L, 2, 3) == [-1] * 6                        # null pointers
    # R = 0 or Bper = 0 (or negative) are refused whatever the pointers are; nothing is dereferenced on the host
    for R, Bper in ((0, 4), (4, 0), (-1, 4), (4, -1), (70000, 1), (65535, 1 << 20)):
        assert _calls(L, R, Bper, 4096) == [-1] * 6, (R, Bper)
    assert b"R and Bper must be positive" in L.ntm_last_error() or b"replicas" in L.ntm_last_error() or b"streams" in L.ntm_last_error()
    assert L.ntm_loss_sums_replicas(4096, 1, 1, 0, 4096, None) == -1
    assert L.ntm_loss_sums_replicas(4096, 1, 1, 256, 4096, None) == -1
    assert L.ntm_esr_dcpre_grad_replicas(4096, 4096, 1, 1, 4, 1.5, 4096, 4096, 1e-5, 4096, None) == -1
    assert L.ntm_esr_grad_replicas(4096, 4096, 1, 1, 4, 4096, 4096, -1.0, 4096, None) == -1
    assert L.ntm_gru_train_forward_replicas(*([4096] * 6), 4096, 4096, 1, 1, 4, 4, 4, None, 4096, None) == -1      # y aliases x
    assert L.ntm_gru_train_forward_replicas(*([4096] * 6), 4096, 8192, 1, 1, 4, 3, 4, None, 4096, None) == -1      # stride below T


def test_replicas_is_exported_and_the_nodes_are_autograd_functions():
    assert ntm_amd.Replicas is ntm_amd.model.Replicas and "Replicas" in ntm_amd.__all__
    assert issubclass(ntm_amd.training.GRUTrainStep, torch.autograd.Function)
    for cls in (ntm_amd.ESRLoss, ntm_amd.DCPreESR):
        assert callable(getattr(cls, "replicas", None))
    assert callable(ntm_amd.Replicas.train_epoch)


def test_refusals_that_need_no_device():
    with pytest.raises(ValueError, match="at least one"):
        ntm_amd.Replicas([])
    with pytest.raises(TypeError, match="all models must be RNN or all DiffDelRNN"):
        ntm_amd.Replicas([ntm_amd.RNN(1, 64, 1), ntm_amd.DiffDelRNN(1, 64, 1)])
    m = ntm_amd.RNN(1, 64, 1)
    with pytest.raises(ValueError, match="same module appears twice"):
        ntm_amd.Replicas([m, ntm_amd.RNN(1, 64, 1), m])
    a, b = ntm_amd.RNN(1, 64, 1), ntm_amd.RNN(1, 64, 1)
    b.output.weight = a.output.weight
    with pytest.raises(ValueError, match="same parameter appears twice"):
        ntm_amd.Replicas([a, b])
    with pytest.raises(RuntimeError, match="hidden_size=64"):
        ntm_amd.Replicas([ntm_amd.RNN(1, 32, 1), ntm_amd.RNN(1, 64, 1)])      # models are checked in order: configuration, then device
    with pytest.raises(RuntimeError, match=r"RNN\(input_size=1, hidden_size=64, output_size=1, skip=False\)"):
        ntm_amd.Replicas([ntm_amd.RNN(1, 64, 1, skip=True)])
    with pytest.raises(RuntimeError, match="HIP device only"):
        ntm_amd.Replicas([ntm_amd.RNN(1, 64, 1), ntm_amd.RNN(1, 64, 1)])
    with pytest.raises(RuntimeError, match="HIP device only"):
        ntm_amd.Replicas([ntm_amd.DiffDelRNN(1, 64, 1), ntm_amd.DiffDelRNN(1, 64, 1)])


def test_the_supported_configurations_are_unchanged():
    assert ntm_amd.training.SUPPORTED == "RNN(input_size=1, hidden_size=64, output_size=1, skip=False) on a HIP device"
    assert ntm_amd.training.SUPPORTED_DIFFDEL == "DiffDelRNN(input_size=1, hidden_size=64, output_size=1, skip=False) on a HIP device"
