"""CPU: grouped inference of replicas (ntm_gru_forward_replicas, Replicas.infer / validate / predict) -- the symbol, the host-side
argument checks and the refusals that need no device."""
import os
import re
import subprocess
import sys

import pytest

import ntm_amd
from helpers import ROOT

SYM = "ntm_gru_forward_replicas"


def test_the_entry_point_is_in_the_header_and_the_binding_and_the_abi_version_stays_9():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    assert SYM in ntm_amd._lib._SIGNATURES
    assert re.search(rf"\bint {SYM}\(", header)
    assert re.search(r"#define NTM_ABI_VERSION\s+9\b", header)
    L = ntm_amd._lib.lib()
    assert L.ntm_abi_version() == 9 and ntm_amd._lib.ABI_VERSION == 9
    assert getattr(L, SYM).argtypes == ntm_amd._lib._SIGNATURES[SYM][1]
    assert len(ntm_amd._lib._SIGNATURES[SYM][1]) == 15


def test_argument_checks_return_minus_one_before_anything_touches_a_device():
    """No pointer is dereferenced on the host and nothing is enqueued: the calls return on a machine without a device."""
    L = ntm_amd._lib.lib()
    fn = getattr(L, SYM)
    p, q = 4096, 8192
    assert fn(*([None] * 8), 2, 3, 4, 4, 4, None, None) == -1                      # all-null pointers
    assert b"null pointer" in L.ntm_last_error()
    for R, Bper in ((0, 4), (4, 0), (-1, 4), (4, -1), (70000, 1), (65535, 1 << 20)):
        assert fn(*([p] * 7), q, R, Bper, 4, 4, 4, None, None) == -1, (R, Bper)
    assert fn(*([p] * 7), q, 2, 3, -1, 4, 4, None, None) == -1                     # negative T
    assert fn(*([p] * 7), q, 2, 3, 4, 3, 4, None, None) == -1                      # x stride below T
    assert fn(*([p] * 7), q, 2, 3, 4, 4, 3, None, None) == -1                      # y stride below T
    assert b"stride below T" in L.ntm_last_error()
    assert fn(*([p] * 7), p, 2, 3, 4, 4, 4, None, None) == -1                      # y aliases x
    for k in (0, 1, 2, 3, 4, 6, 7):                                               # every required pointer; b_o (5) may be null
        args = [p] * 7 + [q]
        args[k] = None
        assert fn(*args, 2, 3, 4, 4, 4, None, None) == -1, k


def test_replicas_has_the_inference_methods():
    for name in ("infer", "validate", "predict"):
        assert callable(getattr(ntm_amd.Replicas, name, None)), name
    assert callable(ntm_amd.Replicas.forward) and callable(ntm_amd.Replicas.train_epoch)


def test_a_stream_count_that_does_not_divide_by_R_names_both_numbers():
    """Replicas refuses to be constructed without a HIP device (tests/test_train_replicas_cpu.py), so the check that infer(),
    validate() and predict() share is called directly."""
    split = ntm_amd.Replicas._streams_per_replica
    assert split(6, 3, "Replicas.infer") == 2 and split(5, 1, "Replicas.infer") == 5
    with pytest.raises(ValueError, match=r"Replicas\.infer: 7 streams do not divide into 3 replicas"):
        split(7, 3, "Replicas.infer")
    with pytest.raises(ValueError, match=r"Replicas\.predict: 2 streams do not divide into 4 replicas"):
        split(2, 4, "Replicas.predict")


def test_the_low_latency_kernel_still_runs_its_dpp_with_full_exec():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_exec.py"),
                        os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "gru_lat.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
