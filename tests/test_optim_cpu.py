"""CPU: the host side of the fused optimiser step (ntm_amd.optim over ntm_multi_* of include/ntm.h) -- the exports, the
constructor's checks against torch.optim.Adam's, the refusals, the state_dict exchange with torch.optim.Adam in both directions,
the argument checks of the C entry points, and the exact case of tests/optim_cases.py against fractions.Fraction and torch."""
import copy
import ctypes
import os
import re

import pytest
import torch

import ntm_amd
from ntm_amd import _lib, optim
import optim_cases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"ntm_multi_partials": 2, "ntm_multi_sqnorm": 6, "ntm_multi_clip_coef": 5, "ntm_multi_adam": 14, "ntm_multi_ema": 7}


def test_the_module_and_the_c_abi_are_exported():
    assert ntm_amd.FusedAdam is optim.FusedAdam and ntm_amd.ema_update_ is optim.ema_update_
    assert {"FusedAdam", "ema_update_", "optim"} <= set(ntm_amd.__all__)
    assert issubclass(optim.FusedAdam, torch.optim.Optimizer)
    with open(os.path.join(ROOT, "include", "ntm.h")) as f:
        header = f.read()
    L = _lib.lib()
    for s, nargs in SYMS.items():
        assert s in _lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == _lib._SIGNATURES[s][1] and len(_lib._SIGNATURES[s][1]) == nargs, s
    for name, value in (("NTM_MULTI_MAX_TENSORS", _lib.MULTI_MAX_TENSORS), ("NTM_MULTI_CHUNK", _lib.MULTI_CHUNK)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value
    # a chunk is a whole number of 16-byte rounds of a 256-thread workgroup, and the table fits the kernel arguments
    assert _lib.MULTI_CHUNK % 1024 == 0 and _lib.MULTI_MAX_TENSORS * (4 * 8 + 8 + 4) + 64 <= 4096
    with open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS = .*\bmulti_tensor\.hip\b", f.read(), re.M)


@pytest.mark.parametrize("kw", [{"lr": -1e-3}, {"eps": -1e-8}, {"betas": (-0.1, 0.9)}, {"betas": (1.0, 0.9)}, {"betas": (0.9, 1.0)},
                                {"betas": (0.9, -0.5)}, {"weight_decay": -1.0}])
def test_the_constructor_refuses_what_torch_adam_refuses_in_its_words(kw):
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError) as theirs:
        torch.optim.Adam(p, **kw)
    with pytest.raises(ValueError) as ours:
        optim.FusedAdam(p, **kw)
    assert str(ours.value) == str(theirs.value)


@pytest.mark.parametrize("kw", [{"weight_decay": 0.01}, {"amsgrad": True}, {"maximize": True}])
def test_the_constructor_says_what_is_built(kw):
    with pytest.raises(ValueError, match="built for Adam without weight decay: weight_decay == 0, amsgrad=False, maximize=False"):
        optim.FusedAdam([torch.nn.Parameter(torch.zeros(3))], **kw)


def test_defaults_and_param_groups_are_torch_adams():
    p, q = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    ours, theirs = optim.FusedAdam([p]), torch.optim.Adam([p])
    assert ours.defaults == theirs.defaults
    o = optim.FusedAdam([{"params": [p], "lr": 0.5}, {"params": [q], "betas": (0.5, 0.75), "eps": 1.0}], lr=0.25)
    assert [g["lr"] for g in o.param_groups] == [0.5, 0.25] and o.param_groups[1]["betas"] == (0.5, 0.75)
    assert o.param_groups[0]["eps"] == 1e-8 and o.param_groups[1]["eps"] == 1.0


def test_step_refuses_cpu_parameters_and_leaves_the_state_alone():
    p = torch.nn.Parameter(torch.ones(3))
    o = optim.FusedAdam([p])
    assert o.step() is None and o.step(max_grad_norm=1.0) is None          # nothing has a gradient: nothing to do
    p.grad = torch.ones(3)
    for kw in ({}, {"max_grad_norm": 1.0}):
        with pytest.raises(RuntimeError, match="not on a HIP device.*contiguous float32 tensors on a HIP device"):
            o.step(**kw)
    assert len(o.state) == 0 and torch.equal(p.detach(), torch.ones(3))
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        optim.ema_update_([torch.zeros(3)], [torch.ones(3)], 0.5)
    with pytest.raises(ValueError, match="2 destinations for 1 sources"):
        optim.ema_update_([torch.zeros(3), torch.zeros(3)], [torch.ones(3)], 0.5)
    # a group that a caller or a loaded state_dict turned into what is not built
    o.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="built for Adam without weight decay"):
        o.step()


def _stepped(cls, steps=2):
    g = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (4, 7)]
    o = cls([{"params": ps[:1], "lr": 0.01}, {"params": ps[1:], "lr": 0.02, "betas": (0.8, 0.9)}])
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        o.step()
    return ps, o, g


def test_state_dict_goes_to_torch_adam_and_back():
    # torch -> FusedAdam -> torch: nothing is lost on the way, and torch's Adam continues where the first one would have
    ps, theirs, g = _stepped(torch.optim.Adam)
    sd = copy.deepcopy(theirs.state_dict())       # (a state_dict shares its tensors with the optimiser)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ours = optim.FusedAdam([{"params": qs[:1]}, {"params": qs[1:]}])
    ours.load_state_dict(sd)
    assert [grp["lr"] for grp in ours.param_groups] == [0.01, 0.02] and ours.param_groups[1]["betas"] == (0.8, 0.9)
    back = ours.state_dict()
    assert back["param_groups"] == sd["param_groups"] and set(back["state"]) == set(sd["state"])
    for k, st in sd["state"].items():
        assert set(back["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        for name, v in st.items():
            assert torch.equal(back["state"][k][name], v) and back["state"][k][name].dtype == v.dtype, (k, name)
        assert back["state"][k]["step"].device.type == "cpu" and back["state"][k]["step"].dim() == 0
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    again = torch.optim.Adam([{"params": rs[:1]}, {"params": rs[1:]}])
    again.load_state_dict(copy.deepcopy(back))
    for p, r in zip(ps, rs):
        p.grad = torch.randn(p.shape, generator=g)
        r.grad = p.grad.clone()
    theirs.step()
    again.step()
    for p, r in zip(ps, rs):
        assert torch.equal(p, r)
    # a fresh FusedAdam's state_dict has torch's keys, and torch's Adam steps from it
    fresh = optim.FusedAdam([torch.nn.Parameter(torch.zeros(3))]).state_dict()
    assert fresh == torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))]).state_dict()


def test_the_c_entry_points_refuse_bad_arguments_without_a_device():
    L = _lib.lib()
    one = (ctypes.c_void_p * 2)(16, 32)
    two, three = (ctypes.c_void_p * 2)(48, 64), (ctypes.c_void_p * 2)(80, 96)
    hole = (ctypes.c_void_p * 2)(16, None)
    n, neg = _lib.i64_array([4, 4]), _lib.i64_array([4, -1])
    f = [0.0] * 6

    def refused(rc, name, text):
        msg = L.ntm_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and text in msg, (rc, msg)

    refused(L.ntm_multi_sqnorm(one, n, -1, one, None, None), "ntm_multi_sqnorm", "negative count")
    refused(L.ntm_multi_sqnorm(hole, n, 2, one, None, None), "ntm_multi_sqnorm", "null pointer")
    refused(L.ntm_multi_sqnorm(one, neg, 2, one, None, None), "ntm_multi_sqnorm", "negative size")
    refused(L.ntm_multi_sqnorm(None, n, 2, one, None, None), "ntm_multi_sqnorm", "null pointer")
    refused(L.ntm_multi_sqnorm(one, n, 2, None, None, None), "ntm_multi_sqnorm", "null pointer")
    refused(L.ntm_multi_clip_coef(None, 3, 1.0, one, None), "ntm_multi_clip_coef", "null pointer")
    refused(L.ntm_multi_clip_coef(one, 3, 1.0, None, None), "ntm_multi_clip_coef", "null pointer")
    refused(L.ntm_multi_clip_coef(one, -1, 1.0, one, None), "ntm_multi_clip_coef", "negative size")
    refused(L.ntm_multi_adam(one, one, two, three, n, -1, None, *f, None), "ntm_multi_adam", "negative count")
    refused(L.ntm_multi_adam(one, hole, two, three, n, 2, None, *f, None), "ntm_multi_adam", "null pointer")
    refused(L.ntm_multi_adam(one, one, two, three, neg, 2, None, *f, None), "ntm_multi_adam", "negative size")
    for p, m, v in ((one, one, two), (one, two, one), (one, two, two)):
        refused(L.ntm_multi_adam(p, three, m, v, n, 2, None, *f, None), "ntm_multi_adam", "must not alias")
    refused(L.ntm_multi_ema(one, two, n, -1, 0.5, 0.5, None), "ntm_multi_ema", "negative count")
    refused(L.ntm_multi_ema(one, hole, n, 2, 0.5, 0.5, None), "ntm_multi_ema", "null pointer")
    refused(L.ntm_multi_ema(one, two, neg, 2, 0.5, 0.5, None), "ntm_multi_ema", "negative size")
    # the size query, and what needs no device at all: nothing to do
    C = _lib.MULTI_CHUNK
    assert L.ntm_multi_partials(_lib.i64_array([0, 1, C, C + 1, 2 * C + 3]), 5) == 0 + 1 + 1 + 2 + 3
    assert L.ntm_multi_partials(neg, 2) == -1 and L.ntm_multi_partials(n, -1) == -1 and L.ntm_multi_partials(None, 0) == 0
    empty = _lib.i64_array([0, 0])
    got = ctypes.c_int64(-7)
    assert L.ntm_multi_sqnorm(hole, empty, 2, None, ctypes.byref(got), None) == 0 and got.value == 0
    assert L.ntm_multi_adam(hole, hole, hole, hole, empty, 2, None, *f, None) == 0
    assert L.ntm_multi_ema(hole, hole, empty, 2, 0.5, 0.5, None) == 0 and L.ntm_multi_ema(None, None, None, 0, 0.5, 0.5, None) == 0


@pytest.mark.parametrize("foreach", [False, True])
def test_exact_case_fractions_and_torch_adam_on_the_cpu_agree_to_the_bit(foreach):
    O.assert_exact(O.exact_run(lambda groups: torch.optim.Adam(groups, foreach=foreach)))
    dst, src, want = O.ema_exact_case()
    for d, q, w in zip(dst, src, want):
        assert torch.equal(d * 0.5 + q * (1 - 0.5), w)


def test_every_case_has_a_positive_bar_where_it_takes_one():
    """The bars come from the two CPU references alone; a case whose references agreed to the bit would hold nothing."""
    cases = [O.element_case(n, i) for i, n in enumerate(O.ELEMENT_COUNTS)] + [O.count_case(c, i) for i, c in enumerate(O.TENSOR_COUNTS)]
    cases += [O.mixed_case("active"), O.mixed_case("absent", True), O.ramp_case()]
    for case in cases:
        r32, r64 = O.references(case)
        for q in O.QUANTITIES:
            if (q == "norm" and case.max_norm is None) or (q == "grad" and case.clip != "active") or not r64[q].any():
                continue
            assert O.bar_of(r32[q], r64[q]) > 0, (case.sizes, case.clip, q)
