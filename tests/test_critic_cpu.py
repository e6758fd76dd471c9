"""CPU: the host side of the spectral critics' conv stack (ntm_speccrit_*, csrc/critic_kernels.hip) and of ntm_amd.critics --
symbols, the size functions, the argument checks (made before anything touches a device, so they run here with made-up non-null
pointers), what the modules build in their constructors, and the seeded construction against the reference's order of draws."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
from torch import nn
from torch.nn.utils import weight_norm

import ntm_amd
from ntm_amd import critics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ntm_speccrit_saved_floats", "ntm_speccrit_workspace_floats", "ntm_speccrit_forward", "ntm_speccrit_backward")
X, SAVED, OUT, GOUT, GX, WS = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))

# configs/AdversarialConfig.py, critic 1, 2 and 5
COMMON = dict(layers=4, chan_in=16, chan_fac=4, stride=1, g_fac=16, log=True)
CONFIGS = {
    1: dict(scales=[128, 256, 512, 1024], kernel_sizes=[21, 21, 21, 17], hop_sizes=[32, 64, 128, 128], tf_rep="spec", **COMMON),
    2: dict(scales=[128, 256, 512, 1024], kernel_sizes=[21, 21, 21, 17], hop_sizes=[32, 64, 128, 128], tf_rep="mel", **COMMON),
    5: dict(scales=[512, 1024, 2048], kernel_sizes=[21, 17, 7], hop_sizes=[64, 64, 64], tf_rep="spec", **COMMON),
}


def plan(C0, ks):
    """The reference's channel plan behind C0 bins."""
    return ((C0, 16, 10, 1), (16, 64, ks, 4), (64, 256, ks, 16), (256, 256, 5, 1), (256, 1, 3, 1))


def test_entry_points_are_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    L = ntm_amd._lib.lib()
    for s in SYMS:
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1]
    assert len(ntm_amd._lib._SIGNATURES["ntm_speccrit_forward"][1]) == 13
    assert len(ntm_amd._lib._SIGNATURES["ntm_speccrit_backward"][1]) == 17
    assert "ntm_conv1d_layer" in header and ctypes.sizeof(ntm_amd._lib.ConvLayer) == 16
    assert re.search(r"#define\s+NTM_ABI_VERSION\s+9\b", header) and L.ntm_abi_version() == 9
    assert issubclass(ntm_amd.training.SpecCritFn, torch.autograd.Function) and "SpecCritFn" in ntm_amd.training.__doc__
    assert "critics" in ntm_amd.__all__


def counts(B, F0, spec):
    """(saved, workspace) floats as include/ntm.h documents them."""
    W = sum(co * (ci // g) * k for ci, co, k, g in spec)
    R = sum(co for _, co, _, _ in spec)
    F, acts = F0, []
    for _, co, k, _ in spec[:-1]:
        F -= k - 1
        acts.append(B * co * F)
    n0 = min(B, 32)
    per = -(-B // n0)
    chunks = -(-B // per)
    return 2 * W + R + sum(acts), 2 * max(acts + [0]) + chunks * (W + R)


@pytest.mark.parametrize("B,F0,spec", [(16, 513, plan(65, 21)), (3, 40, ((33, 8, 10, 1), (8, 16, 7, 2), (16, 1, 3, 1))),
                                       (70, 65, plan(513, 17)), (1, 12, ((5, 7, 3, 1),))])
def test_the_size_functions_return_the_documented_counts(B, F0, spec):
    L = ntm_amd._lib.lib()
    lay = ntm_amd._lib.conv_layers(spec)
    want = counts(B, F0, spec)
    assert L.ntm_speccrit_saved_floats(B, spec[0][0], F0, len(spec), lay) == want[0]
    assert L.ntm_speccrit_workspace_floats(B, spec[0][0], F0, len(spec), lay) == want[1]


P3 = ((33, 16, 10, 1), (16, 64, 7, 4), (64, 1, 3, 1))
REFUSED = [
    (dict(n=0), "n_layers"), (dict(n=9, spec=((4, 4, 1, 1),) * 9), "n_layers"), (dict(spec=None), "null pointer"),
    (dict(C0=0), "size"), (dict(C0=1026, spec=((1026, 16, 10, 1),)), "1025"), (dict(C0=1025, spec=((1025, 16, 10, 1), (16, 1025, 3, 1))), "1024"), (dict(spec=((33, 1025, 10, 1),)), "1024"),
    (dict(spec=((33, 0, 10, 1),)), "1024"), (dict(spec=((33, 16, 0, 1),)), "k must"), (dict(spec=((33, 16, 65, 1),), F0=100), "k must"),
    (dict(spec=((33, 16, 10, 2),)), "groups"), (dict(spec=((32, 15, 10, 2),), C0=32), "groups"), (dict(spec=((33, 16, 10, 0),)), "groups"),
    (dict(C0=34), "c_in"), (dict(spec=((33, 16, 10, 1), (8, 64, 7, 4))), "c_in"),
    (dict(F0=9), "frames"), (dict(F0=15), "frames"), (dict(F0=17), "frames"),
    (dict(B=-1), "size"), (dict(B=2 ** 31 // (33 * 40) + 1), "2^31"), (dict(B=2 ** 31 // (64 * 25) + 1), "2^31"),
]


def _sizes(fn, B=2, C0=33, F0=40, n=None, spec=P3):
    lay = None if spec is None else ntm_amd._lib.conv_layers(spec)
    return fn(B, C0, F0, (len(spec) if spec else 3) if n is None else n, lay)


def _arrays(spec, null=False):
    n = len(spec) if spec else 1
    return None if null else (ctypes.c_void_p * n)(*([0x70000] * n))


def _forward(B=2, C0=33, F0=40, n=None, spec=P3, x=X, saved=SAVED, out=OUT, g=False, v=False, bias=False, floor=1e-5):
    lay = None if spec is None else ntm_amd._lib.conv_layers(spec)
    return ntm_amd._lib.lib().ntm_speccrit_forward(x, B, C0, F0, floor, (len(spec) if spec else 3) if n is None else n, lay, _arrays(spec, g),
                                                  _arrays(spec, v), _arrays(spec, bias), saved, out, None)


def _backward(B=2, C0=33, F0=40, n=None, spec=P3, x=X, saved=SAVED, gout=GOUT, gx=GX, ws=WS, g=False, v=False, dg=False, dv=False,
              db=False, floor=1e-5):
    lay = None if spec is None else ntm_amd._lib.conv_layers(spec)
    return ntm_amd._lib.lib().ntm_speccrit_backward(x, B, C0, F0, floor, (len(spec) if spec else 3) if n is None else n, lay, _arrays(spec, g),
                                                   _arrays(spec, v), saved, gout, gx, _arrays(spec, dg), _arrays(spec, dv),
                                                   _arrays(spec, db), ws, None)


def test_the_size_functions_refuse_with_minus_one():
    L = ntm_amd._lib.lib()
    for name in SYMS[:2]:
        for kw, word in REFUSED:
            assert _sizes(getattr(L, name), **kw) == -1, (name, kw)
            msg = L.ntm_last_error().decode()
            assert msg.startswith(name + ": ") and word in msg, (name, kw, msg)
    # a k that fits exactly is taken, and so are the 1025 bins of n_fft 2048 (critic 5); B == 0 counts the weights alone
    assert _sizes(L.ntm_speccrit_saved_floats, C0=1025, spec=((1025, 16, 10, 1),)) > 0
    assert _sizes(L.ntm_speccrit_saved_floats, F0=18) > 0
    assert _sizes(L.ntm_speccrit_saved_floats, B=0) == 2 * (33 * 16 * 10 + 64 * 4 * 7 + 64 * 3) + 16 + 64 + 1


@pytest.mark.parametrize("call,name,pointers", [
    (_forward, "ntm_speccrit_forward", [dict(x=None), dict(saved=None), dict(out=None), dict(g=True), dict(v=True), dict(bias=True)]),
    (_backward, "ntm_speccrit_backward", [dict(x=None), dict(saved=None), dict(gout=None), dict(ws=None), dict(g=True), dict(v=True),
                                          dict(dv=True), dict(db=True), dict(gx=X)]),
])
def test_one_refusal_per_check_under_the_called_name(call, name, pointers):
    L = ntm_amd._lib.lib()
    for kw in [kw for kw, _ in REFUSED] + pointers + [dict(floor=-1.0), dict(floor=float("nan"))]:
        assert call(**kw) == -1, kw
        assert L.ntm_last_error().decode().startswith(name + ": "), (kw, L.ntm_last_error())
    assert call(x=None) == -1 and "null pointer" in L.ntm_last_error().decode()


def test_an_empty_batch_is_ok_with_null_pointers():
    assert _forward(B=0, x=None, saved=None, out=None, g=True, v=True, bias=True) == 0
    assert _backward(B=0, x=None, saved=None, gout=None, gx=None, ws=None, g=True, v=True, dg=True, dv=True, db=True) == 0


def conv_keys(cfg):
    """state_dict keys and shapes of the conv layers the reference builds for a MultiSpecCrit configuration."""
    want = {}
    for i, (scale, ks) in enumerate(zip(cfg["scales"], cfg["kernel_sizes"])):
        C0 = scale // 2 + 1 if cfg["tf_rep"] == "spec" else 160
        for j, (ci, co, k, g) in zip((1, 3, 5, 7, 9), plan(C0, ks)):
            want[f"models.{i}.layers.{j}.bias"] = (co,)
            want[f"models.{i}.layers.{j}.weight_g"] = (co, 1, 1)
            want[f"models.{i}.layers.{j}.weight_v"] = (co, ci // g, k)
    return want


@pytest.mark.parametrize("c", [1, 2, 5])
def test_construction_builds_the_reference_s_layers_and_touches_no_device(c, capsys, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the constructor touched a device")
    monkeypatch.setattr(torch.cuda, "_lazy_init", no_device)
    monkeypatch.setattr(ntm_amd._lib, "lib", no_device)
    m = critics.MultiSpecCrit(**CONFIGS[c], test_in_len=16384)
    sd = m.state_dict()
    convs = {k: tuple(v.shape) for k, v in sd.items() if ".layers.0." not in k}
    assert convs == conv_keys(CONFIGS[c])
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in sd.values())
    assert {k.split(".")[-1] for k in sd if ".layers.0." in k} == {"window", "mel_basis"}
    for i, model in enumerate(m.models):
        assert isinstance(model.layers[0], ntm_amd.TimeFreqConverter) and len(model.layers) == 10
        assert all(isinstance(model.layers[j], nn.LeakyReLU) and model.layers[j].negative_slope == 0.2 and model.layers[j].inplace
                   for j in (2, 4, 6, 8))
        assert (model.scale, model.log, model.log_eps, model.tf_rep) == (CONFIGS[c]["scales"][i], True, 1e-5, CONFIGS[c]["tf_rep"])
    assert m.scales == CONFIGS[c]["scales"]
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == len(CONFIGS[c]["scales"])
    if c == 1:
        assert lines == ['Spect Disc = {}, kernel size = {}, layers = 4, output size = 10,1,{} '.format(s, k, f)
                         for s, k, f in ((128, 21, 458), (256, 21, 202), (512, 21, 74), (1024, 17, 18))]


@pytest.mark.parametrize("seed", [0, 7])
def test_a_seeded_construction_gives_the_reference_s_weights(seed):
    cfg = CONFIGS[1]
    torch.manual_seed(seed)
    m = critics.MultiSpecCrit(**cfg, test_in_len=16384)
    after = torch.rand(3)
    torch.manual_seed(seed)
    twin = {}
    for i, (scale, ks) in enumerate(zip(cfg["scales"], cfg["kernel_sizes"])):
        for j, (ci, co, k, g) in zip((1, 3, 5, 7, 9), plan(scale // 2 + 1, ks)):
            conv = weight_norm(nn.Conv1d(ci, co, k, groups=g))
            for name in ("bias", "weight_g", "weight_v"):
                twin[f"models.{i}.layers.{j}.{name}"] = getattr(conv, name).detach()
        torch.randn((10, 1, 16384))
    sd = m.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in twin.items()) and len(twin) == 60
    assert torch.equal(after, torch.rand(3))                     # ... and the generator stands where the reference leaves it


def test_what_is_not_built_is_refused():
    with pytest.raises(RuntimeError, match="stride=2.*supported.*stride=1"):
        critics.MultiSpecCrit(**dict(CONFIGS[1], stride=2), test_in_len=16384)
    m = critics.MultiSpecCrit(**dict(CONFIGS[1], scales=[128], kernel_sizes=[21], hop_sizes=[32]), test_in_len=4096)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(2, 1, 4096))
    with pytest.raises(RuntimeError, match="HIP device"):
        m.models[0](torch.zeros(1, 1, 4096))
    for name in ("MelGanCrit", "DilatedConvDisc"):
        with pytest.raises(RuntimeError, match="MultiSpecCrit"):
            critics.get_critic(name, {}, "cpu", 0, 16384)


def test_get_critic_makes_the_reference_s_adam_even_at_a_zero_learning_rate():
    pars = dict(CONFIGS[5], scales=[512], kernel_sizes=[21], hop_sizes=[64])
    crit, opt = critics.get_critic("MultiSpecCrit", pars, "cpu", 0, 16384)
    assert isinstance(crit, critics.MultiSpecCrit) and pars["test_in_len"] == 16384
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["lr"] == 0 and opt.defaults["betas"] == (0.5, 0.9)
    assert sum(len(g["params"]) for g in opt.param_groups) == 15


def test_critic_kernels_run_dpp_with_full_exec():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_exec.py"),
                        os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "critic_kernels.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
