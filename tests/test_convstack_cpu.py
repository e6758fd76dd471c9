"""CPU: the host side of the dilated conv stack (ntm_convstack_*, csrc/convstack_kernels.hip) and of
ntm_amd.critics.DilatedConvDisc -- symbols, the size functions against the closed forms of include/ntm.h, the argument checks
(made before anything touches a device, so they run here with made-up non-null pointers), and what the constructor builds
against the reference's own numbers (tests/golden/g26_dilated_disc.npz, written by tools/make_goldens_dilated_disc.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

import ntm_amd
from ntm_amd import critics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ntm_convstack_saved_floats", "ntm_convstack_workspace_floats", "ntm_convstack_forward", "ntm_convstack_backward")
X, SAVED, OUT, GOUT, GX, WS = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))
DEFAULT = ((1, 64, 5, 1, 1),) + tuple((64, 64, 5, 1, 2 ** i) for i in range(1, 11)) + ((64, 1, 5, 1, 1),)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g26_dilated_disc.npz"))


def test_entry_points_are_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    L = ntm_amd._lib.lib()
    for s in SYMS:
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1]
    assert len(ntm_amd._lib._SIGNATURES["ntm_convstack_forward"][1]) == 13
    assert len(ntm_amd._lib._SIGNATURES["ntm_convstack_backward"][1]) == 17
    assert "ntm_conv1d_layer_d" in header and ctypes.sizeof(ntm_amd._lib.ConvLayerD) == 20
    assert ctypes.sizeof(ntm_amd._lib.ConvLayer) == 16
    assert re.search(r"#define\s+NTM_ABI_VERSION\s+9\b", header) and L.ntm_abi_version() == 9
    assert issubclass(ntm_amd.training.ConvStackFn, torch.autograd.Function) and "ConvStackFn" in ntm_amd.training.__doc__
    assert "DilatedConvDisc" in critics.__doc__ and "DilatedConvDisc" in critics.SUPPORTED and "MultiSpecCrit" in critics.SUPPORTED


def counts(B, F0, spec):
    """(saved, workspace) floats as include/ntm.h documents them."""
    W = [co * (ci // g) * k for ci, co, k, g, _ in spec]
    R = [co for _, co, _, _, _ in spec]
    F, frames = F0, []
    for _, _, k, _, d in spec:
        F -= (k - 1) * d
        frames.append(F)
    acts = [B * co * f for (_, co, _, _, _), f in zip(spec[:-1], frames[:-1])]
    n0 = max(min(B, 32), 1)
    per = max(-(-B // n0), 1)
    chunks = -(-B // per)                                       # none for an empty batch
    ws = 2 * max(acts + [0]) + sum(chunks * -(-f // 1024) * (w + r) for w, r, f in zip(W, R, frames))
    return 2 * sum(W) + sum(R) + sum(acts), ws


SIZE_CASES = [
    (16, 16384, DEFAULT),                                                                       # the operating point: 12 layers
    (3, 4497 + 37, ((1, 64, 5, 1, 1), (64, 64, 5, 1, 33), (64, 64, 5, 1, 1089), (64, 1, 5, 1, 1))),
    (70, 2000, ((3, 24, 3, 1, 7), (24, 40, 4, 8, 130), (40, 5, 2, 1, 3))),                       # 32 chunks of 3 streams, 24 used
    (1, 500, tuple((4, 4, 2, 1, 65 if l % 2 else 1) for l in range(13))),                       # more than 8 layers
    (2, 2048 + 5, ((2, 6, 2, 2, 4),)),                                                          # 2049 output frames: three segments
    (0, 100, ((1, 8, 5, 1, 1), (8, 1, 5, 1, 2))),
]


@pytest.mark.parametrize("B,F0,spec", SIZE_CASES)
def test_the_size_functions_return_the_documented_counts(B, F0, spec):
    L = ntm_amd._lib.lib()
    lay = ntm_amd._lib.conv_layers_d(spec)
    want = counts(B, F0, spec)
    assert L.ntm_convstack_saved_floats(B, spec[0][0], F0, len(spec), lay) == want[0], L.ntm_last_error()
    assert L.ntm_convstack_workspace_floats(B, spec[0][0], F0, len(spec), lay) == want[1]


P3 = ((3, 16, 5, 1, 2), (16, 64, 3, 4, 5), (64, 1, 2, 1, 1))            # spans 8, 10, 1: receptive field 20
REFUSED = [
    (dict(n=0), "n_layers"), (dict(n=17, spec=((4, 4, 1, 1, 1),) * 17), "n_layers"), (dict(spec=None), "null pointer"),
    (dict(C0=0), "size"), (dict(F0=0), "size"), (dict(B=-1), "size"),
    (dict(C0=1025, spec=((1025, 16, 5, 1, 1),)), "1024"), (dict(spec=((3, 1025, 5, 1, 1),)), "1024"), (dict(spec=((3, 0, 5, 1, 1),)), "1024"),
    (dict(spec=((3, 16, 0, 1, 1),)), "k must"), (dict(spec=((3, 16, 65, 1, 1),), F0=100), "k must"),
    (dict(spec=((3, 16, 5, 1, 0),)), "dilation"), (dict(spec=((3, 16, 5, 1, -1),)), "dilation"),
    (dict(spec=((3, 16, 2, 1, 2 ** 20 + 1),), F0=2 ** 21), "dilation"),
    (dict(spec=((3, 16, 5, 2, 1),)), "groups"), (dict(spec=((4, 15, 5, 2, 1),), C0=4), "groups"), (dict(spec=((3, 16, 5, 0, 1),)), "groups"),
    (dict(C0=4), "c_in"), (dict(spec=((3, 16, 5, 1, 2), (8, 64, 3, 4, 5))), "c_in"),
    (dict(F0=8), "frames"), (dict(F0=18), "frames"), (dict(F0=19), "frames"),                  # too short at layer 1, 2, 3
    (dict(spec=((3, 16, 5, 1, 10),)), "frames"),                                                # the dilation alone: span 41 > 40
    (dict(B=2 ** 31 // (3 * 40) + 1), "2^31"), (dict(B=2 ** 31 // (64 * 22) + 1), "2^31"),
]


def _n(n, spec):
    return (len(spec) if spec else 3) if n is None else n


def _sizes(fn, B=2, C0=3, F0=40, n=None, spec=P3):
    lay = None if spec is None else ntm_amd._lib.conv_layers_d(spec)
    return fn(B, C0, F0, _n(n, spec), lay)


def _arrays(spec, null=False):
    n = len(spec) if spec else 1
    return None if null else (ctypes.c_void_p * n)(*([0x70000] * n))


def _forward(B=2, C0=3, F0=40, n=None, spec=P3, x=X, saved=SAVED, out=OUT, g=False, v=False, bias=False, slope=0.2):
    lay = None if spec is None else ntm_amd._lib.conv_layers_d(spec)
    return ntm_amd._lib.lib().ntm_convstack_forward(x, B, C0, F0, slope, _n(n, spec), lay, _arrays(spec, g), _arrays(spec, v),
                                                   _arrays(spec, bias), saved, out, None)


def _backward(B=2, C0=3, F0=40, n=None, spec=P3, x=X, saved=SAVED, gout=GOUT, gx=GX, ws=WS, g=False, v=False, dg=False, dv=False,
              db=False, slope=0.2):
    lay = None if spec is None else ntm_amd._lib.conv_layers_d(spec)
    return ntm_amd._lib.lib().ntm_convstack_backward(x, B, C0, F0, slope, _n(n, spec), lay, _arrays(spec, g), _arrays(spec, v), saved,
                                                    gout, gx, _arrays(spec, dg), _arrays(spec, dv), _arrays(spec, db), ws, None)


def test_the_size_functions_refuse_with_minus_one():
    L = ntm_amd._lib.lib()
    for name in SYMS[:2]:
        for kw, word in REFUSED:
            assert _sizes(getattr(L, name), **kw) == -1, (name, kw)
            msg = L.ntm_last_error().decode()
            assert msg.startswith(name + ": ") and word in msg, (name, kw, msg)
    # sizes that fit exactly are taken: the receptive field as F0 (one output frame), 16 layers, 1024 channels, k = 64, the
    # largest dilation; B == 0 counts the weights alone
    assert _sizes(L.ntm_convstack_saved_floats, F0=20) > 0
    assert _sizes(L.ntm_convstack_saved_floats, spec=((3, 16, 5, 1, 10),), F0=41) > 0
    assert _sizes(L.ntm_convstack_saved_floats, spec=((3, 3, 1, 1, 1),) * 16) > 0
    assert _sizes(L.ntm_convstack_saved_floats, C0=1024, spec=((1024, 1024, 64, 1024, 1),), F0=64, B=1) > 0
    assert _sizes(L.ntm_convstack_saved_floats, spec=((3, 16, 2, 1, 2 ** 20),), F0=2 ** 20 + 1) > 0
    assert _sizes(L.ntm_convstack_saved_floats, B=0) == 2 * (16 * 3 * 5 + 64 * 4 * 3 + 64 * 2) + 16 + 64 + 1
    assert _sizes(L.ntm_convstack_workspace_floats, B=0) == 0


@pytest.mark.parametrize("call,name,pointers", [
    (_forward, "ntm_convstack_forward", [dict(x=None), dict(saved=None), dict(out=None), dict(g=True), dict(v=True), dict(bias=True)]),
    (_backward, "ntm_convstack_backward", [dict(x=None), dict(saved=None), dict(gout=None), dict(ws=None), dict(g=True), dict(v=True),
                                           dict(dv=True), dict(db=True), dict(gx=X), dict(gx=GOUT)]),
])
def test_one_refusal_per_check_under_the_called_name(call, name, pointers):
    L = ntm_amd._lib.lib()
    slopes = [dict(slope=0.0), dict(slope=1.0), dict(slope=float("nan")), dict(slope=-0.2), dict(slope=1.5)]
    for kw in [kw for kw, _ in REFUSED] + pointers + slopes:
        assert call(**kw) == -1, kw
        assert L.ntm_last_error().decode().startswith(name + ": "), (kw, L.ntm_last_error())
    assert call(x=None) == -1 and "null pointer" in L.ntm_last_error().decode()
    assert call(slope=float("nan")) == -1 and "slope" in L.ntm_last_error().decode()


def test_an_empty_batch_is_ok_with_null_pointers():
    assert _forward(B=0, x=None, saved=None, out=None, g=True, v=True, bias=True) == 0
    assert _backward(B=0, x=None, saved=None, gout=None, gx=None, ws=None, g=True, v=True, dg=True, dv=True, db=True) == 0


# ---- critics.DilatedConvDisc --------------------------------------------------------------------------------------------
def test_construction_builds_the_reference_s_layers_and_touches_no_device(golden, capsys, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the constructor touched a device")
    monkeypatch.setattr(torch.cuda, "_lazy_init", no_device)
    monkeypatch.setattr(ntm_amd._lib, "lib", no_device)
    torch.manual_seed(0)
    m = critics.DilatedConvDisc(test_in_len=8263)
    assert capsys.readouterr().out == str(golden["line"]) == 'Dilated Conv Disc, output size = 10,1,71 \n'
    sd = m.state_dict()
    assert ";".join(sd) == str(golden["keys"])
    assert ";".join(",".join(str(n) for n in v.shape) for v in sd.values()) == str(golden["shapes"])
    assert list(sd) == [f"layers.{2 * i}.{name}" for i in range(12) for name in ("bias", "weight_g", "weight_v")]
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in sd.values())
    for name in ("bias", "weight_g", "weight_v"):
        assert torch.equal(sd[f"layers.0.{name}"], torch.from_numpy(golden["first_" + name])), name
        assert torch.equal(sd[f"layers.22.{name}"], torch.from_numpy(golden["last_" + name])), name
    assert len(m.layers) == 23
    for j in range(1, 23, 2):
        assert type(m.layers[j]) is nn.LeakyReLU and m.layers[j].negative_slope == 0.2 and not m.layers[j].inplace
    convs = [m.layers[j] for j in range(0, 23, 2)]
    assert all(isinstance(c, nn.Conv1d) and c.kernel_size == (5,) and c.stride == (1,) and c.padding == (0,) for c in convs)
    assert [c.dilation[0] for c in convs] == [2 ** i for i in range(11)] + [1]
    assert [(c.in_channels, c.out_channels) for c in convs] == [(1, 64)] + [(64, 64)] * 10 + [(64, 1)]
    assert m.spec() == DEFAULT and m.receptive_field() == 8193
    critics.DilatedConvDisc(test_in_len=16384)
    assert capsys.readouterr().out == 'Dilated Conv Disc, output size = 10,1,8192 \n'


def test_a_seeded_construction_gives_the_reference_s_weights(golden, capsys):
    torch.manual_seed(0)
    m = critics.DilatedConvDisc(layers=4, conv_channels=8, test_in_len=100)
    after = torch.rand(3)
    sd = m.state_dict()
    want = {k[3:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("sd_")}
    assert list(sd) == list(want) and len(want) == 12
    assert all(torch.equal(sd[k], v) for k, v in want.items())
    assert torch.equal(after, torch.from_numpy(golden["after"]))      # ... and the generator stands where the reference leaves it
    assert m.spec() == ((1, 8, 5, 1, 1), (8, 8, 5, 1, 2), (8, 8, 5, 1, 4), (8, 1, 5, 1, 1))
    assert capsys.readouterr().out == 'Dilated Conv Disc, output size = 10,1,68 \n'
    # a reference checkpoint loads
    other = critics.DilatedConvDisc(layers=4, conv_channels=8, test_in_len=100)
    other.load_state_dict(want)
    assert all(torch.equal(v, want[k]) for k, v in other.state_dict().items())


def test_the_reference_s_quirks_are_kept(capsys):
    one = critics.DilatedConvDisc(blocks=1, conv_channels=4, test_in_len=5)                    # no block: the final layer alone
    assert one.spec() == ((4, 1, 5, 1, 1),)
    two = critics.DilatedConvDisc(blocks=3, layers=3, kernel_size=3, conv_channels=4, dil_fac=3, in_channels=2, out_channels=2, test_in_len=40)
    assert two.spec() == ((2, 4, 3, 1, 1), (4, 4, 3, 1, 3), (4, 4, 3, 1, 1), (4, 4, 3, 1, 3), (4, 2, 3, 1, 1))
    assert capsys.readouterr().out.splitlines()[-1] == 'Dilated Conv Disc, output size = 10,2,22 '
    m = critics.DilatedConvDisc(layers=3, conv_channels=4, nl_params={"negative_slope": 0.05}, test_in_len=50)
    assert m.slope == 0.05 and m.layers[1].negative_slope == 0.05


def test_what_is_not_built_is_refused(capsys):
    with pytest.raises(RuntimeError, match="test_in_len=1 .*receptive field of 8193"):
        critics.DilatedConvDisc()
    with pytest.raises(RuntimeError, match="test_in_len=8192 .*receptive field of 8193"):
        critics.DilatedConvDisc(test_in_len=8192)
    with pytest.raises(RuntimeError, match="Tanh"):
        critics.DilatedConvDisc(nl_func="Tanh", nl_params={}, test_in_len=16384)
    for slope in (0.0, 1.0, -0.1):
        with pytest.raises(RuntimeError, match="negative_slope"):
            critics.DilatedConvDisc(nl_params={"negative_slope": slope}, test_in_len=16384)
    m = critics.DilatedConvDisc(layers=4, conv_channels=8, test_in_len=100)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(2, 1, 100))
    with pytest.raises(RuntimeError, match="HIP device"):
        ntm_amd.training.ConvStackFn.apply(torch.zeros(2, 1, 100), 0.2, m.spec(), *[p for c in m.convs() for p in (c.weight_g, c.weight_v, c.bias)])
    capsys.readouterr()
    with pytest.raises(RuntimeError, match="HIP device.*MultiSpecCrit"):
        critics.get_critic("DilatedConvDisc", {}, "cpu", 0, 16384)
    assert capsys.readouterr().out == ""                                                        # refused before anything is built
    with pytest.raises(RuntimeError, match="'MelGanCrit' is not built.*MultiSpecCrit"):
        critics.get_critic("MelGanCrit", {}, "cpu", 0, 16384)
    with pytest.raises(RuntimeError, match="'MelGanCrit' is not built"):
        critics.get_critic("MelGanCrit", {}, "cuda", 0, 16384)


def test_convstack_kernels_run_dpp_with_full_exec():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_exec.py"),
                        os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "convstack_kernels.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
