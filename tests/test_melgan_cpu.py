"""CPU: the host side of the strided conv stack (ntm_sconvstack_*, csrc/sconv_kernels.hip) and of ntm_amd.critics.MelGCrit /
NLayerDiscriminator -- symbols, the frame rule and the size functions against the closed forms of include/ntm.h, the argument
checks (made before anything touches a device, so they run here with made-up non-null pointers), what the constructor builds
against the reference's own numbers (tests/golden/g27_melgan_crit.npz, written by tools/make_goldens_melgan.py), and the
condition under which tests/test_gpu_melgan.py asserts its tight bar."""
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
from melgan_cases import (CANCELLATION_CASE, CONDITION_MAX, R, STACKS, Z, MelTwin, conditioning, chunk_rule, frames, make_case, raw_cases, raw_table, sides_agree, sizes, twin)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ntm_sconvstack_saved_floats", "ntm_sconvstack_workspace_floats", "ntm_sconvstack_forward", "ntm_sconvstack_backward")
X, SAVED, GX, WS = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x50000, 0x60000))
CONFIG0 = STACKS["e"][0]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g27_melgan_crit.npz"))


def test_entry_points_are_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    L = ntm_amd._lib.lib()
    for s in SYMS:
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1]
    assert len(ntm_amd._lib._SIGNATURES["ntm_sconvstack_forward"][1]) == 13
    assert len(ntm_amd._lib._SIGNATURES["ntm_sconvstack_backward"][1]) == 18
    assert "ntm_conv1d_layer_s" in header and ctypes.sizeof(ntm_amd._lib.ConvLayerS) == 28
    assert [f for f, _ in ntm_amd._lib.ConvLayerS._fields_] == ["c_in", "c_out", "k", "groups", "stride", "pad", "pad_mode"]
    assert re.search(r"#define\s+NTM_ABI_VERSION\s+9\b", header) and L.ntm_abi_version() == 9
    assert issubclass(ntm_amd.training.StridedConvStackFn, torch.autograd.Function) and "StridedConvStackFn" in ntm_amd.training.__doc__
    assert "MelGCrit" in critics.__doc__ and "MelGanCrit" in critics.SUPPORTED and critics.SUPPORTED.startswith("MultiSpecCrit")
    assert "sconv_kernels.hip" in open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "Makefile")).read()


# ---- the frame rule and the size functions -------------------------------------------------------------------------------
def test_the_frame_rule():
    assert frames(300, CONFIG0) == [300, 300, 75, 19, 5, 2, 2, 2]
    assert frames(16384, CONFIG0) == [16384, 16384, 4096, 1024, 256, 64, 64, 64]
    assert frames(2101, STACKS["a"][0])[:4] == [2101, 2101, 526, 132]
    assert [frames(T, STACKS["c"][0]) for T in (4, 24, 1205)] == [[4, 1, 1, 4], [24, 7, 3, 5], [1205, 401, 134, 70]]
    assert frames(8, STACKS["a"][0]) == [8, 8, 2, 1, 1, 1] and frames(8, STACKS["b"][0]) == [8, 8, 4, 2, 2, 2]
    d = critics.NLayerDiscriminator(16, 4, 4)
    assert d.output_frames(300) == [300, 75, 19, 5, 2, 2, 2] and ntm_amd.training._sconvstack_frames(300, d.spec()) == frames(300, CONFIG0)


def one_layer_partials(B, layer, F_in):
    """chunks x segments of one layer's weight gradient, read off ntm_sconvstack_workspace_floats of the one-layer stack:
    ws = 2 B c_out F_out + (reflected: B c_in (F_in + 2 pad)) + chunks segments (W + c_out)."""
    L = ntm_amd._lib.lib()
    ci, co, k, g, s, pad, mode = layer
    Fo = frames(F_in, (layer,))[1]
    ws = L.ntm_sconvstack_workspace_floats(B, ci, F_in, 1, ntm_amd._lib.conv_layers_s((layer,)))
    assert ws >= 0, L.ntm_last_error()
    rest = ws - 2 * B * co * Fo - (B * ci * (F_in + 2 * pad) if mode == R and pad else 0)
    W = co * (ci // g) * k
    assert rest % (W + co) == 0
    return rest // (W + co)


def test_the_chunk_rule_at_the_operating_point():
    """B = 16, T = 16 384, configuration 0, every layer as a one-layer stack through the C size function: the dense layer (64
    output frames per stream, 5.2 M weights) is ONE partial summed over 1024 frames, not 16 partials of 64 frames and 335 MB."""
    Fr = frames(16384, CONFIG0)
    want = [(1024, 16, 2, 8), (1024, 4, 2, 8), (1024, 1, 2, 8), (1024, 1, 8, 2), (1024, 1, 16, 1), (1024, 1, 16, 1), (1024, 1, 16, 1)]
    for l, (layer, rule) in enumerate(zip(CONFIG0, want)):
        ci, co, k, g, *_ = layer
        assert chunk_rule(16, Fr[l + 1], co * (ci // g) * k) == rule, l
        assert one_layer_partials(16, layer, Fr[l]) == rule[1] * rule[3], l
    # the partials are bounded: a dense 1024 x 1024 x 64 layer over 2^15 frames and 32 streams stays at one 2^26-float partial
    assert chunk_rule(32, 2 ** 15, 2 ** 26) == (2 ** 15, 1, 32, 1)
    assert one_layer_partials(32, (1024, 1024, 64, 1, 1, 0, Z), 2 ** 15 + 63) == 1
    assert chunk_rule(40, 3000, 1000) == (1024, 3, 2, 20) and one_layer_partials(40, (10, 10, 10, 1, 1, 0, Z), 3009) == 60
    assert chunk_rule(3, 50, 10 ** 6) == (1024, 1, 3, 1) and one_layer_partials(3, (100, 1000, 10, 1, 1, 0, Z), 59) == 1
    assert chunk_rule(40, 5000, 2 ** 22) == (2048, 3, 40, 1) and one_layer_partials(40, (64, 1024, 64, 1, 1, 0, Z), 5063) == 3
    assert chunk_rule(0, 50, 10)[3] == 0 and one_layer_partials(0, (1, 10, 1, 1, 1, 0, Z), 50) == 0
    # 32 stream chunks at the most, two segments: 70 streams in chunks of 3
    assert chunk_rule(70, 2000, 240) == (1024, 2, 3, 24) and one_layer_partials(70, (3, 16, 5, 1, 1, 0, Z), 2004) == 48


SIZE_STACKS = [("a", 2101), ("b", 39), ("c", 1205), ("e", 300), ("e", 16384), ("a", 8), ("c", 4)]


@pytest.mark.parametrize("name,T", SIZE_STACKS)
@pytest.mark.parametrize("B", [0, 1, 3, 16, 40])
def test_the_size_functions_return_the_documented_counts(name, T, B):
    L = ntm_amd._lib.lib()
    spec = STACKS[name][0]
    lay = ntm_amd._lib.conv_layers_s(spec)
    want = sizes(B, spec[0][0], T, spec)
    assert L.ntm_sconvstack_saved_floats(B, spec[0][0], T, len(spec), lay) == want[0], L.ntm_last_error()
    assert L.ntm_sconvstack_workspace_floats(B, spec[0][0], T, len(spec), lay) == want[1]
    if B == 0:
        assert want[1] == 0


def test_the_saved_buffer_holds_no_activations():
    spec = CONFIG0
    W = sum(co * (ci // g) * k for ci, co, k, g, *_ in spec)
    assert W == 16924086 // 3 - 2 * sum(s[1] for s in spec)          # weight_v of one discriminator
    L, lay = ntm_amd._lib.lib(), ntm_amd._lib.conv_layers_s(spec)
    assert (L.ntm_sconvstack_saved_floats(16, 1, 16384, len(spec), lay) == L.ntm_sconvstack_saved_floats(0, 1, 8, len(spec), lay)
            == sizes(16, 1, 16384, spec)[0] == 2 * W + sum(s[1] for s in spec))


# ---- refusals -----------------------------------------------------------------------------------------------------------
P3 = ((3, 16, 5, 1, 2, 2, R), (16, 64, 3, 4, 1, 1, Z), (64, 1, 2, 1, 3, 0, Z))       # frames 40 -> 20 -> 20 -> 7
REFUSED = [
    (dict(n=0), "n_layers"), (dict(n=17, spec=((4, 4, 1, 1, 1, 0, Z),) * 17, C0=4), "n_layers"), (dict(spec=None), "null pointer"),
    (dict(C0=0), "size"), (dict(F0=0), "size"), (dict(B=-1), "size"),
    (dict(C0=1025, spec=((1025, 16, 5, 1, 1, 0, Z),)), "1024"), (dict(spec=((3, 1025, 5, 1, 1, 0, Z),)), "1024"),
    (dict(spec=((3, 0, 5, 1, 1, 0, Z),)), "1024"),
    (dict(spec=((3, 16, 0, 1, 1, 0, Z),)), "k must"), (dict(spec=((3, 16, 65, 1, 1, 0, Z),), F0=100), "k must"),
    (dict(spec=((3, 16, 5, 1, 0, 0, Z),)), "stride"), (dict(spec=((3, 16, 5, 1, 65, 0, Z),)), "stride"), (dict(spec=((3, 16, 5, 1, -1, 0, Z),)), "stride"),
    (dict(spec=((3, 16, 5, 1, 1, 5, Z),)), "pad must"), (dict(spec=((3, 16, 5, 1, 1, -1, Z),)), "pad must"), (dict(spec=((3, 16, 1, 1, 1, 1, Z),)), "pad must"),
    (dict(spec=((3, 16, 5, 1, 1, 2, 2),)), "pad_mode"), (dict(spec=((3, 16, 5, 1, 1, 2, -1),)), "pad_mode"),
    (dict(spec=((3, 16, 5, 1, 1, 2, Z), (16, 16, 5, 1, 1, 2, R))), "first layer"),
    (dict(spec=((3, 16, 15, 1, 1, 7, R),), F0=7), "reflected"), (dict(spec=((3, 16, 5, 1, 1, 4, R),), F0=4), "reflected"),
    (dict(spec=((3, 16, 5, 2, 1, 0, Z),)), "groups"), (dict(spec=((4, 15, 5, 2, 1, 0, Z),), C0=4), "groups"), (dict(spec=((3, 16, 5, 0, 1, 0, Z),)), "groups"),
    (dict(C0=4), "c_in"), (dict(spec=((3, 16, 5, 1, 2, 2, R), (8, 64, 3, 4, 1, 1, Z))), "c_in"),
    (dict(spec=((3, 16, 5, 1, 1, 0, Z),), F0=4), "no output frame"), (dict(spec=((3, 16, 7, 1, 2, 1, Z),), F0=4), "no output frame"),
    (dict(spec=((3, 16, 5, 1, 4, 2, Z), (16, 4, 4, 1, 1, 0, Z)), F0=9), "no output frame"),       # 9 -> 3 frames, k = 4
    (dict(B=2 ** 31 // (3 * 44) + 1), "2^31"), (dict(B=2 ** 31 // (64 * 20) + 1), "2^31"),         # the padded input, a middle tensor
    (dict(B=2 ** 24, C0=1, F0=64, spec=((1, 1, 1, 1, 1, 0, Z),)), "2^24"),                          # 2^30 elements, 2^24 workgroups forward
    (dict(B=2 ** 18, C0=1, F0=64, spec=((1, 1, 64, 1, 64, 0, Z),)), "2^24"),                       # ... in the data gradient's 64 phases
]


def _n(n, spec):
    return (len(spec) if spec else 3) if n is None else n


def _sizes(fn, B=2, C0=3, F0=40, n=None, spec=P3):
    lay = None if spec is None else ntm_amd._lib.conv_layers_s(spec)
    return fn(B, C0, F0, _n(n, spec), lay)


def _arrays(spec, null=False, entries=None):
    n = len(spec) if spec else 1
    if null:
        return None
    return (ctypes.c_void_p * n)(*(entries if entries is not None else [0x70000] * n))


def _forward(B=2, C0=3, F0=40, n=None, spec=P3, x=X, saved=SAVED, outs=False, g=False, v=False, bias=False, slope=0.2, out_entries=None):
    lay = None if spec is None else ntm_amd._lib.conv_layers_s(spec)
    return ntm_amd._lib.lib().ntm_sconvstack_forward(x, B, C0, F0, slope, _n(n, spec), lay, _arrays(spec, g), _arrays(spec, v),
                                                    _arrays(spec, bias), saved, _arrays(spec, outs, out_entries), None)


def _backward(B=2, C0=3, F0=40, n=None, spec=P3, x=X, saved=SAVED, outs=False, gouts=False, gx=GX, ws=WS, g=False, v=False, dg=False,
              dv=False, db=False, slope=0.2, gout_entries=None):
    lay = None if spec is None else ntm_amd._lib.conv_layers_s(spec)
    return ntm_amd._lib.lib().ntm_sconvstack_backward(x, B, C0, F0, slope, _n(n, spec), lay, _arrays(spec, g), _arrays(spec, v), saved,
                                                     _arrays(spec, outs), _arrays(spec, gouts, gout_entries), gx, _arrays(spec, dg),
                                                     _arrays(spec, dv), _arrays(spec, db), ws, None)


def test_the_size_functions_refuse_with_minus_one():
    L = ntm_amd._lib.lib()
    for name in SYMS[:2]:
        for kw, word in REFUSED:
            assert _sizes(getattr(L, name), **kw) == -1, (name, kw)
            msg = L.ntm_last_error().decode()
            assert msg.startswith(name + ": ") and word in msg, (name, kw, msg)
    # sizes that fit exactly are taken: the minimum under the reflect pad, pad = k - 1, 16 layers, 1024 channels, k = stride = 64,
    # one output frame; B == 0 counts the weights alone
    assert _sizes(L.ntm_sconvstack_saved_floats, spec=((3, 16, 15, 1, 1, 7, R),), F0=8) > 0
    assert _sizes(L.ntm_sconvstack_saved_floats, spec=((3, 16, 5, 1, 1, 4, Z),), F0=1) > 0
    assert _sizes(L.ntm_sconvstack_saved_floats, spec=((3, 3, 1, 1, 1, 0, Z),) * 16) > 0
    assert _sizes(L.ntm_sconvstack_saved_floats, C0=1024, spec=((1024, 1024, 64, 1024, 64, 0, Z),), F0=64, B=1) > 0
    assert _sizes(L.ntm_sconvstack_saved_floats, B=0) == 2 * (16 * 3 * 5 + 64 * 4 * 3 + 64 * 2) + 16 + 64 + 1
    assert _sizes(L.ntm_sconvstack_workspace_floats, B=0) == 0
    assert frames(40, P3) == [40, 20, 20, 7]


@pytest.mark.parametrize("call,name,pointers", [
    (_forward, "ntm_sconvstack_forward", [dict(x=None), dict(saved=None), dict(outs=True), dict(g=True), dict(v=True), dict(bias=True),
                                          dict(out_entries=[0x70000, None, 0x70000])]),
    (_backward, "ntm_sconvstack_backward", [dict(x=None), dict(saved=None), dict(outs=True), dict(gouts=True), dict(ws=None), dict(g=True),
                                            dict(v=True), dict(dv=True), dict(db=True), dict(gx=X), dict(gx=ctypes.c_void_p(0x70000)),
                                            dict(gout_entries=[None, None, None])]),
])
def test_one_refusal_per_check_under_the_called_name(call, name, pointers):
    L = ntm_amd._lib.lib()
    slopes = [dict(slope=0.0), dict(slope=1.0), dict(slope=float("nan")), dict(slope=-0.2), dict(slope=1.5)]
    for kw in [kw for kw, _ in REFUSED] + pointers + slopes:
        assert call(**kw) == -1, kw
        assert L.ntm_last_error().decode().startswith(name + ": "), (kw, L.ntm_last_error())
    assert call(x=None) == -1 and "null pointer" in L.ntm_last_error().decode()
    assert call(slope=float("nan")) == -1 and "slope" in L.ntm_last_error().decode()
    if call is _backward:
        assert call(gout_entries=[None, None, None]) == -1 and "gouts" in L.ntm_last_error().decode()


def test_an_empty_batch_is_ok_with_null_pointers():
    assert _forward(B=0, x=None, saved=None, outs=True, g=True, v=True, bias=True) == 0
    assert _backward(B=0, x=None, saved=None, outs=True, gouts=True, gx=None, ws=None, g=True, v=True, dg=True, dv=True, db=True) == 0


# ---- critics.MelGCrit ---------------------------------------------------------------------------------------------------
def test_a_seeded_construction_gives_the_reference_s_weights_and_draws(golden, capsys, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the constructor touched a device")
    monkeypatch.setattr(torch.cuda, "_lazy_init", no_device)
    monkeypatch.setattr(ntm_amd._lib, "lib", no_device)
    torch.manual_seed(0)
    m = critics.MelGCrit(num_D=2, ndf=8, n_layers=2, downsampling_factor=1)
    after = torch.rand(3)
    assert capsys.readouterr().out == str(golden["printed"]) == ""              # the constructor prints nothing
    sd = m.state_dict()
    want = {k[3:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("sd_")}
    assert ";".join(sd) == str(golden["skeys"]) and set(sd) == set(want) and len(want) == 30
    assert all(torch.equal(sd[k], want[k]) for k in sd)
    assert torch.equal(after, torch.from_numpy(golden["after"]))      # weights_init drew: the generator stands where the reference leaves it
    assert sum(p.numel() for p in m.parameters()) == 3188
    # without weights_init the parameters are the same and the generator is not
    torch.manual_seed(0)
    plain = nn.ModuleDict({f"disc_{i}": critics.NLayerDiscriminator(8, 2, 1) for i in range(2)})
    assert all(torch.equal(v, sd["model." + k]) for k, v in plain.state_dict().items()) and not torch.equal(torch.rand(3), after)
    # a reference checkpoint loads
    other = critics.MelGCrit(num_D=2, ndf=8, n_layers=2, downsampling_factor=1)
    other.load_state_dict(want)
    assert all(torch.equal(v, want[k]) for k, v in other.state_dict().items())
    assert m.model["disc_1"].spec() == ((1, 8, 15, 1, 1, 7, R), (8, 8, 11, 2, 1, 5, Z), (8, 8, 11, 2, 1, 5, Z), (8, 16, 5, 1, 1, 2, Z),
                                        (16, 1, 3, 1, 1, 1, Z))


def test_configuration_0_is_the_reference_s(golden):
    torch.manual_seed(0)
    m = critics.MelGCrit(num_D=3, ndf=16, n_layers=4, downsampling_factor=4)
    after = torch.rand(3)
    sd = m.state_dict()
    assert ";".join(sd) == str(golden["keys"])
    assert ";".join(",".join(str(n) for n in v.shape) for v in sd.values()) == str(golden["shapes"])
    assert list(sd) == [f"model.disc_{i}.model.layer_{n}.{'' if n == 6 else '1.' if n == 0 else '0.'}{name}"
                        for i in range(3) for n in range(7) for name in ("bias", "weight_g", "weight_v")]
    assert sum(p.numel() for p in m.parameters()) == int(golden["n_params"]) == 16924086
    stored = [k for k in golden.files if k.startswith("c0_model.")]
    assert len(stored) == 12 and all(torch.equal(sd[k[3:]], torch.from_numpy(golden[k])) for k in stored)
    assert torch.equal(after, torch.from_numpy(golden["c0_after"]))
    assert all(d.spec() == CONFIG0 for d in m.model.values()) and m.num_D == 3 and m.n_layers == 4
    assert type(m.model) is nn.ModuleDict and type(m.model["disc_0"].model) is nn.ModuleDict
    l0, l6 = m.model["disc_0"].model["layer_0"], m.model["disc_0"].model["layer_6"]
    assert type(l0[0]) is nn.ReflectionPad1d and l0[0].padding == (7, 7) and type(l0[2]) is nn.LeakyReLU and l0[2].inplace
    assert l0[2].negative_slope == 0.2 and isinstance(l6, nn.Conv1d)


def test_the_reference_s_quirks_are_kept(capsys):
    for pars in ((4, 16, 2), (3, 16, 2), (2, 4, 1)):                     # (downsampling_factor, ndf, n_layers): construct, cannot run
        m = critics.MelGCrit(num_D=2, ndf=pars[1], n_layers=pars[2], downsampling_factor=pars[0])
        spec = m.model["disc_0"].spec()
        bad = next(l for l in range(1, len(spec)) if spec[l][0] != spec[l - 1][1])
        with pytest.raises(RuntimeError, match=rf"layer_{bad} expects {spec[bad][0]} input channels and is handed {spec[bad - 1][1]}\b"):
            m(torch.zeros(2, 1, 64))
    for pars in ((2, 512, 2), (1, 8, 2), (4, 16, 4)):                    # these run in the reference: the chain holds
        d = critics.NLayerDiscriminator(pars[1], pars[2], pars[0])
        d.check_chain()
    m = critics.MelGCrit(num_D=1, ndf=8, n_layers=2, downsampling_factor=1)
    assert type(m.downsample) is nn.AvgPool1d and list(m.downsample.parameters()) == [] and "downsample" in dict(m.named_modules())
    assert (m.downsample.kernel_size, m.downsample.stride, m.downsample.padding, m.downsample.count_include_pad) in (
        ((4,), (2,), (1,), False), (4, 2, 1, False))
    assert capsys.readouterr().out == ""


def test_get_critic_and_what_is_refused(capsys):
    with pytest.raises(RuntimeError, match="'MelGanCrit' is not built from critic_pars without num_D, ndf, n_layers, downsampling_factor.*MultiSpecCrit"):
        critics.get_critic("MelGanCrit", {}, "cpu", 0, 16384)
    with pytest.raises(RuntimeError, match="without n_layers;"):
        critics.get_critic("MelGanCrit", dict(num_D=3, ndf=16, downsampling_factor=4), "cuda", 0, 16384)
    pars = dict(num_D=3, ndf=16, n_layers=4, downsampling_factor=4)
    before = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="MelGanCrit on device 'cpu': HIP device only"):
        critics.get_critic("MelGanCrit", pars, "cpu", 0, 16384)
    assert torch.equal(before, torch.get_rng_state()) and pars == dict(num_D=3, ndf=16, n_layers=4, downsampling_factor=4)   # nothing was built
    with pytest.raises(RuntimeError, match="'NoSuchCrit' is not built \\(MelGanCrit"):
        critics.get_critic("NoSuchCrit", {}, "cpu", 0, 16384)
    m = critics.MelGCrit(num_D=1, ndf=8, n_layers=2, downsampling_factor=1)
    for x in (torch.zeros(2, 1, 40), torch.zeros(1, 40)):
        with pytest.raises(RuntimeError, match="HIP device"):
            m(x)
    d = m.model["disc_0"]
    with pytest.raises(RuntimeError, match="HIP device"):
        ntm_amd.training.StridedConvStackFn.apply(torch.zeros(2, 1, 40), 0.2, d.spec(), *[p for c in d.convs() for p in (c.weight_g, c.weight_v, c.bias)])
    assert capsys.readouterr().out == ""


# ---- the condition of the tight bar ----------------------------------------------------------------------------------------
def test_the_references_agree_on_every_leaky_relu_side_where_the_tight_bar_is_asserted(golden):
    """tests/test_gpu_melgan.py asserts its tight bar on every case of the stacks a to c, on the LeakyReLU-at-0 and layer-1-only
    cases and on the small module (golden g27 as ref32, the feature-matching inputs): in all of them the float32 and the float64
    twin sit on the same side of every LeakyReLU, so ref32 - ref64 is rounding and no flipped slope."""
    rows, _, _ = raw_table()
    small = [c for c in raw_cases() if c[0] != "e"]
    assert len(small) == 28 and len(raw_cases()) == 31
    for case in small:
        assert sides_agree(rows[case][1], rows[case][2]), case
        # ... and no output tensor is small by cancellation against the terms of its sums (the bar scales with max|ref64|)
        assert max(conditioning(rows[case][0][0], rows[case][0][1], *STACKS[case[0]])) <= CONDITION_MAX, case
    name, B, T, seed = CANCELLATION_CASE            # the seed left out of the table is the ill-conditioned one, and is run apart
    x, params, _ = make_case(seed, B, T, STACKS[name][0])
    assert max(conditioning(x, params, *STACKS[name])) > 4 * CONDITION_MAX
    spec, slope = STACKS["a"]
    x, params, gouts = make_case(6, 3, 60, spec)
    params[1][0][5] = 0.0
    params[1][2][5] = 0.0
    assert sides_agree(*(twin(x, params, spec, slope, gouts, dt) for dt in (torch.float64, torch.float32)))
    assert max(conditioning(x, params, spec, slope)[:1] + conditioning(x, params, spec, slope)[2:]) <= CONDITION_MAX
    x, params, gouts = make_case(8, 3, 39, spec)
    assert sides_agree(*(twin(x, params, spec, slope, gouts, dt) for dt in (torch.float64, torch.float32)))
    assert max(conditioning(x, params, spec, slope)) <= CONDITION_MAX
    m = critics.MelGCrit(num_D=2, ndf=8, n_layers=2, downsampling_factor=1)
    m.load_state_dict({k[3:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("sd_")})
    rng = np.random.default_rng(28)
    inputs = [torch.from_numpy(golden["x"])] + [torch.from_numpy(rng.uniform(-1.0, 1.0, (3, 1, 40)).astype(np.float32)) for _ in range(2)]
    for xin in inputs:
        with torch.no_grad():
            o64, o32 = (MelTwin(m, dt)(xin) for dt in (torch.float64, torch.float32))
        for s64, s32 in zip(o64, o32):
            assert all(torch.equal(a > 0, b > 0) for a, b in zip(s64[:-1], s32[:-1]))
    # ... and the twin in float32 gives the reference's own outputs to rounding
    with torch.no_grad():
        o32 = MelTwin(m, torch.float32)(inputs[0])
    for d in range(2):
        for l in range(5):
            assert np.allclose(o32[d][l].numpy(), golden[f"out_{d}_{l}"], rtol=0, atol=2e-6), (d, l)


def test_sconv_kernels_run_dpp_with_full_exec():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_exec.py"),
                        os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "sconv_kernels.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
