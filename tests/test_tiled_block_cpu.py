"""CPU: the host side of the tiled ResnetBlock's training entry points (ntm_unet_resblock_tiled_*, csrc/unet_train.hip under
training.ResBlockTiledFn): the declarations, the size queries against their formulas, and every documented refusal -- all made
before anything touches a device, so they run here with made-up non-null pointers."""
import ctypes
import os
import re

import pytest

import ntm_amd
from ntm_amd import diffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"ntm_unet_resblock_tiled_save_floats": 2, "ntm_unet_resblock_tiled_workspace_floats": 2,
        "ntm_unet_resblock_tiled_wgrad_floats": 1, "ntm_unet_resblock_tiled_partial_floats": 2,
        "ntm_unet_resblock_tiled_forward_save": 13, "ntm_unet_resblock_tiled_backward": 18}
QUERIES = [s for s in SYMS if s.endswith("_floats")]
P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(16)]     # made-up device pointers: a refusal never looks at them
TILED = diffusion.FORMS["tiled"]


def spec(c0=8, c1=0, c_out=8, n=8, T=100, T0=None, off0=0, T1=0, off1=0, init=0, form=TILED):
    return diffusion.BlockSpec(c0, c1, c_out, n, T, T if T0 is None else T0, off0, T1, off1, init, form)


def query(L, name, B, k):
    return getattr(L, name)(ctypes.byref(k)) if name.endswith("wgrad_floats") else getattr(L, name)(B, ctypes.byref(k))


def test_new_symbols_are_declared_and_bound():
    L = ntm_amd._lib.lib()
    with open(os.path.join(ROOT, "include", "ntm.h")) as f:
        header = f.read()
    for s, nargs in SYMS.items():
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1] and len(ntm_amd._lib._SIGNATURES[s][1]) == nargs, s
    # the operand lists of the whole-form namesakes
    for s in ("forward_save", "backward"):
        assert ntm_amd._lib._SIGNATURES["ntm_unet_resblock_tiled_" + s] == ntm_amd._lib._SIGNATURES["ntm_unet_resblock_" + s], s
    assert hasattr(ntm_amd.training, "ResBlockTiledFn") and ntm_amd.training.ResBlockTiledFn is not ntm_amd.training.ResBlockFn
    assert diffusion._TrainWalk.tiled_blocks is True


@pytest.mark.parametrize("kw", [dict(), dict(T=1), dict(T=512), dict(T=513, n=7), dict(c0=16, c1=16, c_out=16, T=1537, T0=1544, off0=3, T1=1537),
                                dict(c0=8, c_out=16, T=1300, T0=1302, off0=2, init=1, n=1), dict(c0=5, c1=3, c_out=12, T=65536, T1=65536, form=0),
                                dict(T=1025, form=0)])
def test_size_queries_equal_their_formulas(kw):
    L, k = ntm_amd._lib.lib(), spec(**kw)
    cin, B = k.c0 + k.c1, 3
    per = k.n_layers * k.c_out * k.c_out * 5 + 2 * k.c_out * cin + (5 * k.c0 if k.init else 0)
    tiles = -(-k.T // diffusion.TILE)
    runs = 2 if k.n_layers == 8 else 1              # layers 0-6 reach 254 frames of the 256 of halo; layer 7 takes them all
    r = ctypes.byref(k)
    assert L.ntm_unet_resblock_tiled_save_floats(B, r) == B * k.n_layers * k.c_out * k.T
    assert L.ntm_unet_resblock_tiled_wgrad_floats(r) == per
    assert L.ntm_unet_resblock_tiled_workspace_floats(B, r) == runs * B * k.c_out * k.T + B * tiles * cin
    # per stream: its sum, one partial per tile, one per tile and wave
    assert L.ntm_unet_resblock_tiled_partial_floats(B, r) == B * (1 + tiles * (1 + 8)) * per
    assert L.ntm_unet_resblock_tiled_partial_floats(0, r) == 0 and L.ntm_unet_resblock_tiled_workspace_floats(0, r) == 0


REFUSED = {"the whole form": dict(form=1), "auto at T = 1024": dict(T=1024, form=0), "auto at T = 1": dict(T=1, form=0),
           "an unknown form": dict(form=3), "c_out = 17": dict(c_out=17), "c_out = 0": dict(c_out=0),
           "c_in = 33": dict(c0=17, c1=16, T1=100), "off0 past the source": dict(T=2000, T0=2020, off0=21),
           "src1 too short": dict(c1=4, T=2000, T1=1999), "no layers": dict(n=0), "nine layers": dict(n=9),
           "a negative crop": dict(off0=-1), "no frames": dict(T=0)}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_size_queries_and_entry_points_refuse_before_the_device(why):
    L, k = ntm_amd._lib.lib(), spec(**REFUSED[why])
    for q in QUERIES:
        assert query(L, q, 2, k) == -1, (why, q)
        assert L.ntm_last_error().decode().startswith(q), (why, q)
    rc = L.ntm_unet_resblock_tiled_forward_save(P[0], P[1], None, P[2], 0, P[3], P[4], P[5], 2, ctypes.byref(k), P[6], P[7], None)
    assert rc < 0 and L.ntm_last_error().decode().startswith("ntm_unet_resblock_tiled_forward_save"), why
    rc = L.ntm_unet_resblock_tiled_backward(P[0], P[1], None, P[2], 0, P[3], P[4], P[5], 2, ctypes.byref(k), P[6], P[7], P[8], P[9],
                                            P[10], P[11], P[12], None)
    assert rc < 0 and L.ntm_last_error().decode().startswith("ntm_unet_resblock_tiled_backward"), why


def test_the_whole_form_family_still_refuses_the_tiled_form():
    L = ntm_amd._lib.lib()
    for k in (spec(T=100), spec(T=1025, form=0)):
        assert L.ntm_unet_resblock_save_floats(2, ctypes.byref(k)) == -1
        assert L.ntm_unet_resblock_tiled_save_floats(2, ctypes.byref(k)) == 2 * 8 * 8 * k.T


def test_inconsistent_and_null_arguments_are_refused_before_the_device():
    L = ntm_amd._lib.lib()
    fwd = lambda k, a: L.ntm_unet_resblock_tiled_forward_save(*a[:8], 2, ctypes.byref(k), a[8], a[9], None)       # noqa: E731
    bwd = lambda k, a: L.ntm_unet_resblock_tiled_backward(*a[:8], 2, ctypes.byref(k), *a[8:16], None)             # noqa: E731
    good_f = [P[0], None, None, P[2], 0, P[3], P[4], P[5], P[6], P[7]]
    good_b = [P[0], None, None, P[2], 0, P[3], P[4], P[5], P[6], P[7], P[8], P[9], None, P[10], P[11]]

    def refused(rc, who, word):
        msg = L.ntm_last_error().decode()
        assert rc < 0 and msg.startswith(who) and word in msg, (rc, msg)

    k = spec(c0=8, c_out=16, T=1500)             # W_res == NULL with c_in != c_out
    a = list(good_f)
    a[7] = None
    refused(fwd(k, a), "ntm_unet_resblock_tiled_forward_save", "identity residual")
    a = list(good_b)
    a[7] = None
    refused(bwd(k, a), "ntm_unet_resblock_tiled_backward", "identity residual")
    k = spec(T=1500)
    for i in (0, 3, 5, 6, 8, 9):                 # src0, film, w_first, w_gated, ysave, out
        a = list(good_f)
        a[i] = None
        refused(fwd(k, a), "ntm_unet_resblock_tiled_forward_save", "null pointer")
    for i in (0, 3, 5, 6, 8, 9, 10, 13, 14):     # ... ysave, gout, ws, gfilm, partials
        a = list(good_b)
        a[i] = None
        refused(bwd(k, a), "ntm_unet_resblock_tiled_backward", "null pointer")
    a = list(good_f)
    a[4] = 7                                     # a FiLM stride below c_in
    refused(fwd(k, a), "ntm_unet_resblock_tiled_forward_save", "film_stride")
    a = list(good_b)
    a[4] = 7
    refused(bwd(k, a), "ntm_unet_resblock_tiled_backward", "film_stride")
    a = list(good_b)
    a[12] = P[12]                                # a gradient for a second source that is not there
    refused(bwd(k, a), "ntm_unet_resblock_tiled_backward", "g_src1")
    a = list(good_b)
    a[2] = P[13]
    refused(bwd(spec(init=1, T=1500), a), "ntm_unet_resblock_tiled_backward", "waveform")        # init: g_src0 must be NULL
    a = list(good_f)
    a[2] = None
    refused(fwd(spec(init=1, T=1500), a), "ntm_unet_resblock_tiled_forward_save", "null pointer")  # init without init_w
    a = list(good_f)
    a[9] = a[0]
    refused(fwd(k, a), "ntm_unet_resblock_tiled_forward_save", "alias")
    k2 = spec(c0=8, c1=8, c_out=16, T=1500, T1=1500)
    a = list(good_b)
    a[1] = None                                  # a second source without its pointer
    refused(bwd(k2, a), "ntm_unet_resblock_tiled_backward", "null pointer")
    # B == 0 is fine and touches nothing; so is leaving out both source gradients
    none = [None] * 8
    assert L.ntm_unet_resblock_tiled_forward_save(*none[:3], None, 0, *none[:3], 0, ctypes.byref(k), None, None, None) == 0
    assert L.ntm_unet_resblock_tiled_backward(*none[:3], None, 0, *none[:3], 0, ctypes.byref(k), *none[:7], None) == 0
