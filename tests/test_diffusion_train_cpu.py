"""CPU: the host side of the diffusion generators' training (ntm_amd.diffusion.EDMTrainer, UNet1D.forward_train,
training.ResBlockFn on csrc/unet_train.hip) against the reference's own training run (tests/golden/g30_*, written by
tools/make_goldens_diffusion_train.py from code/train-diffusion.py): the C entry points' declarations, the size queries, every
documented refusal (made before anything touches a device, so they run here with made-up non-null pointers), and the EDM loop
on the torch backend replayed in float64 (the same arithmetic in the same dtype: 1e-9) and in float32 (the bar of
diffusion_train_cases)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ntm_amd
from ntm_amd import diffusion
import diffusion_train_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"ntm_unet_resblock_save_floats": 2, "ntm_unet_resblock_wgrad_floats": 1, "ntm_unet_resblock_partial_floats": 2,
        "ntm_unet_resblock_forward_save": 13, "ntm_unet_resblock_backward": 18, "ntm_unet_wgrad_reduce": 5}
P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(16)]     # made-up device pointers: a refusal never looks at them


def spec(c0=8, c1=0, c_out=8, n=8, T=100, T0=None, off0=0, T1=0, off1=0, init=0, form=0):
    return diffusion.BlockSpec(c0, c1, c_out, n, T, T if T0 is None else T0, off0, T1, off1, init, form)


def test_new_symbols_are_declared_bound_and_built():
    L = ntm_amd._lib.lib()
    with open(os.path.join(ROOT, "include", "ntm.h")) as f:
        header = f.read()
    for s, nargs in SYMS.items():
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1] and len(ntm_amd._lib._SIGNATURES[s][1]) == nargs, s
    assert "unet_train.hip" in open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "Makefile")).read()
    assert ntm_amd.EDMTrainer is diffusion.EDMTrainer and "EDMTrainer" in ntm_amd.__all__
    assert hasattr(ntm_amd.training, "ResBlockFn") and hasattr(diffusion.UNet1D, "forward_train")


@pytest.mark.parametrize("kw", [dict(), dict(c0=16, c1=16, c_out=16, T=512, T1=512), dict(c0=8, c_out=16, T=17, init=1, n=1),
                                dict(c0=5, c1=3, c_out=12, T=1024, T1=1024, form=1), dict(T=1), dict(T=129, n=3)])
def test_size_queries_equal_their_formulas(kw):
    L, k = ntm_amd._lib.lib(), spec(**kw)
    cin, B = k.c0 + k.c1, 3
    per = k.n_layers * k.c_out * k.c_out * 5 + 2 * k.c_out * cin + (5 * k.c0 if k.init else 0)
    waves = min(8, -(-k.T // 16))
    assert L.ntm_unet_resblock_save_floats(B, ctypes.byref(k)) == B * k.n_layers * k.c_out * k.T
    assert L.ntm_unet_resblock_wgrad_floats(ctypes.byref(k)) == per
    assert L.ntm_unet_resblock_partial_floats(B, ctypes.byref(k)) == B * waves * per
    assert L.ntm_unet_resblock_partial_floats(0, ctypes.byref(k)) == 0


REFUSED = {"T = 1025": dict(T=1025), "the tiled form": dict(form=2), "c_out = 17": dict(c_out=17), "c_in = 33": dict(c0=17, c1=16, T1=100),
           "off0 past the source": dict(T=100, T0=120, off0=21), "no layers": dict(n=0), "nine layers": dict(n=9),
           "a negative crop": dict(off0=-1)}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_size_queries_and_entry_points_refuse_before_the_device(why):
    L, k = ntm_amd._lib.lib(), spec(**REFUSED[why])
    assert L.ntm_unet_resblock_save_floats(2, ctypes.byref(k)) == -1, why
    assert L.ntm_last_error().decode().startswith("ntm_unet_resblock_save_floats"), why
    assert L.ntm_unet_resblock_wgrad_floats(ctypes.byref(k)) == -1 and L.ntm_unet_resblock_partial_floats(2, ctypes.byref(k)) == -1
    rc = L.ntm_unet_resblock_forward_save(P[0], P[1], None, P[2], 0, P[3], P[4], P[5], 2, ctypes.byref(k), P[6], P[7], None)
    assert rc < 0 and L.ntm_last_error().decode().startswith("ntm_unet_resblock_forward_save"), why
    rc = L.ntm_unet_resblock_backward(P[0], P[1], None, P[2], 0, P[3], P[4], P[5], 2, ctypes.byref(k), P[6], P[7], P[8], P[9], P[10],
                                      P[11], P[12], None)
    assert rc < 0 and L.ntm_last_error().decode().startswith("ntm_unet_resblock_backward"), why


def test_inconsistent_and_null_arguments_are_refused_before_the_device():
    L = ntm_amd._lib.lib()
    fwd = lambda k, a: L.ntm_unet_resblock_forward_save(*a[:8], 2, ctypes.byref(k), a[8], a[9], None)       # noqa: E731
    bwd = lambda k, a: L.ntm_unet_resblock_backward(*a[:8], 2, ctypes.byref(k), *a[8:16], None)             # noqa: E731
    good_f = [P[0], None, None, P[2], 0, P[3], P[4], P[5], P[6], P[7]]
    good_b = [P[0], None, None, P[2], 0, P[3], P[4], P[5], P[6], P[7], P[8], P[9], None, P[10], P[11]]

    def refused(rc, who, word):
        msg = L.ntm_last_error().decode()
        assert rc < 0 and msg.startswith(who) and word in msg, (rc, msg)

    k = spec(c0=8, c_out=16)                     # W_res == NULL with c_in != c_out
    a = list(good_f)
    a[7] = None
    refused(fwd(k, a), "ntm_unet_resblock_forward_save", "identity residual")
    a = list(good_b)
    a[7] = None
    refused(bwd(k, a), "ntm_unet_resblock_backward", "identity residual")
    k = spec()
    for i in (0, 3, 5, 6, 8, 9):                 # src0, film, w_first, w_gated, ysave, out
        a = list(good_f)
        a[i] = None
        refused(fwd(k, a), "ntm_unet_resblock_forward_save", "null pointer")
    for i in (0, 3, 5, 6, 8, 9, 10, 13, 14):     # ... ysave, gout, ws, gfilm, partials
        a = list(good_b)
        a[i] = None
        refused(bwd(k, a), "ntm_unet_resblock_backward", "null pointer")
    a = list(good_f)
    a[4] = 7                                     # a FiLM stride below c_in
    refused(fwd(k, a), "ntm_unet_resblock_forward_save", "film_stride")
    a = list(good_b)
    a[12] = P[12]                                # a gradient for a second source that is not there
    refused(bwd(k, a), "ntm_unet_resblock_backward", "g_src1")
    a = list(good_b)
    a[2] = P[13]
    refused(bwd(spec(init=1), a), "ntm_unet_resblock_backward", "waveform")        # init: g_src0 must be NULL
    a = list(good_f)
    a[2] = None
    refused(fwd(spec(init=1), a), "ntm_unet_resblock_forward_save", "null pointer")  # init without init_w
    a = list(good_f)
    a[9] = a[0]
    refused(fwd(k, a), "ntm_unet_resblock_forward_save", "alias")
    assert L.ntm_unet_wgrad_reduce(P[0], -1, 4, P[1], None) < 0 and L.ntm_unet_wgrad_reduce(None, 2, 4, P[1], None) < 0
    assert L.ntm_unet_wgrad_reduce(P[0], 2, 4, None, None) < 0 and L.ntm_unet_wgrad_reduce(None, 0, 0, None, None) == 0
    # B == 0 is fine and touches nothing
    assert L.ntm_unet_resblock_forward_save(None, None, None, None, 0, None, None, None, 0, ctypes.byref(k), None,
                                                             None, None) == 0


@pytest.fixture(scope="module")
def replay64():
    return C.replay(C.trainer("cpu", torch.float64, "torch"), "cpu", torch.float64)


@pytest.fixture(scope="module")
def replay32():
    return C.replay(C.trainer("cpu", torch.float32, "torch"), "cpu", torch.float32)


def test_float64_replay_equals_the_reference_run(replay64):
    """The same arithmetic in the same dtype: what remains is the order of operations."""
    a, r, worst = C.arrays(), replay64, {}

    def close(what, got, ref):
        e = C.rel_err(np.asarray(got), np.asarray(ref, np.float64))
        kind = what.split()[0]
        worst[kind] = max(worst.get(kind, 0.0), e)
        assert e <= 1e-9, (what, e)

    close("loss", r["loss"], a["loss_ref64"])
    close("sigma", r["sigma0"], a["sigma_ref64"][0])
    close("grad_norm", r["grad_norm"], a["grad_norm_ref64"])
    assert r["lr"] == list(a["lr_ref64"]) == [0.0, 2e-4 * 1 / 1000, 2e-4 * 2 / 1000]
    assert sorted(r["grads"]) == sorted(C.trained_keys())
    for k in C.trained_keys():
        close(f"grad {k}", r["grads"][k], a["grad64_" + k])
    for k in C.param_keys():
        close(f"net {k}", r["net"][k], C.final("net", "64", k))
        close(f"ema {k}", r["ema"][k], C.final("ema", "64", k))
    print("float64 replay, worst relative error per kind:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_float32_replay_holds_the_bar(replay32):
    a, r, worst = C.arrays(), replay32, {}
    C.hold("loss", np.asarray(r["loss"]), a["loss_ref32"], a["loss_ref64"], worst)
    C.hold("grad_norm", np.asarray(r["grad_norm"]), a["grad_norm_ref32"], a["grad_norm_ref64"], worst)
    for k in C.trained_keys():
        C.hold(f"grad {k}", r["grads"][k], a["grad32_" + k], a["grad64_" + k], worst)
    for k in C.param_keys():
        C.hold(f"net {k}", r["net"][k], C.final("net", "32", k), C.final("net", "64", k), worst)
        C.hold(f"ema {k}", r["ema"][k], C.final("ema", "32", k), C.final("ema", "64", k), worst)
    print("float32 replay, worst ratio per kind:", {k: f"{v:.2f}" for k, v in worst.items()})


def test_forward_train_is_hip_only_and_names_forward_torch():
    net = C.network()
    with pytest.raises(RuntimeError, match=r"HIP device only.*forward_torch"):
        net.forward_train(torch.zeros(2, 64), torch.zeros(2, 1))
    tr = C.trainer(backend="hip")
    with pytest.raises(RuntimeError, match="HIP device only"):
        tr.train_step(*C.batch(0))
    with pytest.raises(ValueError, match="backend"):
        diffusion.EDMTrainer(C.config(), net, None, "cpu", backend="triton")


def test_trainer_checkpoint_loads_into_the_generator():
    tr = C.trainer()
    sd = tr.state_dict()
    assert list(sd) == ["it", "network", "optimizer", "ema", "args"] and sd["it"] == 0
    args = C.config()
    args.network.checkpoint = None
    gen = diffusion.DiffusionGenerator(args, "cpu")
    gen.network.load_state_dict(sd["ema"], strict=True)
    assert not any(p.requires_grad for p in tr.ema.parameters()) and not tr.ema.training


def test_g30_is_complete():
    a = C.arrays()
    keys, params = str(a["keys"]).split(";"), C.param_keys()
    net = diffusion.UNet1D(C.config(), "cpu")
    assert keys == list(net.state_dict()) and params == [k for k, _ in net.named_parameters()]
    assert a["x"].shape == (C.ITERS, C.B, C.T) == a["noise"].shape and a["a"].shape == (C.ITERS, C.B)
    assert a["x"].dtype == a["noise"].dtype == a["a"].dtype == np.float32
    for tag in ("ref32", "ref64"):
        for name, shape in (("loss", (3,)), ("grad_norm", (3,)), ("lr", (3,)), ("sigma", (3, C.B, 1)), ("net_out", (C.B, C.T))):
            assert a[f"{name}_{tag}"].shape == shape, (name, tag)
        assert a["net_out_" + tag].dtype == (np.float32 if tag == "ref32" else np.float64)
    sd = net.state_dict()
    for k in keys:
        assert a["init_" + k].shape == tuple(sd[k].shape) and a["init_" + k].dtype == np.float32, k
    assert C.trained_keys() == [k for k, p in net.named_parameters() if p.requires_grad]
    for k in params:
        shape = tuple(sd[k].shape)
        for name in ("net32d_", "net64d_", "ema32d_", "ema64d_"):
            assert a[name + k].shape == shape and a[name + k].dtype == np.float32, (name, k)
        if k in C.trained_keys():
            assert a["grad64_" + k].shape == shape and a["grad64_" + k].dtype == np.float64, k
            assert a["grad32_" + k].shape == shape and a["grad32_" + k].dtype == np.float32, k
            assert np.any(a["grad64_" + k]), f"{k}: a parameter without a gradient checks nothing"
    for f in C.FILES:
        assert os.path.getsize(os.path.join(C.GOLDEN, f)) < (1 << 20), f
