"""CPU: the host side of the diffusion generators (ntm_amd.diffusion, csrc/unet_kernels.hip) against the reference's own numbers
(tests/golden/g29_*, written by tools/make_goldens_diffusion.py from the reference's UNet1D / DiffusionGenerator and its three
shipped checkpoints): the configurations, the state_dict layout, torchaudio's filters, the schedules, the torch path of the
network in float64 (exact restatement: 1e-10) and float32 (the bar of diffusion_cases), the samplers with regenerated draws, the two
checkpoint formats, the C entry points' declarations and every documented refusal (made before anything touches a device, so
they run here with made-up non-null pointers)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import ntm_amd
from ntm_amd import diffusion
from diffusion_cases import (EV_BLOCKS, GOLDEN, NAMES, NOISE_DEPTH, NOISE_SMALL, arrays, check, config, draws, generator, normal,
                             outpaint_inputs, rel_err, seeds, weights_path)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"ntm_unet_resblock_workspace_floats": 2, "ntm_unet_resblock_forward": 13, "ntm_unet_down_combine": 13,
        "ntm_unet_up_combine": 14, "ntm_unet_upsample": 9, "ntm_edm_pre": 15, "ntm_edm_post": 9}
P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(12)]     # made-up device pointers: a refusal never looks at them


@pytest.fixture(scope="module")
def gens():
    return {"trajectories": generator("trajectories"), "toytrajectories": generator("toytrajectories"),
            "noise": generator("noise", **NOISE_SMALL)}


def test_exports_and_configs_equal_the_reference_yaml():
    assert {"UNet1D", "DiffusionGenerator", "load_config"} <= set(ntm_amd.__all__)
    assert ntm_amd.UNet1D is diffusion.UNet1D and ntm_amd.load_config is diffusion.load_config
    with open(os.path.join(GOLDEN, "g29_diffusion_configs.json")) as f:
        want = json.load(f)
    for n in NAMES:
        got = diffusion.load_config(n)
        assert json.loads(json.dumps(got)) == want[n], n
        assert got.network.depth == want[n]["network"]["depth"] and got.diff_params.T == want[n]["diff_params"]["T"]
        got.network.depth = 99                                   # a fresh copy every call
        assert diffusion.load_config(n).network.depth == want[n]["network"]["depth"]
    with pytest.raises(ValueError, match="neither"):
        diffusion.load_config("nope")


def test_yaml_path_reads_exponents_as_floats(tmp_path):
    p = tmp_path / "c.yaml"
    p.write_text("diff_params:\n  sigma_data: 8e-4\n  T: 16\nnetwork:\n  Ns: [8, 16]\n  name: \"unet_1d\"\n")
    c = diffusion.load_config(str(p))
    assert c.diff_params.sigma_data == 8e-4 and c.diff_params.T == 16 and c.network.Ns == [8, 16] and c.network.name == "unet_1d"


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_and_shapes_are_the_references(name):
    a = arrays()
    net = diffusion.UNet1D(config(name), "cpu")
    sd = net.state_dict()
    assert ";".join(sd) == str(a[f"keys_{name}"])
    assert ";".join(",".join(str(d) for d in v.shape) for v in sd.values()) == str(a[f"shapes_{name}"])
    assert len(sd) == {"noise": 176}.get(name, 122) and any(k == "downs.0.1.resample.kernel" for k in sd)
    with np.load(weights_path(name)) as z:
        ck = {k: torch.from_numpy(z[k]) for k in z.files}
    # the recomputed filters against torchaudio's own, carried by the checkpoint: within 1 ulp of float32
    for k, v in ck.items():
        if k.endswith("resample.kernel"):
            mine = sd[k].numpy().astype(np.float64)
            ulp = np.spacing(np.maximum(np.abs(v.numpy()), np.abs(sd[k].numpy())))
            assert np.max(np.abs(mine - v.numpy().astype(np.float64)) / ulp) <= 1.0, k
    net.load_state_dict(ck, strict=True)
    assert all(torch.equal(net.state_dict()[k], v) for k, v in ck.items())


def test_noise_checkpoint_depth_is_named():
    """conf_noise.yaml says depth 8, the checkpoint it names holds 6 levels: refused by name, with the depth to set."""
    a = diffusion.load_config("noise")
    a.network.checkpoint = weights_path("noise")
    with pytest.raises(ValueError, match=r"depth %d.*args.network.depth is 8" % NOISE_DEPTH):
        diffusion.DiffusionGenerator(a, "cpu")


def test_schedule_and_gamma_equal_the_references(gens):
    a = arrays()
    for n, key in (("trajectories", "trajectories"), ("toytrajectories", "toytrajectories"), ("noise", "noise_T3")):
        assert torch.equal(gens[n].schedule, torch.from_numpy(a[f"schedule_{key}"])), n
        assert torch.equal(gens[n].gamma, torch.from_numpy(a[f"gamma_{key}"])), n
    full = generator("noise")
    assert torch.equal(full.schedule, torch.from_numpy(a["schedule_noise"])) and torch.equal(full.gamma, torch.from_numpy(a["gamma_noise"]))
    assert gens["noise"].gamma[0] > 0 and gens["trajectories"].gamma[0] == 0


def test_forward_torch_trajectory_every_recorded_tensor(gens):
    a = arrays()
    x, s = normal(seeds()["ev"], (2, 512)), torch.from_numpy(a["ev_sigma"])
    net = gens["trajectories"].network
    for dt in (torch.float64, torch.float32):
        net.to(dt)
        rec = {}
        with torch.no_grad():
            y = net.forward_torch(x.to(dt), s.to(dt), record=rec.__setitem__)
        assert tuple(rec) == EV_BLOCKS and torch.equal(y, rec["final"])
        for n, v in rec.items():
            if dt == torch.float64:
                assert rel_err(v, a[f"ev_{n}_ref64"]) <= 1e-10, n
            else:
                check(f"ev_{n}", v)
    net.float()


@pytest.mark.parametrize("case,name,T,sig", [("toy_ev_out", "toytrajectories", 512, -0.9), ("noise_ev1k_out", "noise", 1024, -1.5),
                                             ("noise_ev16k_out", "noise", 16384, -1.5), ("noise_ev32k_out", "noise", 32768, -1.5)])
def test_forward_torch_whole_evaluations(gens, case, name, T, sig):
    a = arrays()
    x, s = normal(seeds()[case[:-4]], (1, T)), torch.tensor([[sig]])
    net = gens[name].network
    with torch.no_grad():
        y64 = net.double().forward_torch(x.double(), s.double())
        y32 = net.float().forward_torch(x, s)
    assert rel_err(y64, a[case + "_ref64"]) <= 1e-10
    check(case, y32)


def test_samplers_on_the_torch_path(gens):
    sd = seeds()
    t, n = gens["trajectories"], gens["noise"]
    with torch.no_grad():
        check("traj_sample", t.sample(draws=draws(sd["traj_sample"], 1, 512)))
        y = t.sample_long(9.3, draws=draws(sd["traj_long"], 1, 512))
        assert t.segments == 3 and y.shape == (1, 930 * 441)
        check("traj_long_44k", y[..., :88200])
        check("noise_sample", n.sample(draws=draws(sd["noise_sample"], 1, 16384)))
        xo, mask = outpaint_inputs(n)
        check("noise_outpaint", n.outpaint_sample(xo, mask, draws=draws(sd["noise_outpaint"], 1, 16384)))


def test_sample_long_at_100_hz_and_the_resampler(gens):
    t = gens["trajectories"]
    got = {}
    orig = t.resampler
    t.resampler = lambda x: got.setdefault("x", x.clone())
    try:
        with torch.no_grad():
            t.sample_long(9.3, draws=draws(seeds()["traj_long"], 1, 512))
    finally:
        t.resampler = orig
    assert got["x"].shape == (1, 930)
    check("traj_long_100", got["x"])
    x = torch.randn(2, 50)
    assert t.resampler(x).shape == (2, 50 * 441) and t._rs_kernel[0].shape == (441, 1, 15)
    n = gens["noise"]
    assert n.resampler(x) is x                                     # 44 100 -> 44 100


def test_batched_sampler_streams_equal_their_own_sample(gens):
    """sample_batch with draws given per stream: every stream is its own sample() (the torch path: to rounding of the batched
    convolutions; the HIP path pins bit equality in tests/test_gpu_diffusion.py)."""
    t = gens["trajectories"]
    per = [list(next(draws(100 + i, 1, 512)) for _ in range(1)) for i in range(3)]
    with torch.no_grad():
        batch = t.sample_batch(3, draws=iter([torch.cat([p[0] for p in per])]))
        single = [t.sample(draws=iter(p)) for p in per]
    assert batch.shape == (3, 512)
    for i in range(3):
        assert float((batch[i] - single[i][0]).abs().max() / single[i].abs().max()) < 1e-5


def test_pt_and_npz_checkpoints_load(tmp_path):
    """A `.pt` in the reference's layout -- the "ema" dict next to a pickled object of a class that is not installed."""
    import pickle
    import types
    with np.load(weights_path("toytrajectories")) as z:
        ema = {k: torch.from_numpy(z[k]) for k in z.files}
    mod = types.ModuleType("not_installed_conf")
    mod.DictConfig = type("DictConfig", (), {"__module__": "not_installed_conf"})
    import sys
    sys.modules["not_installed_conf"] = mod
    try:
        path = str(tmp_path / "toy.pt")
        torch.save({"ema": ema, "args": mod.DictConfig(), "it": 36000}, path)
    finally:
        del sys.modules["not_installed_conf"]
    a = config("toytrajectories")
    a.network.checkpoint = path
    g_pt, g_npz = diffusion.DiffusionGenerator(a, "cpu"), generator("toytrajectories")
    for (k, v), (k2, v2) in zip(g_pt.network.state_dict().items(), g_npz.network.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)
    assert pickle  # (imported for the reader: the .pt above is a pickle)


def test_refusals_of_the_host_layer():
    a = config("trajectories")
    a.network.use_norm = True
    with pytest.raises(ValueError, match="use_norm=True"):
        diffusion.UNet1D(a, "cpu")
    net = diffusion.UNet1D(config("trajectories"), "cpu")
    with pytest.raises(RuntimeError, match="HIP device only"):
        net(torch.zeros(1, 512), torch.zeros(1, 1))
    with pytest.raises(RuntimeError, match="HIP device only"):
        diffusion.resblock_forward(torch.zeros(1, 8, 16), torch.zeros(1, 8), torch.zeros(8, 8, 1), torch.zeros(8, 8, 8, 5))


# (B, T) -> bound calls, launches (a tiled block is two).  5000 -> 1250 -> 313 -> 79 -> 20 -> 5: tiled blocks and odd crops;
# 1024: a bottom level of one frame; 65536: the shipped segment
PLAN_CASES = [("trajectories", 2, 512, 16, 16), ("toytrajectories", 1, 512, 16, 16), ("noise", 1, 1024, 24, 24),
              ("noise", 3, 5000, 24, 28), ("noise", 1, 65536, 24, 30)]


@pytest.mark.parametrize("name,B,T,calls,launches", PLAN_CASES)
def test_plan_binds_the_tensors_forward_torch_records(gens, name, B, T, calls, launches):
    """The plan of the HIP path builds on CPU tensors (it allocates and asks the host-side workspace function): its named
    buffers are forward_torch's recorded tensors, name by name and shape by shape, and its launch counts are pinned."""
    net, cpu = gens[name].network, torch.device("cpu")
    plan = net._plan_for(B, T, False, cpu)
    rec = {}
    with torch.no_grad():
        net.forward_torch(torch.zeros(B, T), torch.tensor([[-1.5]]), record=rec.__setitem__)
    assert tuple(plan.buffers) == tuple(rec)
    for n, v in rec.items():
        assert plan.buffers[n].shape == v.shape, n
    assert len(plan.calls) == calls and plan.launches == launches
    assert len(plan.record_calls) == net.depth - 1 and len(plan.inputs) == 2 and len(plan.films) == 2 * net.depth + 1
    assert net._plan_for(B, T, False, cpu) is plan                       # served from the cache
    assert net._plan_for(B, T, True, cpu) is not plan
    net.load_state_dict(net.state_dict())
    assert not net._plans and net._plan_for(B, T, False, cpu) is not plan


def test_entry_points_are_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    L = ntm_amd._lib.lib()
    for s, nargs in SYMS.items():
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1] and len(ntm_amd._lib._SIGNATURES[s][1]) == nargs
    assert "ntm_unet_block" in header and ctypes.sizeof(diffusion.BlockSpec) == 64
    assert re.search(r"#define\s+NTM_ABI_VERSION\s+9\b", header) and L.ntm_abi_version() == 9
    assert re.search(r"#define\s+NTM_UNET_WHOLE_MAX_T\s+%d\b" % diffusion.WHOLE_MAX_T, header)
    assert re.search(r"#define\s+NTM_UNET_TILE\s+%d\b" % diffusion.TILE, header)
    assert "unet_kernels.hip" in open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "Makefile")).read()


def spec(c0=8, c1=0, c_out=8, n=8, T=100, T0=None, off0=0, T1=0, off1=0, init=0, form=0):
    return diffusion.BlockSpec(c0, c1, c_out, n, T, T if T0 is None else T0, off0, T1, off1, init, form)


def test_workspace_sizes():
    L = ntm_amd._lib.lib()
    ws = lambda B, s: L.ntm_unet_resblock_workspace_floats(B, ctypes.byref(s))
    assert ws(3, spec(T=1024)) == 0 and ws(3, spec(T=1025)) == 3 * 8 * 1025          # whole: one launch; tiled: y between two
    assert ws(2, spec(T=600, form=2, c_out=16, c0=16)) == 2 * 16 * 600 and ws(2, spec(T=5000, n=7)) == 0   # layers 0-6: one run
    assert ws(0, spec(T=5000)) == 0


BAD_BLOCKS = [(dict(c0=0), "channels"), (dict(c0=20, c1=13), "channels"), (dict(c_out=17), "c_out"), (dict(c_out=0), "c_out"),
              (dict(n=0), "n_layers"), (dict(n=9), "n_layers"), (dict(T=0), "T must be positive"), (dict(off0=-1), "src0"),
              (dict(T=100, T0=99), "src0"), (dict(c1=8, T1=99), "src1"), (dict(c1=8, T1=200, off1=101), "src1"),
              (dict(T=1, T0=2 ** 27), "2\\^31"), (dict(form=3), "form"), (dict(T=1025, form=1), "whole form")]


@pytest.mark.parametrize("kw,msg", BAD_BLOCKS)
def test_resblock_refusals_come_before_the_device(kw, msg):
    L = ntm_amd._lib.lib()
    s = spec(**kw)
    assert L.ntm_unet_resblock_workspace_floats(2, ctypes.byref(s)) == -1
    assert re.match(r"ntm_unet_resblock_workspace_floats: .*" + msg, L.ntm_last_error().decode())
    rc = L.ntm_unet_resblock_forward(P[0], P[1], None, P[2], 0, P[3], P[4], P[5], 2, ctypes.byref(s), P[6], P[7], None)
    assert rc == -1 and re.match(r"ntm_unet_resblock_forward: .*" + msg, L.ntm_last_error().decode())


def test_resblock_refusals_of_the_forward_alone():
    L = ntm_amd._lib.lib()
    fwd = lambda s, src0=P[0], src1=None, init_w=None, film=P[2], fs=0, wf=P[3], wg=P[4], wr=P[5], B=2, ws=P[6], out=P[7]: \
        (L.ntm_unet_resblock_forward(src0, src1, init_w, film, fs, wf, wg, wr, B, None if s is None else ctypes.byref(s), ws, out, None),
         L.ntm_last_error().decode())
    for call, msg in ((fwd(None), "null pointer"), (fwd(spec(), B=-1), "B must lie"), (fwd(spec(), B=65536), "B must lie"),
                      (fwd(spec(), fs=7), "film_stride"), (fwd(spec(c0=16), wr=None), "identity residual"),
                      (fwd(spec(), src0=None), "null pointer"), (fwd(spec(), film=None), "null pointer"),
                      (fwd(spec(c1=8, T1=100)), "null pointer"), (fwd(spec(init=1)), "null pointer"),
                      (fwd(spec(T=2000), ws=None), r"null pointer \(ws\)"), (fwd(spec(), out=P[0]), "alias")):
        assert call[0] == -1 and re.match(r"ntm_unet_resblock_forward: .*" + msg, call[1]), (call, msg)
    assert fwd(spec(), B=0, src0=None)[0] == 0
    assert L.ntm_unet_resblock_workspace_floats(2, None) == -1


def test_resample_and_edm_refusals_come_before_the_device():
    L = ntm_amd._lib.lib()
    err = lambda: L.ntm_last_error().decode()
    down = lambda x=P[0], B=2, C=8, F=100, S=4, width=25, taps=54: L.ntm_unet_down_combine(x, P[1], P[2], P[3], B, C, F, S, width, taps, P[4], P[5], None)
    for kw, msg in ((dict(x=None), "null pointer"), (dict(B=-1), "B must lie"), (dict(C=0), "C must lie"), (dict(C=33), "C must lie"),
                    (dict(F=0), "F must be positive"), (dict(S=0), "S must lie"), (dict(taps=53), "taps must be"),
                    (dict(width=-1, taps=2), "width"), (dict(S=2, width=40, taps=82), "taps at most 64"), (dict(F=2 ** 30), "2\\^31")):
        assert down(**kw) == -1 and re.match("ntm_unet_down_combine: .*" + msg, err()), (kw, err())
    assert down(B=0, x=None) == 0
    up = lambda x=P[0], pyr=P[1], pyr_T=100, ker=P[2], B=2, C=16, F=100, S=4, width=7, taps=15, xo=P[4]: \
        L.ntm_unet_up_combine(x, pyr, pyr_T, ker, P[3], B, C, F, S, width, taps, xo, P[5], None)
    for kw, msg in ((dict(x=None), "null pointer"), (dict(ker=None), "null pointer"), (dict(xo=None), "null pointer"),
                    (dict(taps=14), "taps must be"), (dict(S=1), "taps must be"), (dict(pyr_T=99), "shorter than F"),
                    (dict(S=1025), "S must lie"), (dict(F=2 ** 28), "2\\^31")):
        assert up(**kw) == -1 and re.match("ntm_unet_up_combine: .*" + msg, err()), (kw, err())
    assert up(B=0, x=None) == 0
    ups = lambda x=P[0], S=441, taps=15: L.ntm_unet_upsample(x, P[1], 1, 930, S, 7, taps, P[2], None)
    for kw, msg in ((dict(x=None), "null pointer"), (dict(S=1), "at least 2"), (dict(taps=16), "2 \\* width \\+ 1")):
        assert ups(**kw) == -1 and re.match("ntm_unet_upsample: .*" + msg, err()), (kw, err())
    pre = lambda z=P[0], mask=None, ms=0, xo=None, B=1, T=512: L.ntm_edm_pre(z, None, 0.0, 1.0, mask, ms, xo, xo, 0.1, 1.0, B, T, P[1], P[2], None)
    for kw, msg in ((dict(z=None), "null pointer"), (dict(B=-1), "negative"), (dict(mask=P[3]), "a mask comes with"),
                    (dict(mask=P[3], xo=P[4], ms=7), "mask_stride")):
        assert pre(**kw) == -1 and re.match("ntm_edm_pre: .*" + msg, err()), (kw, err())
    assert pre(B=0, z=None) == 0
    post = lambda z=P[0], N=512: L.ntm_edm_post(z, P[1], 1.0, 1.0, 1.0, 1.0, N, P[2], None)
    assert post(z=None) == -1 and err().startswith("ntm_edm_post: null pointer")
    assert post(N=-1) == -1 and err().startswith("ntm_edm_post: negative") and post(N=0, z=None) == 0
