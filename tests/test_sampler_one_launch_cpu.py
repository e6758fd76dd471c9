"""CPU: the host side of the one-launch sampler (DiffusionGenerator(sampler="one_launch"), ntm_unet_sample_one_launch,
csrc/unet_sampler.hip): the declaration and its binding, the stage record's size, the option's values, the refusals that are made
before anything touches a device, and the stage table against the step path's own plan."""
import ctypes
import os
import re

import pytest
import torch

import ntm_amd
from ntm_amd import _lib, diffusion
from diffusion_cases import config, generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"ntm_unet_sample_workspace_floats": 2, "ntm_unet_sample_one_launch": 19}
CPU = torch.device("cpu")


def small(**over):
    """A random network of the toy configuration's family on the CPU: no checkpoint."""
    return diffusion.DiffusionGenerator(config("toytrajectories", network__checkpoint=None, **over), "cpu")


def test_entry_points_are_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    L = _lib.lib()
    for s, nargs in SYMS.items():
        assert s in _lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == _lib._SIGNATURES[s][1] and len(_lib._SIGNATURES[s][1]) == nargs
        decl = re.search(r"\b%s\(([^;]*)\);" % s, header).group(1)
        assert len(decl.split(",")) == nargs, s
    assert re.search(r"#define\s+NTM_ABI_VERSION\s+9\b", header) and L.ntm_abi_version() == 9
    for name, v in (("MAX_STAGES", _lib.UNET_SAMPLE_MAX_STAGES), ("MAX_STEPS", _lib.UNET_SAMPLE_MAX_STEPS),
                    ("SCALARS", _lib.UNET_SAMPLE_SCALARS)):
        assert re.search(r"#define\s+NTM_UNET_SAMPLE_%s\s+%d\b" % (name, v), header), name
    for name, v in _lib.USTAGE_KINDS.items():
        assert re.search(r"#define\s+NTM_USTAGE_%s\s+%d\b" % (name.upper(), v), header), name
    assert "unet_sampler.hip" in open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "Makefile")).read()


def test_stage_record_is_the_headers_struct():
    """168 bytes: the number the header documents, the .hip file static_asserts on the C struct and the binding states."""
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    kernel = open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "unet_sampler.hip")).read()
    assert ctypes.sizeof(_lib.UnetStage) == 168 == _lib.UNET_STAGE_BYTES and ctypes.sizeof(_lib.UnetBlock) == 64
    assert re.search(r"\}\s*ntm_unet_stage;\s*/\* 168 bytes \*/", header)
    assert re.search(r"static_assert\(sizeof\(ntm_unet_stage\) == 168\b", kernel)
    body = re.search(r"typedef struct \{([^}]*)\}\s*ntm_unet_stage;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    names = [n.strip(" *") for line in body.split(";") if line.strip() for n in line.split(None, 1)[1].replace("float", "").split(",")]
    assert names == [f[0] for f in _lib.UnetStage._fields_]
    assert diffusion.BlockSpec is _lib.UnetBlock and _lib.UnetStage.blk.offset == 40 and _lib.UnetStage.a.offset == 104


def test_sampler_option_values():
    g = generator("toytrajectories")
    assert g.sampler == "steps" and diffusion.SAMPLERS == ("steps", "one_launch")
    assert generator("toytrajectories").sampler == "steps"
    with pytest.raises(ValueError, match="bogus"):
        diffusion.DiffusionGenerator(config("toytrajectories"), "cpu", sampler="bogus")
    g.sampler = "bogus"                                   # a plain attribute: read, and refused, by the next call
    with pytest.raises(ValueError, match="bogus"):
        g.sample()
    g.sampler = "steps"
    assert g.sample().shape == (1, 512) and g.last_launches == 0        # the torch path: none of this project's launches


def test_one_launch_on_the_cpu_is_refused():
    g = diffusion.DiffusionGenerator(config("toytrajectories"), "cpu", sampler="one_launch")
    for call in (g.sample, lambda: g.sample_batch(2), lambda: g.outpaint_sample(torch.zeros(1, 512), torch.zeros(1, 512)),
                 lambda: g.sample_long(6.0)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()


def test_level_lengths():
    assert generator("trajectories").network.level_lengths(512) == [512, 256, 128, 32]
    n = diffusion.UNet1D(config("noise"), "cpu")
    assert n.level_lengths(65536) == [65536, 16384, 4096, 1024, 256, 64]
    assert small(network__depth=3, network__Ns=[8, 16, 16, 16], network__Ss=[4, 4, 4]).network.level_lengths(100) == [100, 25, 7]


CASES = [dict(), dict(network__depth=3, network__Ns=[8, 16, 16, 16], network__Ss=[4, 4, 4], exp__seg_len=100),
         dict(network__depth=2, network__Ns=[5, 12, 12], network__Ss=[3, 3], exp__seg_len=1000)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("over", CASES, ids=["toy", "depth3_T100", "depth2_S3_T1000"])
def test_stage_table_lists_the_plans_calls(over, B):
    """The table against the _Plan of the step path, call by call: kind, shapes and operands, with what run() patches per
    evaluation (input, FiLM row, output) null -- also after a run has patched the plan's own arguments."""
    g = small(**over)
    net, T = g.network, g.seg_len
    plan = net._plan_for(B, T, False, CPU)
    kinds = {"ntm_unet_resblock_forward": "block", "ntm_unet_down_combine": "down", "ntm_unet_up_combine": "up"}
    for patched in (False, True):
        if patched:            # what run() does to the bound arguments, without launching
            for args, pos in plan.inputs + [plan.output]:
                args[pos] = 0xdead0000
        table = plan.stages()
        assert len(table) == len(plan.calls) == 4 * net.depth
        for i, (st, call) in enumerate(zip(table, plan.calls)):
            want = "final" if i == len(table) - 1 else kinds[call.name]
            assert st.kind == _lib.USTAGE_KINDS[want], i
            outs = call.out if isinstance(call.out, tuple) else (call.out,)
            if want == "block":
                k, sp = st.blk, call.spec
                assert [getattr(k, f) for f, _ in k._fields_] == [getattr(sp, f) for f, _ in sp._fields_]
                assert (k.c_out, k.T) == tuple(outs[0].shape[1:]) and k.T <= diffusion.WHOLE_MAX_T and k.form == 0
                assert st.film_off == plan.offs[sum(c.name == call.name for c in plan.calls[:i])]
                assert st.o0 == outs[0].data_ptr() and (st.a is None) == (i == 0) and (st.b is None) == (k.c1 == 0)
                assert st.w0 and st.w1 and (st.w3 is not None) == bool(k.init)
            else:
                x_out, p_out = outs
                Fo = -(-st.F // st.S) if want == "down" else st.S * st.F
                assert p_out.shape == (B, Fo) if want == "final" else p_out.shape == (B, 1, Fo)
                assert st.a and st.w1 and (st.w0 is None) == (want == "final")
                if want == "final":
                    assert (st.S, st.taps, st.width, st.F, st.o0, st.o1) == (1, 0, 0, T, None, None)
                else:
                    assert x_out.shape == (B, st.C, Fo) and st.o0 == x_out.data_ptr() and st.o1 == p_out.data_ptr()
                    assert st.taps == (2 * st.width + st.S if want == "down" else 2 * st.width + 1)
                if want == "down":
                    assert (st.b is None) == (i == 1)                      # the first pyramid is the network's input
    kinds_in_order = [st.kind for st in plan.stages()]
    d = net.depth
    assert kinds_in_order == [0, 1] * (d - 1) + [0, 0] + [0, 2] * (d - 1) + [0, 3]


def test_raw_entry_refuses_bad_arguments_before_any_device_work():
    """With made-up non-null pointers: every refusal comes back as NTM_EINVAL with the function's name, nothing is launched."""
    L = _lib.lib()
    g = small()
    B, T = 2, g.seg_len
    plan = g.network._plan_for(B, T, False, CPU)
    P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]

    def call(stages=None, n_stages=None, film_len=200, n_steps=4, eps=0, n_draws=0, xo=None, mask=None, ms=0, B=B, T=T, z=P[5]):
        stages = plan.stages() if stages is None else stages
        host = _lib.unet_stages(stages)
        rc = L.ntm_unet_sample_one_launch(host, P[0], len(stages) if n_stages is None else n_stages, P[1], P[2], film_len, n_steps,
                                          eps, P[3], P[6] if n_draws else None, n_draws, xo, mask, ms, B, T, P[4], z, None)
        return rc, L.ntm_last_error().decode()

    def edited(i, **fields):
        st = plan.stages()
        for k, v in fields.items():
            setattr(st[i], k, v)
        return st

    assert L.ntm_unet_sample_workspace_floats(3, 512) == 3 * 3 * 512
    assert L.ntm_unet_sample_workspace_floats(1, 1025) == -1 and L.ntm_unet_sample_workspace_floats(65536, 512) == -1
    assert call(B=0)[0] == 0                                                       # nothing to do
    bad = [dict(T=1025), dict(T=0), dict(B=65536), dict(n_steps=65), dict(n_steps=0), dict(n_stages=65), dict(n_stages=0),
           dict(film_len=100), dict(n_draws=1), dict(eps=0b101, n_draws=1), dict(mask=P[7]), dict(xo=P[7]),
           dict(mask=P[7], xo=P[6], n_draws=4, ms=5), dict(z=P[3]), dict(z=P[4]),
           dict(stages=edited(0, kind=7)), dict(stages=edited(1, taps=65)), dict(stages=edited(1, C=33)), dict(stages=edited(1, F=1025)),
           dict(stages=edited(1, F=100)), dict(stages=edited(1, o1=None)), dict(stages=edited(9, S=1024)),
           dict(stages=edited(11, pyr_T=3)), dict(stages=edited(15, F=100)), dict(stages=edited(15, S=2)),
           dict(stages=edited(0, film_off=-1)), dict(stages=edited(2, w0=None))]
    st = plan.stages()
    st[0].blk.T = st[0].blk.T0 = 2048
    bad.append(dict(stages=st))
    st = plan.stages()
    st[2].blk.n_layers = 9
    bad.append(dict(stages=st))
    st = plan.stages()
    st[2].blk.form = 2
    bad.append(dict(stages=st))
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("ntm_unet_sample_one_launch"), (bad.index(kw), rc, msg)
