"""GPU: the diffusion generators on the HIP path (csrc/unet_kernels.hip under ntm_amd.diffusion) against the reference's own
numbers (tests/golden/g29_*) and against this project's torch path in float64.

The bar of a float32 result is 3 x the float32-against-float64 distance of the torch implementation on the same case, max norm
relative to max |ref64|: for the goldens the reference's own two runs (diffusion_cases.bar), for the kernel-level cases the torch
module run here in both precisions on the CPU.  The margin covers the device's erf / division against libm and the matrix pipe's
summation order.  Every figure is printed before it is held against its bar."""
import numpy as np
import pytest
import torch

from ntm_amd import diffusion
from diffusion_cases import (EV_BLOCKS, NOISE_SMALL, arrays, check, draws, generator, normal, outpaint_inputs, seeds)

pytestmark = pytest.mark.gpu
DEV = "cuda"
R2 = 2 ** 0.5


@pytest.fixture(scope="module")
def gens():
    return {"trajectories": generator("trajectories", DEV), "toytrajectories": generator("toytrajectories", DEV),
            "noise": generator("noise", DEV, **NOISE_SMALL)}


@pytest.fixture(scope="module")
def ev_record(gens):
    x, s = normal(seeds()["ev"], (2, 512)).to(DEV), torch.from_numpy(arrays()["ev_sigma"]).to(DEV)
    rec = {}
    with torch.no_grad():
        y = gens["trajectories"].network(x, s, record=rec.__setitem__)
    assert torch.equal(y, rec["final"])
    return rec


@pytest.mark.parametrize("block", EV_BLOCKS)
def test_trajectory_evaluation_every_block_and_combiner(ev_record, block):
    check(f"ev_{block}", ev_record[block])


@pytest.mark.parametrize("case,name,T,sig", [("toy_ev_out", "toytrajectories", 512, -0.9), ("noise_ev1k_out", "noise", 1024, -1.5),
                                             ("noise_ev16k_out", "noise", 16384, -1.5), ("noise_ev32k_out", "noise", 32768, -1.5)])
def test_whole_evaluations(gens, case, name, T, sig):
    x = normal(seeds()[case[:-4]], (1, T)).to(DEV)
    with torch.no_grad():
        y = gens[name].network(x, torch.tensor([[sig]], device=DEV))
    check(case, y)


def test_trajectory_sampler_and_sample_long(gens):
    t, sd = gens["trajectories"], seeds()
    check("traj_sample", t.sample(draws=draws(sd["traj_sample"], 1, 512)))
    got = {}
    orig = t.resampler
    t.resampler = lambda x: orig(got.setdefault("x", x.clone()))
    try:
        y = t.sample_long(9.3, draws=draws(sd["traj_long"], 1, 512))
    finally:
        t.resampler = orig
    assert t.segments == 3 and y.shape == (1, 930 * 441) and got["x"].shape == (1, 930)
    check("traj_long_100", got["x"])
    check("traj_long_44k", y[..., :88200])


def test_noise_sampler_and_outpainting(gens):
    n, sd = gens["noise"], seeds()
    check("noise_sample", n.sample(draws=draws(sd["noise_sample"], 1, 16384)))
    xo, mask = outpaint_inputs(n)
    check("noise_outpaint", n.outpaint_sample(xo.to(DEV), mask.to(DEV), draws=draws(sd["noise_outpaint"], 1, 16384)))


# ---- the ResnetBlock kernel alone ------------------------------------------------------------------------------------------------

def block_case(c0, c1, c_out, T, seed=0, B=2):
    """A seeded ResnetBlock of the torch path, inputs with the first source 5 frames longer than T when there is a second one
    (the crop starts at frame 2), and its output in float64 and float32 on the CPU."""
    torch.manual_seed(seed)
    blk = diffusion.ResnetBlock(c0 + c1, c_out, 16)
    g = np.random.RandomState(seed + 1)
    off0 = 2 if c1 else 0
    src0 = torch.from_numpy(g.standard_normal((B, c0, T + (5 if c1 else 0))).astype(np.float32))
    src1 = torch.from_numpy(g.standard_normal((B, c1, T)).astype(np.float32)) if c1 else None
    film = torch.from_numpy((1.0 + 0.5 * g.standard_normal((B, c0 + c1))).astype(np.float32))

    def torch_out(dt):
        x = src0[:, :, off0:off0 + T] if src1 is None else torch.cat((src0[:, :, off0:off0 + T], src1), 1)
        x = x.to(dt) * film.to(dt).unsqueeze(-1)
        b = blk.to(dt)
        y = b.first_conv(x)
        for h in b.H:
            y = h(y)
        return ((y + b.res_conv(x)) / R2).detach()

    with torch.no_grad():
        r64, r32 = torch_out(torch.float64), torch_out(torch.float32)
    blk.float()
    return blk, src0, src1, film, off0, r64, r32


def run_block(blk, src0, src1, film, off0, T, form, rows=slice(None)):
    d = lambda t: None if t is None else t[rows].contiguous().to(DEV)
    res = None if isinstance(blk.res_conv, torch.nn.Identity) else blk.res_conv.weight.detach().to(DEV)
    gated = torch.stack([h.conv.weight.detach() for h in blk.H]).contiguous().to(DEV)
    return diffusion.resblock_forward(d(src0), d(film), blk.first_conv[1].weight.detach().to(DEV), gated, res, d(src1), off0, T,
                                      form=form)


CHANNELS = [(8, 0, 8), (4, 4, 8), (32, 0, 16), (16, 16, 16)]
SHAPES = [(1, "auto"), (4, "auto"), (5, "auto"), (255, "auto"), (1000, "auto"), (1024, "auto"), (1025, "auto"),
          (511, "tiled"), (512, "tiled"), (513, "tiled"), (1027, "tiled")]


@pytest.mark.parametrize("T,form", SHAPES)
@pytest.mark.parametrize("c0,c1,c_out", CHANNELS)
def test_resblock_kernel_at_the_edges(c0, c1, c_out, T, form):
    blk, src0, src1, film, off0, r64, r32 = block_case(c0, c1, c_out, T)
    got = run_block(blk, src0, src1, film, off0, T, form).cpu().double()
    scale = float(r64.abs().max())
    own = float((r32.double() - r64).abs().max()) / scale
    err = float((got - r64).abs().max()) / scale
    print(f"resblock {c0}+{c1}->{c_out} T={T} {form}: error {err:.3e}, torch float32's own {own:.3e}, ratio {err / own:.2f}")
    # a handful of outputs (T = 1: 16 numbers) can sit closer to float64 than float32 resolves: never ask for less than one ulp
    assert got.shape == r64.shape and err <= 3.0 * max(own, 2.0 ** -23)


@pytest.mark.parametrize("T,form", [(700, "auto"), (1500, "auto")])
def test_resblock_batch_of_three_equals_three_calls_and_repeats(T, form):
    blk, src0, src1, film, off0, _, _ = block_case(16, 16, 16, T, seed=3, B=3)
    all3 = run_block(blk, src0, src1, film, off0, T, form)
    assert torch.equal(all3, run_block(blk, src0, src1, film, off0, T, form))            # two equal calls, equal bits
    for i in range(3):
        assert torch.equal(all3[i:i + 1], run_block(blk, src0, src1, film, off0, T, form, rows=slice(i, i + 1))), i


def test_resblock_init_conv_form():
    """The first block of the network: the waveform through init_conv on the fly, whole and tiled."""
    torch.manual_seed(5)
    blk, conv = diffusion.ResnetBlock(8, 8, 16), torch.nn.Conv1d(1, 8, 5, padding="same", bias=False)
    for T in (37, 1300):
        wav = normal(50 + T, (2, 1, T))
        film = 1.0 + 0.5 * normal(51, (1, 8))
        outs = []
        for dt in (torch.float64, torch.float32):
            with torch.no_grad():
                x = conv.to(dt)(wav.to(dt)) * film.to(dt).unsqueeze(-1)
                b = blk.to(dt)
                y = b.first_conv(x)
                for h in b.H:
                    y = h(y)
                outs.append(((y + x) / R2).double())
        blk.float(), conv.float()
        gated = torch.stack([h.conv.weight.detach() for h in blk.H]).contiguous().to(DEV)
        got = diffusion.resblock_forward(wav.to(DEV), film.to(DEV), blk.first_conv[1].weight.detach().to(DEV), gated,
                                         init_w=conv.weight.detach().to(DEV)).cpu().double()
        scale = float(outs[0].abs().max())
        own, err = float((outs[1] - outs[0]).abs().max()) / scale, float((got - outs[0]).abs().max()) / scale
        print(f"init-conv block T={T}: error {err:.3e}, torch float32's own {own:.3e}, ratio {err / own:.2f}")
        assert err <= 3.0 * max(own, 2.0 ** -23)


# ---- the resample + combine kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 3, 54, 1000])
@pytest.mark.parametrize("S", [2, 4])
def test_down_and_up_combine_kernels(S, F):
    torch.manual_seed(S * 1000 + F)
    C, B = 16, 2
    down, cd = diffusion.Downsample(S), diffusion.CombinerDown(1, C)
    up, cu = diffusion.Upsample(S), diffusion.CombinerUp(1, C)
    torch.nn.init.normal_(cu.conv1x1.weight, std=0.3)
    x, pyr, pyr_long = normal(F, (B, C, F)), normal(F + 1, (B, 1, F)), normal(F + 2, (B, 1, F + 3))

    def ref(dt):
        with torch.no_grad():
            d, c, u, k = down.to(dt), cd.to(dt), up.to(dt), cu.to(dt)
            pd = d(pyr.to(dt))
            p0, p1 = k(None, x.to(dt)), k(pyr_long.to(dt), x.to(dt))
            return [c(pd, d(x.to(dt))), pd, u(x.to(dt)), u(p0), u(p1), p1]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for m in (down, cd, up, cu):
        m.float()
    g = lambda t: t.to(DEV)
    xo, po = diffusion.down_combine(g(x), g(pyr), g(down.resample.kernel), g(cd.conv1x1.weight.detach()), S, down.resample.width)
    wc, ku = g(cu.conv1x1.weight.detach()), g(up.resample.kernel)
    xu, pu0 = diffusion.up_combine(g(x), None, ku, wc, S, up.resample.width)
    xu1, pu1 = diffusion.up_combine(g(x), g(pyr_long), ku, wc, S, up.resample.width)
    none, pl = diffusion.up_combine(g(x), g(pyr_long), None, wc, 1, 0)
    assert none is None and torch.equal(xu, xu1)
    for name, got, a, b in zip(("down x", "down pyr", "up x", "up pyr (none)", "up pyr", "combiner"), (xo, po, xu, pu0, pu1, pl), r64, r32):
        scale = float(a.abs().max())
        own, err = float((b.double() - a).abs().max()) / scale, float((got.cpu().double() - a).abs().max()) / scale
        print(f"S={S} F={F} {name}: error {err:.3e}, torch float32's own {own:.3e}")
        assert got.shape == a.shape and err <= 3.0 * max(own, 2.0 ** -24), name     # own can be 0 on a one-frame case: half an ulp then


def test_network_batch_of_three_equals_three_calls_and_repeats(gens):
    net = gens["noise"].network
    x, s = normal(7, (3, 5000)).to(DEV), torch.tensor([[-1.5]], device=DEV)
    with torch.no_grad():
        y = net(x, s)
        assert torch.equal(y, net(x, s))
        for i in range(3):
            assert torch.equal(y[i:i + 1], net(x[i:i + 1], s)), i


@pytest.mark.parametrize("sigma", [[[-1.5]], [[-1.5], [-0.7], [-2.2]]], ids=["shared_sigma", "per_stream_sigma"])
def test_recording_reports_the_plans_own_buffers(gens, sigma):
    """record= on the shipped path, at a shape with tiled blocks and odd crops (5000 -> 1250 -> 313 -> 79 -> 20 -> 5): it
    disturbs nothing, names what forward_torch names, and every tensor meets the bar of the kernel-level cases."""
    net, cpu = gens["noise"].network, generator("noise", **NOISE_SMALL).network
    x, s = normal(7, (3, 5000)), torch.tensor(sigma)
    rec, refs = {}, ({}, {})
    with torch.no_grad():
        y = net(x.to(DEV), s.to(DEV), record=rec.__setitem__)
        assert torch.equal(y, rec["final"]) and torch.equal(y, net(x.to(DEV), s.to(DEV)))
        for r, dt in zip(refs, (torch.float64, torch.float32)):
            cpu.to(dt).forward_torch(x.to(dt), s.to(dt), record=r.__setitem__)
    assert tuple(rec) == tuple(refs[0])
    for name, got in rec.items():
        r64, r32 = refs[0][name], refs[1][name]
        scale = float(r64.abs().max())
        own, err = float((r32.double() - r64).abs().max()) / scale, float((got.cpu().double() - r64).abs().max()) / scale
        print(f"{name}: error {err:.3e}, torch float32's own {own:.3e}, ratio {err / own:.2f}")
        assert got.shape == r64.shape and err <= 3.0 * max(own, 2.0 ** -23), name


def test_sample_batch_streams_equal_their_own_sample_bit_for_bit(gens):
    n = gens["noise"]                     # the epsilon branch: two draws per step
    streams = [[next(d) for _ in range(8)] for d in (draws(300 + i, 1, 16384) for i in range(3))]
    batch = n.sample_batch(3, draws=iter([torch.cat([s[k] for s in streams]) for k in range(8)]))
    for i in range(3):
        assert torch.equal(batch[i:i + 1], n.sample(draws=iter(streams[i]))), i
    t = gens["trajectories"]
    streams = [[next(draws(400 + i, 1, 512))] for i in range(3)]
    batch = t.sample_batch(3, draws=iter([torch.cat([s[0] for s in streams])]))
    for i in range(3):
        assert torch.equal(batch[i:i + 1], t.sample(draws=iter(streams[i]))), i


def test_edm_step_kernels_follow_the_reference_expressions(gens):
    """ntm_edm_pre / ntm_edm_post against the reference's tensor expressions in float64, the bar from the same expressions in
    float32 on the CPU.  (z - k score cancels to sigma_next / sigma of z: float32 runs that differ only in how the division is
    rounded -- a quotient here, a product with the reciprocal in torch's kernels -- sit 2.8e-6 apart on this case, so bits are not
    compared.)"""
    n = gens["noise"]
    st = n._plan()[0]
    B, T = 2, 16384
    z, eps, noise, Fx = (normal(60 + i, (B, T)) for i in range(4))
    z = z * 0.1
    xo, mask = outpaint_inputs(n)

    def ref(dt):
        c = lambda v: v.to(dt)
        wz = c(z) + c(st["eps"]) * (c(eps) * n.Snoise)
        wz = c(mask) * (c(xo) + c(noise) * c(st["s0"])) + (1 - c(mask)) * wz
        x0 = c(st["cskip"]) * wz + c(st["cout"]) * c(Fx)
        return c(st["cin"]) * wz, wz - c(st["k"]) * ((x0 - wz) / c(st["b2"]))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    n.network_saved, calls = n.network, []

    class Net:
        def __call__(self, net_in, sigma, films=None):
            calls.append(net_in.clone())
            return Fx.to(DEV)
    n.network = Net()
    try:
        got = n._hip_step(z.to(DEV), st, eps.to(DEV), xo.to(DEV), mask.to(DEV), noise.to(DEV))
    finally:
        n.network = n.network_saved
    for name, g, a, b in (("net_in", calls[0], r64[0], r32[0]), ("z", got, r64[1], r32[1])):
        scale = float(a.abs().max())
        own, err = float((b.double() - a).abs().max()) / scale, float((g.cpu().double() - a).abs().max()) / scale
        print(f"edm {name}: error {err:.3e}, torch float32's own {own:.3e}, equal bits: {torch.equal(g.cpu(), b)}")
        assert err <= 3.0 * own
