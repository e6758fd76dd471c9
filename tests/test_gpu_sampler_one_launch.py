"""GPU: DiffusionGenerator(sampler="one_launch") -- the whole sampler as one launch of csrc/unet_sampler.hip -- against the
step-by-step path of the same generator with the same supplied draws.  Every comparison is torch.equal: the two modes run the
same code per output (csrc/unet_steps.h, csrc/unet_block.h), so there is no tolerance to state.

Depth 1, which the issue lists among the small nets, cannot be built: UNet1D needs depth >= 2 (its last level reuses the combiner
of the level before, as the reference does) and says so with a ValueError, in either mode; test_depth_one_is_refused_as_before
pins that, and depth 2 is the shallowest network the small cases run."""
import ctypes

import pytest
import torch

from ntm_amd import _lib, diffusion
from diffusion_cases import config, draws, generator

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHIPPED = ("trajectories", "toytrajectories")       # the shipped checkpoints whose levels are all <= 1024 frames


def both(gen, call, seed, B):
    """call(gen, draws) in the two modes with the same frozen draws -> (steps, one_launch), with their launch counts checked."""
    keep, out = gen.sampler, {}
    try:
        for mode in diffusion.SAMPLERS:
            gen.sampler = mode
            out[mode] = call(gen, draws(seed, B, gen.seg_len))
            plan = gen.network._plan_for(B, gen.seg_len, False, torch.device(DEV))
            want = 1 if mode == "one_launch" else (len(gen.schedule) - 1) * (plan.launches + 2)
            assert gen.last_launches == want, (mode, gen.last_launches, want)
    finally:
        gen.sampler = keep
    assert torch.isfinite(out["steps"]).all() and out["steps"].abs().max() > 0
    return out["steps"], out["one_launch"]


def assert_modes_equal(gen, call, seed, B):
    a, b = both(gen, call, seed, B)
    assert a.shape == b.shape and torch.equal(a, b), float((a - b).abs().max())
    return b


@pytest.fixture(scope="module")
def gens():
    return {n: generator(n, DEV) for n in SHIPPED}


def outpaint_operands(gen, B, per_stream, seed=7):
    g = torch.Generator().manual_seed(seed)
    T = gen.seg_len
    xo = (torch.randn(B, T, generator=g) * gen.sigma_data).to(DEV)
    mask = torch.zeros(B if per_stream else 1, T)
    for i in range(mask.shape[0]):
        mask[i, :T // 4 + 13 * i] = 1
    return xo, mask.to(DEV)


@pytest.mark.parametrize("name", SHIPPED)
def test_shipped_checkpoints(gens, name):
    g = gens[name]
    assert_modes_equal(g, lambda g, d: g.sample(draws=d), 11, 1)
    assert_modes_equal(g, lambda g, d: g.sample_batch(3, draws=d), 12, 3)
    for per_stream in (False, True):
        xo, mask = outpaint_operands(g, 3, per_stream)
        assert mask.shape[0] == (3 if per_stream else 1)
        assert_modes_equal(g, lambda g, d: g.outpaint_sample(xo, mask, draws=d), 13, 3)


def test_seeded_runs_without_draws_agree(gens):
    g, out = gens["toytrajectories"], {}
    try:
        for mode in diffusion.SAMPLERS:
            g.sampler = mode
            torch.manual_seed(5)
            out[mode] = g.sample_batch(2)
    finally:
        g.sampler = "steps"
    assert torch.equal(out["steps"], out["one_launch"])


# ---- small random networks -----------------------------------------------------------------------------------------------------------

def small(seed=0, one_step=False, **over):
    """A random network of the toy configuration's family (no checkpoint; the zero-initialised CombinerUp weights drawn too)."""
    torch.manual_seed(seed)
    g = diffusion.DiffusionGenerator(config("toytrajectories", network__checkpoint=None, **over), DEV)
    with torch.no_grad():
        for p in g.network.parameters():
            if float(p.abs().max()) == 0.0:
                p.normal_(0.0, 0.5)
    if one_step:          # sigma_max -> 0 in one step (create_schedule needs two)
        g._schedule = torch.tensor([float(g.sigma_max), 0.0])
        g._gamma = g.get_gamma(g._schedule)
        g.schedule, g.gamma, g._steps = g._schedule.to(g.device), g._gamma.to(g.device), None
    return g


# levels 1024 | 512: a level of exactly 1024 frames; 5 and 12 channels: not multiples of 16 (5: nor of 4); one step; no eps
EXACT_1024 = dict(network__depth=2, network__Ns=[5, 12, 12], network__Ss=[2, 2], exp__seg_len=1024, one_step=True)
# levels 100 | 25 | 7: not multiples of 16, the lowest below 16 frames; Schurn > 0: an eps draw in every step
ODD_LEVELS = dict(network__depth=3, network__Ns=[8, 16, 16, 16], network__Ss=[4, 4, 4], exp__seg_len=100, diff_params__T=3,
                  diff_params__Schurn=0.6)
# levels 1000 | 334: S = 3, the up path carries 1002 frames into a skip of 1000 (a crop), 41 taps down
CROP_S3 = dict(network__depth=2, network__Ns=[6, 10, 10], network__Ss=[3, 3], exp__seg_len=1000, diff_params__T=2)
SMALL = {"exact_1024": EXACT_1024, "odd_levels": ODD_LEVELS, "crop_s3": CROP_S3}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", list(SMALL))
def test_small_random_nets(case, B):
    g = small(seed=len(case), **SMALL[case])
    steps = g._plan()
    assert len(steps) == {"exact_1024": 1, "odd_levels": 3, "crop_s3": 2}[case]
    assert all((st["eps"] is not None) == (case == "odd_levels") for st in steps)          # the null-draw path and the other
    assert max(g.network.level_lengths(g.seg_len)) <= diffusion.WHOLE_MAX_T
    assert_modes_equal(g, lambda g, d: g.sample_batch(B, draws=d), 21, B)
    xo, mask = outpaint_operands(g, B, per_stream=B > 1)
    assert_modes_equal(g, lambda g, d: g.outpaint_sample(xo, mask, draws=d), 22, B)


def test_depth_one_is_refused_as_before():
    for mode in diffusion.SAMPLERS:
        g = diffusion.DiffusionGenerator(config("toytrajectories", network__checkpoint=None, network__depth=1, network__Ns=[8, 8],
                                                network__Ss=[2]), DEV, sampler=mode)
        with pytest.raises(ValueError, match="depth >= 2"):
            g.sample()


def test_a_stream_does_not_see_its_batch(gens):
    g = small(seed=3, **ODD_LEVELS)                       # two draws per step with the mask: eps and n
    g.sampler = "one_launch"
    xo, mask = outpaint_operands(g, 3, per_stream=True)
    n = 1 + 2 * len(g._plan())
    streams = [[next(d) for _ in range(n)] for d in (draws(300 + i, 1, g.seg_len) for i in range(3))]
    batch = g.outpaint_sample(xo, mask, draws=iter([torch.cat([s[k] for s in streams]) for k in range(n)]))
    for i in range(3):
        assert torch.equal(batch[i:i + 1], g.outpaint_sample(xo[i:i + 1], mask[i:i + 1], draws=iter(streams[i]))), i
    t = gens["trajectories"]
    t.sampler = "one_launch"
    try:
        streams = [[next(draws(400 + i, 1, 512))] for i in range(3)]
        batch = t.sample_batch(3, draws=iter([torch.cat([s[0] for s in streams])]))
        for i in range(3):
            assert torch.equal(batch[i:i + 1], t.sample(draws=iter(streams[i]))), i
    finally:
        t.sampler = "steps"


def test_equal_calls_give_equal_bits_and_a_parameter_update_is_seen():
    g = small(seed=4, **CROP_S3)
    g.sampler = "one_launch"
    first = g.sample_batch(2, draws=draws(31, 2, g.seg_len))
    assert torch.equal(first, g.sample_batch(2, draws=draws(31, 2, g.seg_len)))
    table = g.network._plan_for(2, g.seg_len, False, torch.device(DEV)).one_launch
    with torch.no_grad():                                 # in place: what an optimiser's step does
        g.network.middle[0][0].H[3].conv.weight.mul_(1.5)
        g.network.downs[0][0].first_conv[1].weight.add_(0.05)
    after = assert_modes_equal(g, lambda g, d: g.sample_batch(2, draws=d), 31, 2)
    assert not torch.equal(after, first)
    assert g.network._plan_for(2, g.seg_len, False, torch.device(DEV)).one_launch is not table    # rebuilt with the plan


def test_launch_counts_and_sample_long(gens):
    t = gens["trajectories"]
    plan = t.network._plan_for(1, 512, False, torch.device(DEV))
    assert len(plan.calls) == plan.launches == 16
    t.sample(draws=draws(1, 1, 512))
    assert t.sampler == "steps" and t.last_launches == 8 * (16 + 2) == 144
    a, b = both(t, lambda g, d: g.sample_long(9.3, draws=d), 41, 1)          # the first segment and two outpainting hops
    assert t.segments == 3 and a.shape == (1, 930 * 441) and torch.equal(a, b)
    a, b = both(t, lambda g, d: g.sample_long(9.3, batch=2, draws=d), 42, 2)
    assert torch.equal(a, b)


def test_the_noise_net_is_refused_by_name_of_its_levels():
    n = generator("noise", DEV)
    n.sampler = "one_launch"
    with pytest.raises(RuntimeError, match=r"65536, 16384, 4096, 1024, 256, 64\].*\[65536, 16384, 4096\]"):
        n.sample()
    n.sampler = "steps"                                   # nothing was consumed or cached by the refusal
    assert n._steps is None


def test_arguments_beyond_a_cap_leave_the_output_untouched(gens):
    g, L = gens["toytrajectories"], _lib.lib()
    B, T, dev = 2, g.seg_len, torch.device(DEV)
    g.sampler = "one_launch"
    try:
        ref = g.sample_batch(B, draws=draws(51, B, T))
    finally:
        g.sampler = "steps"
    scal, films, bits = g._one_launch_consts()
    host, table, ws = g.network._plan_for(B, T, False, dev).one_launch
    z0 = next(draws(51, B, T)).to(dev) * g.schedule[0]
    z = torch.full((B, T), 7.0, device=dev)

    def call(n_stages=len(host), n_steps=len(g._plan()), film_len=films.shape[1], T=T, B=B, stages=host):
        rc = L.ntm_unet_sample_one_launch(stages, _lib.ptr(table), n_stages, _lib.ptr(scal), _lib.ptr(films), film_len, n_steps, bits,
                                          _lib.ptr(z0), None, 0, None, None, 0, B, T, _lib.ptr(ws), _lib.ptr(z), _lib.current_stream())
        torch.cuda.synchronize()
        return rc

    over = _lib.unet_stages(g.network._plan_for(B, T, False, dev).stages())
    over[1].taps = 65
    deep = _lib.unet_stages(g.network._plan_for(B, T, False, dev).stages())
    deep[2].blk.n_layers = 9
    wide = _lib.unet_stages(g.network._plan_for(B, T, False, dev).stages())
    wide[2].blk.c_out = 17
    for kw in (dict(n_steps=65), dict(n_stages=65), dict(T=1025), dict(B=65536), dict(film_len=films.shape[1] - 1), dict(stages=over),
               dict(stages=deep), dict(stages=wide)):
        assert call(**kw) == -1 and L.ntm_last_error().decode().startswith("ntm_unet_sample_one_launch"), kw
        assert bool((z == 7.0).all()), kw
    assert call() == 0 and torch.equal(z, ref)                      # the same buffers, within the caps: the sample
    assert ctypes.sizeof(host) == len(host) * _lib.UNET_STAGE_BYTES == table.numel()
