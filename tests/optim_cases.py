"""What tests/test_optim_cpu.py and tests/test_gpu_optim.py share: the cases of the fused optimiser step (ntm_amd.optim), their
references and the bar.

The reference of a case is torch's own machinery on the CPU from the same float32 inputs: torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam(foreach=False), and the reference's EMA expression dst * s + src * (1 - s), in float64 (ref64) and in float32
(ref32).  The bar of a quantity is diffusion_train_cases.bar_of: 3 x max|ref32 - ref64| / max|ref64|, taken over the
CONCATENATION of all tensors of the case, so that a one-element tensor cannot produce a zero bar -- computed from the two
references, never from the HIP result.  The quantities: the update p_new - p_old (formed in float64 from the values, so that
the rounding of p does not hide a wrong formula where p = 0), exp_avg, exp_avg_sq, the clipped gradients of the last step, the
returned norms of all steps, and the EMA update dst_new - dst_old.  Two kinds of quantity have no error to take a bar from and
are held exactly instead: a reference that is identically zero (lr = 0: the parameters keep their bits), and gradients that
no active clip scales (they keep their bits)."""
import functools
from fractions import Fraction

import numpy as np
import torch

from ntm_amd import _lib, diffusion
from diffusion_train_cases import bar_of, rel_err

CHUNK, MAX = _lib.MULTI_CHUNK, _lib.MULTI_MAX_TENSORS
ELEMENT_COUNTS = (1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
TENSOR_COUNTS = (1, 2, MAX - 1, MAX, MAX + 1, 2 * MAX + 1)
CLIPS = {"active": 0.25, "inactive": 1e6, "absent": None}
COMPANION = 1021        # odd, below a chunk: a second tensor with a scalar tail of its own
QUANTITIES = ("update", "exp_avg", "exp_avg_sq", "grad", "norm")


@functools.lru_cache(None)
def reference_hyper():
    """The reference's Adam: lr 2e-4, betas (0.9, 0.999), eps 1e-8 (the toytrajectories configuration)."""
    t = diffusion.load_config("toytrajectories").train
    return {"lr": t.lr, "betas": (t.optimizer.beta1, t.optimizer.beta2), "eps": t.optimizer.eps}


def small_sizes(count):
    """`count` tensors of 1 - 7 elements; the first has 7, so that a list of one still has a norm that rounds."""
    return tuple(7 - k % 7 for k in range(count))


class Case:
    """sizes: elements per tensor.  p0: the float32 parameters.  grads[step][k]: a float32 gradient or None.  groups: a list of
    (indices, hyper-parameters); lrs: an lr for every step (all groups) or None.  clip: a key of CLIPS."""

    def __init__(self, sizes, seed, steps=3, zero_p=False, clip="absent", none_at=(), groups=None, lrs=None):
        g = torch.Generator().manual_seed(seed)
        self.sizes, self.clip, self.max_norm, self.lrs = tuple(sizes), clip, CLIPS[clip], lrs
        self.p0 = [torch.zeros(n) if zero_p else torch.randn(n, generator=g) for n in sizes]
        self.grads = [[None if k in none_at else torch.randn(n, generator=g) * (0.1 + 3 * torch.rand(1, generator=g))
                       for k, n in enumerate(sizes)] for _ in range(steps)]
        self.groups = groups or [(list(range(len(sizes))), reference_hyper())]

    def live(self):
        return [k for k in range(len(self.sizes)) if self.grads[0][k] is not None]


def _cat(ts):
    return np.concatenate([t.detach().double().cpu().numpy().ravel() for t in ts]) if ts else np.zeros(0)


def collect(case, ps, opt, norms):
    """The quantities of a finished run, each one float64 vector over all tensors of the case."""
    live = case.live()
    return {"update": _cat([ps[k].detach().double().cpu() - case.p0[k].double() for k in range(len(ps))]),
            "exp_avg": _cat([opt.state[ps[k]]["exp_avg"] for k in live]),
            "exp_avg_sq": _cat([opt.state[ps[k]]["exp_avg_sq"] for k in live]),
            "grad": _cat([ps[k].grad for k in live]),
            "norm": np.asarray([float(v) for v in norms], np.float64),
            "steps": [float(opt.state[ps[k]]["step"]) for k in live],
            "stateless": [k for k in range(len(ps)) if len(opt.state[ps[k]]) == 0 and k not in live]}


def run(case, make_opt, dtype=torch.float32, device="cpu", fused=False, params=None):
    """The case's steps with the optimiser make_opt(param groups) -> the quantities.  fused: the optimiser clips inside step();
    else torch's clip_grad_norm_ goes first.  params: the float32 parameters to step in place of fresh copies of p0."""
    ps = params or [torch.nn.Parameter(p.to(device, dtype).clone()) for p in case.p0]
    opt = make_opt([{"params": [ps[k] for k in idx], **hyper} for idx, hyper in case.groups])
    norms = []
    for i, gs in enumerate(case.grads):
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(device, dtype).clone()
        if case.lrs is not None:
            for grp in opt.param_groups:
                grp["lr"] = case.lrs[i]
        if fused:
            n = opt.step(max_grad_norm=case.max_norm)
            assert (n is None) == (case.max_norm is None)
        else:
            n = None if case.max_norm is None else torch.nn.utils.clip_grad_norm_(ps, case.max_norm, foreach=False)
            opt.step()
        if n is not None:
            norms.append(n)
    return collect(case, ps, opt, norms)


def torch_adam(groups):
    return torch.optim.Adam(groups, foreach=False)


@functools.lru_cache(None)
def references(case):
    """-> (ref32, ref64) of a case, computed once."""
    r32, r64 = run(case, torch_adam, torch.float32), run(case, torch_adam, torch.float64)
    if case.clip == "active":
        assert np.all(r64["norm"] > case.max_norm), "the case's clip is not active"
    if case.clip == "inactive":
        assert np.all(r64["norm"] < case.max_norm), "the case's clip is active"
    return r32, r64


def hold(what, got, ref32, ref64):
    """Print the figure, then hold it against the bar (which must be positive).  A reference that is identically zero asks for
    exact zeros."""
    got, ref32, ref64 = (np.asarray(v, np.float64) for v in (got, ref32, ref64))
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    if not np.any(ref64):
        print(f"{what}: the reference is identically zero")
        assert not np.any(got), what
        return
    e, b = rel_err(got, ref64), bar_of(ref32, ref64)
    print(f"{what}: error {e:.3e}, bar {b:.3e}, ratio to torch's own float32 error {3 * e / b if b else float('inf'):.2f}")
    assert b > 0, (what, "the two references agree to the bit: no bar")
    assert e <= b, (what, e, b)


def hold_case(name, case, got):
    """Every quantity of a fused run against the case's references."""
    r32, r64 = references(case)
    assert got["steps"] == r64["steps"] and got["stateless"] == r64["stateless"], name
    for q in QUANTITIES:
        if q == "norm" and case.max_norm is None:
            assert got[q].size == 0
        elif q == "grad" and case.clip != "active":
            assert np.array_equal(got[q], r64[q]), (name, "gradients that nothing scales must keep their bits")
        else:
            hold(f"{name} {q}", got[q], r32[q], r64[q])


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def element_case(n, i):
    """One tensor of n elements beside one of COMPANION; the clip and p = 0 rotate.  Why the companion: the bar is a sample
    maximum of torch's float32 rounding errors.  Over a handful of elements that maximum is a lottery -- torch's CPU kernels
    contract a multiply-add here and there (addcmul, lerp), the HIP kernel by its specification never does, so the two carry
    different roundings and over nine elements either may come out several times luckier than the other (a one-element list
    even has a norm that does not round at all).  Over a thousand elements both maxima sit near their worst case, k roundings
    of 2^-24 each with k within a factor 1.5 of each other, and the factor 3 of the bar has its meaning."""
    return Case((n, COMPANION), seed=100 + i, zero_p=i % 2 == 1, clip=list(CLIPS)[i % 3])


@functools.lru_cache(None)
def count_case(c, i):
    return Case(small_sizes(c), seed=200 + i, zero_p=i % 2 == 0, clip=list(CLIPS)[(i + 1) % 3])


@functools.lru_cache(None)
def mixed_case(clip="active", zero_p=False):
    """Both kinds in one list of more than two tables: a .grad = None in the middle, a zero-element parameter, two groups."""
    sizes = small_sizes(MAX - 3) + (CHUNK + 1, 0, 3) + small_sizes(MAX + 2) + (2 * CHUNK + 3, 257, 1)
    half = len(sizes) // 2
    groups = [(list(range(half)), reference_hyper()),
              (list(range(half, len(sizes))), {"lr": 3e-3, "betas": (0.8, 0.95), "eps": 1e-6})]
    return Case(sizes, seed=300, zero_p=zero_p, clip=clip, none_at=(MAX - 5, half + 2), groups=groups)


@functools.lru_cache(None)
def ramp_case():
    """lr = 0 at the first step, as in the first iteration of the reference's ramp: one step."""
    return Case((5, CHUNK + 1, 3), seed=400, steps=1, clip="active", lrs=(0.0,))


# ---- the exact cases ------------------------------------------------------------------------------------------------------------------

EXACT_HYPER = {"lr": 2.0 ** -4, "betas": (0.5, 0.75), "eps": 1.0}
EXACT_MAX_NORM = 64.0
EXACT_SIZES = (1, 4, 5, 33, 27)


@functools.lru_cache(None)
def exact_case():
    """beta = (0.5, 0.75), eps = 1, lr = 2^-4, zero state, first step, gradients in {0, +-1, +-3, +-7}, dyadic parameters and a
    clip above the norm (coef exactly 1): m' = g / 2, v' = g^2 / 4, p' = p - g / (16 (|g| + 1)), all exact in float32.
    -> (p0, g, expected p, m, v as float32 tensors from fractions.Fraction, the norm as float32)."""
    gen = torch.Generator().manual_seed(500)
    vals = torch.tensor([0.0, 1.0, -1.0, 3.0, -3.0, 7.0, -7.0])
    p0 = [torch.randint(-64, 65, (n,), generator=gen).float() / 8 for n in EXACT_SIZES]
    g = [vals[torch.randint(0, 7, (n,), generator=gen)] for n in EXACT_SIZES]
    want = {"p": [], "m": [], "v": []}
    for p, q in zip(p0, g):
        fp, fg = [Fraction(float(x)) for x in p], [Fraction(float(x)) for x in q]
        for key, fr in (("p", [a - b / (16 * (abs(b) + 1)) for a, b in zip(fp, fg)]), ("m", [b / 2 for b in fg]),
                        ("v", [b * b / 4 for b in fg])):
            t = torch.tensor([float(f) for f in fr], dtype=torch.float32)
            assert [Fraction(float(x)) for x in t] == fr, "the expectation is not exact in float32"
            want[key].append(t)
    sq = sum(int(x) ** 2 for q in g for x in q)
    assert 0 < sq < EXACT_MAX_NORM ** 2
    return p0, g, want["p"], want["m"], want["v"], np.float32(np.sqrt(np.float64(sq)))


def exact_run(make_opt, device="cpu", fused=False):
    """The exact case's one step -> (p, exp_avg, exp_avg_sq, grads as lists of CPU tensors, the norm as a float)."""
    p0, g = exact_case()[:2]
    ps = [torch.nn.Parameter(p.to(device).clone()) for p in p0]
    opt = make_opt([{"params": ps, **EXACT_HYPER}])
    for p, q in zip(ps, g):
        p.grad = q.to(device).clone()
    if fused:
        norm = opt.step(max_grad_norm=EXACT_MAX_NORM)
    else:
        norm = torch.nn.utils.clip_grad_norm_(ps, EXACT_MAX_NORM, foreach=False)
        opt.step()
    return ([p.detach().cpu() for p in ps], [opt.state[p]["exp_avg"].cpu() for p in ps],
            [opt.state[p]["exp_avg_sq"].cpu() for p in ps], [p.grad.cpu() for p in ps], float(norm))


def assert_exact(got):
    p0, g, wp, wm, wv, wnorm = exact_case()
    p, m, v, gg, norm = got
    for k in range(len(p0)):
        assert torch.equal(p[k], wp[k]) and torch.equal(m[k], wm[k]) and torch.equal(v[k], wv[k]) and torch.equal(gg[k], g[k]), k
    assert np.float32(norm) == wnorm, (norm, wnorm)


@functools.lru_cache(None)
def ema_exact_case():
    """s = 0.5 and dyadic values: dst' = (dst + src) / 2 exactly."""
    gen = torch.Generator().manual_seed(600)
    sizes = (1, 5, 256, CHUNK + 1)
    dst = [torch.randint(-512, 513, (n,), generator=gen).float() / 16 for n in sizes]
    src = [torch.randint(-512, 513, (n,), generator=gen).float() / 16 for n in sizes]
    return dst, src, [(a.double() + b.double()).div(2).float() for a, b in zip(dst, src)]


@functools.lru_cache(None)
def ema_case(sizes, s, seed):
    """-> (dst, src, ref32 update, ref64 update): the reference's expression on the CPU in both precisions."""
    gen = torch.Generator().manual_seed(seed)
    dst, src = ([torch.randn(n, generator=gen) for n in sizes] for _ in range(2))
    ups = []
    for dt in (torch.float32, torch.float64):
        ups.append(_cat([(d.to(dt) * s + q.to(dt) * (1 - s)).double() - d.double() for d, q in zip(dst, src)]))
    return dst, src, ups[0], ups[1]
