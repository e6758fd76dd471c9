"""What tests/test_resample_adjoint_cpu.py and tests/test_gpu_resample_adjoint.py share: the case tables of the adjoints of the
resample + combine steps (csrc/unet_resample_train.hip under training.DownCombineFn / UpCombineFn), a numpy restatement of
both adjoints, and the references.

The reference of a case is torch autograd of the torch modules (diffusion.Downsample + CombinerDown, CombinerUp + Upsample) on the
CPU in float64.  The bound is derived, not measured: every output is a sum of products of the operands, so ANY float32 evaluation
order satisfies, elementwise, |got - ref64| <= N 2^-24 A, where A is the same forward + backward in float64 with every operand
replaced by its absolute value and N counts the roundings on the longest path:
    N_down = taps + C + ceil(taps / S) + 8      (pyr_d: taps; the combiner: C; the gather: ceil(taps / S); scalings, the rounding of
                                                 the partials and of their sum, the float32 1 / sqrt 2: 8)
    N_up   = C + taps S + 8
Where A is 0 the result must equal the reference.  A wrong tap, phase or edge misses the bound by orders of magnitude."""
import functools
import math

import numpy as np
import torch

from ntm_amd import diffusion

# ---- the constants behind the frame edges, each the mirror of one line of csrc/unet_resample_train.hip
R_TILE = 256        # `constexpr int kRTile = 256`: frames of a workgroup, one per thread; the up adjoint's partials per stream
R_SEG = 32          # `constexpr int kRSeg = 32`: frames a thread adds for the up adjoint's combiner weight
R_STAGE = 336       # `constexpr int kRStage = kRTile + 64 + 16`: g_pd values a tile of the down adjoint may stage (taps <= 64)
MAX_TAPS, MAX_C = 64, 32        # ntm_api.hip unet_resample_check
B = 2
U = 2.0 ** -24


def filter_of(kind, S):
    """The module's own filter bank and width: down (1, 1, 2 w + S), up (S, 1, 2 w + 1); up with S = 1: (None, 0)."""
    if kind == "up" and S == 1:
        return None, 0
    return diffusion.sinc_resample_kernel(S, 1) if kind == "down" else diffusion.sinc_resample_kernel(1, S)


def taps_of(kind, S):
    k, _ = filter_of(kind, S)
    return 0 if k is None else k.shape[-1]


def n_roundings(kind, S, C):
    taps = taps_of(kind, S)
    return taps + C + -(-taps // S) + 8 if kind == "down" else C + taps * S + 8


def _frames(kind, S):
    _, w = filter_of(kind, S)
    taps = taps_of(kind, S)
    fs = {1, 2, S - 1, S + 1, 4 * S - 1, 4 * S + 1, w - 1, taps, taps + 1, 1000}
    for edge in (R_TILE, R_SEG):
        fs |= {edge - 1, edge, edge + 1}
    fs |= {2 * R_TILE + 1}                         # a third tile with one frame
    return sorted(f for f in fs if f >= 1)


def _table():
    """name -> dict(kind, S, F, C, extra): extra None = no pyramid (up only), else pyr_T = F + extra.  Every frame edge at
    C = 5; C = 1 and 16 on the edges of the tile; the pyramid forms in turn."""
    cases = {}
    for kind, Ss in (("down", (2, 4, 3)), ("up", (2, 4, 3, 1))):
        for S in Ss:
            for n, Fr in enumerate(_frames(kind, S)):
                Cs = (1, 5, 16) if Fr in (1, S + 1, R_TILE - 1, R_TILE + 1, 1000) else (5,)
                for C in Cs:
                    extra = 0 if kind == "down" else (None, 0, 3)[(n + C) % 3]
                    cases[f"{kind} S={S} F={Fr} C={C} pyr={extra}"] = dict(kind=kind, S=S, F=Fr, C=C, extra=extra)
            if kind == "up":                       # every pyramid form at one multi-tile and one tiny shape
                for Fr in (3, R_TILE + 1):
                    for extra in (None, 0, 3):
                        cases[f"{kind} S={S} F={Fr} C=5 pyr={extra}"] = dict(kind=kind, S=S, F=Fr, C=5, extra=extra)
    return cases


CASES = _table()
LONG = {"down long": dict(kind="down", S=4, F=65536, C=16, extra=0, B=1),
        "up long": dict(kind="up", S=4, F=65536, C=16, extra=0, B=1)}
GRADS = ("both", "xo", "po")                       # which upstream gradients are there


def operands(case, seed=0):
    """Float32 operands of one case on the CPU: x, pyr (or None), ker (or None), wc, g_xo (or None: S = 1), g_po, width."""
    kind, S, Fr, C, extra = (case[k] for k in ("kind", "S", "F", "C", "extra"))
    Bn = case.get("B", B)
    g = torch.Generator().manual_seed(7000 + 131 * seed + 17 * S + Fr + 1000 * C)
    ker, w = filter_of(kind, S)
    Fo = -(-Fr // S) if kind == "down" else S * Fr
    op = {"x": torch.randn(Bn, C, Fr, generator=g),
          "pyr": None if extra is None else torch.randn(Bn, 1, Fr + extra, generator=g),
          "ker": ker, "wc": torch.randn((C, 1, 1) if kind == "down" else (1, C, 1), generator=g) / math.sqrt(C),
          "g_xo": None if kind == "up" and S == 1 else torch.randn(Bn, C, Fo, generator=g),
          "g_po": torch.randn(Bn, 1, Fo, generator=g)}
    return op, w


def integer_operands(case, seed=0):
    """The same operands as small integers, the filter among them (the functions take `kernel`): every product and sum of the
    adjoint is then exact in float32 wherever no 1 / sqrt 2 enters."""
    op, w = operands(case, seed)
    g = torch.Generator().manual_seed(9000 + seed + case["F"])
    ints = lambda t, hi: None if t is None else torch.randint(-hi, hi + 1, t.shape, generator=g).float()      # noqa: E731
    return {"x": ints(op["x"], 3), "pyr": ints(op["pyr"], 3), "ker": ints(op["ker"], 2), "wc": ints(op["wc"], 2),
            "g_xo": ints(op["g_xo"], 3), "g_po": ints(op["g_po"], 3)}, w


# the exact cases: no 1 / sqrt 2 enters up_combine without a pyramid (g_x, g_wc), nor down_combine's g_pyr with g_xo absent
EXACT = {f"{kind} S={S} F={Fr}": dict(kind=kind, S=S, F=Fr, C=5, extra=None if kind == "up" else 0)
         for kind, S in (("up", 2), ("up", 1), ("down", 2)) for Fr in (R_TILE - 1, R_TILE + 1)}


def torch_step(case, op, w, dt, grads="both", absolute=False, dev="cpu"):
    """The torch modules under autograd -> dict(xo, po, g_x, g_pyr, g_wc) (absent ones None), in dt on dev."""
    kind, S = case["kind"], case["S"]
    prep = lambda t: None if t is None else (t.abs() if absolute else t).detach().to(dev, dt).clone()      # noqa: E731
    t = {k: prep(v) for k, v in op.items()}
    for k in ("x", "pyr", "wc"):
        if t[k] is not None:
            t[k].requires_grad_(True)
    C = t["x"].shape[1]
    if kind == "down":
        res, comb = diffusion.Downsample(S), diffusion.CombinerDown(1, C)
        res.resample.kernel = t["ker"]
        comb.conv1x1.weight = torch.nn.Parameter(t["wc"])
        xd, po = res(t["x"]), res(t["pyr"])
        xo = comb(po, xd)
    else:
        comb = diffusion.CombinerUp(1, C)
        comb.conv1x1.weight = torch.nn.Parameter(t["wc"])
        p = comb(t["pyr"], t["x"])
        if S == 1:
            xo, po = None, p
        else:
            res = diffusion.Upsample(S)
            res.resample.kernel = t["ker"]
            xo, po = res(t["x"]), res(p)
    loss = 0
    if grads in ("both", "xo") and xo is not None:
        loss = loss + (xo * t["g_xo"]).sum()
    if grads in ("both", "po"):
        loss = loss + (po * t["g_po"]).sum()
    loss.backward()
    # an operand the present gradients do not reach has no .grad: its gradient is zero
    grad = lambda v: None if v is None else (torch.zeros_like(v) if v.grad is None else v.grad)      # noqa: E731
    return {"xo": None if xo is None else xo.detach(), "po": po.detach(), "g_x": grad(t["x"]), "g_pyr": grad(t["pyr"]),
            "g_wc": grad(comb.conv1x1.weight)}


@functools.lru_cache(None)
def reference(name, grads="both"):
    """-> (ref64, A) of a case of CASES or LONG, each a dict of float64 numpy arrays (g_x, g_pyr | None, g_wc)."""
    case = CASES.get(name) or LONG[name]
    op, w = operands(case)
    keep = lambda r: {k: None if r[k] is None else r[k].numpy() for k in ("g_x", "g_pyr", "g_wc")}      # noqa: E731
    return (keep(torch_step(case, op, w, torch.float64, grads)), keep(torch_step(case, op, w, torch.float64, grads, absolute=True)))


def variants(case):
    """The upstream-gradient variants a case has: the S = 1 form has no g_xo."""
    return ("both",) if case["kind"] == "up" and case["S"] == 1 else GRADS


def fraction(got, ref64, A, N):
    """max |got - ref64| / (N 2^-24 A) where A > 0; where A == 0 the result must equal the reference."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    got = got.astype(np.float64)
    assert got.shape == ref64.shape == A.shape, (got.shape, ref64.shape, A.shape)
    zero = A == 0
    assert np.array_equal(got[zero], ref64[zero]), "where every term is zero the result must equal the reference"
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got - ref64)[~zero] / (N * U * A[~zero])))


# ---- the adjoints restated in numpy, in the dtype of their operands (float64, or int64 for the exact cases) -------------------------

def down_adjoint(ker, wc, pd, g_xo, g_po, Fr, S, w):
    """ker [taps], wc [C], pd [B][Fo] (the forward's second output), g_xo [B][C][Fo] | None, g_po [B][Fo] | None
    -> g_x [B][C][F], g_pyr [B][F], g_wc [C].  1 / sqrt 2 enters only through g_xo."""
    Fo, taps = -(-Fr // S), len(ker)
    r2 = 1 / math.sqrt(2)

    def gather(g):
        out = np.zeros(g.shape[:-1] + (Fr,), g.dtype)
        j = np.arange(Fo)
        for i in range(taps):
            f = j * S - w + i
            ok = (f >= 0) & (f < Fr)
            out[..., f[ok]] += ker[i] * g[..., j[ok]]
        return out

    Bn = (g_xo if g_xo is not None else g_po).shape[0]
    if g_xo is None:
        return np.zeros((Bn, len(wc), Fr), g_po.dtype), gather(g_po), np.zeros(len(wc), g_po.dtype)
    g_pd = np.einsum("c,bcj->bj", wc, g_xo) * r2
    if g_po is not None:
        g_pd = g_pd + g_po
    return gather(g_xo) * r2, gather(g_pd), np.einsum("bcj,bj->c", g_xo, pd) * r2


def up_adjoint(x, ker, wc, g_xo, g_po, S, w, pyr_T):
    """x [B][C][F], ker [S][taps] | None, wc [C], g_xo [B][C][S F] | None, g_po [B][S F] | None, pyr_T 0 = no pyramid
    -> g_x [B][C][F], g_pyr [B][pyr_T] | None, g_wc [C].  1 / sqrt 2 enters only with a pyramid."""
    Bn, C, Fr = x.shape

    def gather(g):
        if ker is None:
            return g.copy()
        out = np.zeros(g.shape[:-1] + (Fr,), g.dtype)
        f = np.arange(Fr)
        for ph in range(S):
            for i in range(ker.shape[1]):
                j = f - i + w
                ok = (j >= 0) & (j < Fr)
                out[..., f[ok]] += ker[ph, i] * g[..., j[ok] * S + ph]
        return out

    g_p = np.zeros((Bn, Fr), x.dtype) if g_po is None else gather(g_po)
    if pyr_T:
        g_p = g_p * (1 / math.sqrt(2))
    g_x = wc[None, :, None] * g_p[:, None, :]
    if g_xo is not None:
        g_x = g_x + gather(g_xo)
    g_pyr = None
    if pyr_T:
        g_pyr = np.zeros((Bn, pyr_T), g_p.dtype)
        g_pyr[:, :Fr] = g_p
    return g_x, g_pyr, np.einsum("bf,bcf->c", g_p, x)


def numpy_step(case, op, w, grads="both", dtype=np.float64):
    """The numpy adjoints on a case's operands -> dict(g_x, g_pyr | None, g_wc) shaped like torch_step's.  The forward value the
    down adjoint needs (pyr_d) comes from the float64 torch forward."""
    a = {k: None if v is None else v.numpy().astype(dtype) for k, v in op.items()}
    g_xo = a["g_xo"] if grads in ("both", "xo") else None
    g_po = a["g_po"][:, 0] if grads in ("both", "po") else None
    if case["kind"] == "down":
        pd = torch_step(case, op, w, torch.float64, "po")["po"].numpy()[:, 0].astype(dtype)
        g_x, g_pyr, g_wc = down_adjoint(a["ker"][0, 0], a["wc"][:, 0, 0], pd, g_xo, g_po, case["F"], case["S"], w)
        return {"g_x": g_x, "g_pyr": g_pyr[:, None], "g_wc": g_wc[:, None, None]}
    ker = None if a["ker"] is None else a["ker"][:, 0]
    pyr_T = 0 if a["pyr"] is None else a["pyr"].shape[-1]
    g_x, g_pyr, g_wc = up_adjoint(a["x"], ker, a["wc"][0, :, 0], g_xo, g_po, case["S"], w, pyr_T)
    return {"g_x": g_x, "g_pyr": None if g_pyr is None else g_pyr[:, None], "g_wc": g_wc[None, :, None]}
