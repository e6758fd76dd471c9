#!/usr/bin/env python3
"""High-precision references for the fp64 arithmetic of the tape simulator's Jiles-Atherton stage (csrc/tape_math.h,
tape_hmag_kernel): mpmath at 50 digits, rounded to fp64 -- CPU only, dev-only like the other tools/make_goldens_*.py.
The fp64 CPU oracle of the tests follows the reference operation for operation, including the ill-conditioned closed
form of L', and is itself 1e-10 off on unsaturated input; the tests of tests/test_gpu_tape.py therefore measure the
device AND the oracle against these values (E_gpu <= max(4 E_ref, floor)).

Three parts, all from fixed seeds:
  * helper points: the argument ranges of rcp_nr, expm1_neg, coth_gt and langevin_prime_lt1, log-spaced plus the edges
    (range ends, multiples of ln2/2 +- 1 ulp, powers of two and their neighbours), with E_ref of the library function;
  * ja_f points (Mn, Hn, Hp) in classes by |Q| (both sides of the 1e-4 switches of L and L', up to 1e4) with the exact
    cases Hp = 0 and Mn = Hn = 0.  Points at which the value itself is ill-conditioned (M_diff, the denominator of the
    irreversible term or the final sum cancel to less than COND of their operands) are not drawn: there any error of
    L(Q) is amplified alike for every implementation and the comparison says nothing.  A point where mpmath and plain
    fp64 disagree on one of the four selectors (|Q| > 1e-4, |L(Q)| > 1e-4, sign of M_diff, sign of Hp) is marked
    ja_keep = 0 (at most 1 %);
  * trajectory families, 4 streams x 300 samples at Ts = 1 / (48000 * 16) from zero state, with the state after 150 and
    300 samples and the share of samples clamped to +-Ms.
Output: tests/golden/g25_tape_mp.npz (tests/test_oracle_tape.py regenerates a subset where mpmath imports)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g25_tape_mp.npz")

DPS = 50
SEED = 2025
PARAMS = (1.6e6, 1.1e3, 1.6e-3, 4.0e2, 1.7e-1)          # Ms, A, alpha, K, c (code/tape.py:251-256)
TS = 1.0 / (48000 * 16)
TRAJ_B, TRAJ_N, TRAJ_MID = 4, 300, 150
FAMILIES = ("sin001", "sin100", "sin1000", "walk_small", "chain", "step", "const", "zeros", "sat")
UNSATURATED = FAMILIES[:4]                                 # clamped share 0, asserted on the mpmath result
HELPERS = ("rcp_nr", "expm1_neg", "coth_gt", "langevin_prime_lt1")
LP_BINS = (1e-4, 1e-3, 1e-2, 1e-1, 0.5, 1.0)              # langevin_prime_lt1 is judged per bin of |x|: the closed form's
#                                                           error falls from 1e-8 at 1e-4 to 1e-16 at 1
JA_CLASSES = ("q_tiny", "q_edge", "lq_edge", "lq_small", "mid", "large", "hp_zero", "origin")
JA_PER_CLASS = 450
COND = 0.05
SWITCH = 1e-4


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


# ------------------------------------------------------------------------------------------------- helper points
def _logspace_pm(lo, hi, n):
    x = np.exp(np.linspace(np.log(lo), np.log(hi), n))
    x[0], x[-1] = lo, hi
    return np.concatenate([x, -x])


def helper_points():
    """name -> fp64 arguments (no mpmath needed: the GPU case tables are checked from these on the CPU)."""
    up = lambda v: np.nextafter(v, np.inf)          # noqa: E731
    dn = lambda v: np.nextafter(v, -np.inf)         # noqa: E731
    pts = {}
    p2 = 2.0 ** np.arange(-330, 331, 11)
    pts["rcp_nr"] = np.concatenate([_logspace_pm(1e-100, 1e100, 900), p2, up(p2), dn(p2), -p2, -up(p2), -dn(p2)])
    half = np.log(2.0) / 2 * np.concatenate([np.arange(1, 41), [101, 1000, 2047, 2048, 2049, 2300]])
    pts["expm1_neg"] = np.concatenate([-_logspace_pm(2e-4, 800.0, 2400)[:2400], -half, -up(half), -dn(half), [-1e4, -1e7]])
    pts["coth_gt"] = _logspace_pm(up(SWITCH), 50.0, 1300)
    near1 = 1.0 - np.exp(np.linspace(np.log(1e-6), np.log(0.5), 300))
    pts["langevin_prime_lt1"] = np.concatenate([_logspace_pm(up(SWITCH), 0.999999, 1200), near1, -near1])
    return pts


def mp_helper(name, x):
    mp = _mp()
    f = {"rcp_nr": lambda v: 1 / v, "expm1_neg": mp.expm1, "coth_gt": mp.coth,
         "langevin_prime_lt1": lambda v: 1 / v ** 2 - mp.coth(v) ** 2 + 1}[name]
    return np.array([float(f(mp.mpf(float(v)))) for v in x])


def lib_helper(name, x):
    """The library function in fp64 that the hand-written helper replaces (for L': the oracle's closed form)."""
    x = np.asarray(x, np.float64)
    if name == "rcp_nr":
        return 1.0 / x
    if name == "expm1_neg":
        return np.expm1(x)
    if name == "coth_gt":
        return 1.0 / np.tanh(x)
    ct = 1.0 / np.tanh(x)
    return 1.0 / (x * x) - ct * ct + 1.0


def rel_err(got, want):
    """|got - want| / |want| per element; where want is 0, 0 if got is 0 too and inf otherwise."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(got - want) / np.abs(want)
    return np.where(got == want, 0.0, np.where(want == 0, np.inf, e))


def lp_bin(x):
    """Index into LP_BINS' intervals (lo, hi] of |x|."""
    return np.searchsorted(np.asarray(LP_BINS), np.abs(x), side="left") - 1


# ------------------------------------------------------------------------------------------------- ja_f
def mp_ja_f(Mn, Hn, Hp, par=PARAMS, detail=False):
    """Tape._f (code/tape.py:587-635) in mpmath: the reference's formulas and switches."""
    mp = _mp()
    Ms, A, alpha, K, c = (mp.mpf(v) for v in par)
    Mn, Hn, Hp = mp.mpf(Mn), mp.mpf(Hn), mp.mpf(Hp)
    Q = (Hn + alpha * Mn) / A
    sq = abs(Q) > mp.mpf(SWITCH)
    LQ = mp.coth(Q) - 1 / Q if sq else Q / 3
    sl = abs(LQ) > mp.mpf(SWITCH)
    LpQ = 1 / (LQ * LQ) - mp.coth(LQ) ** 2 + 1 if sl else mp.mpf(1) / 3
    M_diff = Ms * LQ - Mn
    dS = 1 if Hp > 0 else -1
    sgn = (M_diff > 0) - (M_diff < 0)
    dM = 1 if dS == sgn else 0
    t1d = (1 - c) * dS * K - alpha * M_diff
    t1 = ((1 - c) * dM * M_diff / t1d) * Hp
    t2 = c * (Ms / A) * Hp * LpQ
    t3 = 1 - c * alpha * (Ms / A) * LpQ
    f = (t1 + t2) / t3
    if not detail:
        return f
    ok = (M_diff == 0 or abs(M_diff) >= COND * max(abs(Ms * LQ), abs(Mn))) and abs(t1d) >= COND * (1 - c) * K and \
        ((t1 == 0 and t2 == 0) or abs(t1 + t2) >= COND * max(abs(t1), abs(t2)))
    return f, (int(sq), int(sl), int(sgn), dS), bool(ok)


def fp64_selectors(pts, par=PARAMS):
    """The four selectors as plain fp64 evaluates them, in the oracle's operation order -> int8 [n,4]."""
    import math
    Ms, A, alpha, _, _ = par
    out = np.empty((len(pts), 4), np.int8)
    for i, (Mn, Hn, Hp) in enumerate(np.asarray(pts, np.float64).tolist()):
        Q = (Hn + alpha * Mn) / A
        sq = abs(Q) > SWITCH
        LQ = (1.0 / math.tanh(Q)) - 1.0 / Q if sq else Q / 3.0
        Md = Ms * LQ - Mn
        out[i] = (sq, abs(LQ) > SWITCH, (Md > 0) - (Md < 0), 1 if Hp > 0.0 else -1)
    return out


def fp64_ja_f(Mn, Hn, Hp, par=PARAMS):
    """Tape._f in plain fp64 (Python floats, libm's tanh), operation for operation as the reference and the CPU oracle
    evaluate it: the E_ref side of the fixture (tests/test_oracle_tape.py holds the oracle to these bits)."""
    import math
    Ms, A, alpha, K, c = par
    Q = (Hn + alpha * Mn) / A
    LQ = (1.0 / math.tanh(Q)) - 1.0 / Q if abs(Q) > SWITCH else Q / 3.0
    if abs(LQ) > SWITCH:
        ct = 1.0 / math.tanh(LQ)
        LpQ = 1.0 / (LQ * LQ) - ct * ct + 1.0
    else:
        LpQ = 1.0 / 3.0
    M_diff = Ms * LQ - Mn
    dS = 1.0 if Hp > 0.0 else -1.0
    sgn = 1.0 if M_diff > 0.0 else (-1.0 if M_diff < 0.0 else 0.0)
    dM = 1.0 if dS == sgn else 0.0
    t1n = (1.0 - c) * dM * M_diff
    t1d = (1.0 - c) * dS * K - alpha * M_diff
    t1 = (t1n / t1d) * Hp
    t2 = c * (Ms / A) * Hp * LpQ
    t3 = 1.0 - c * alpha * (Ms / A) * LpQ
    return (t1 + t2) / t3


def fp64_hmag(H, Ts=TS, par=PARAMS):
    """Tape.H_mag in plain fp64 from zero state (see fp64_ja_f) -> M [B,N]."""
    M = np.empty_like(H)
    for b, row in enumerate(np.asarray(H, np.float64).tolist()):
        Mp = Hpv = Hpp = 0.0
        for n, Hn in enumerate(row):
            Hprime = 2.0 * (Hn - Hpv) / Ts - Hpp
            k1 = Ts * fp64_ja_f(Mp, Hpv, Hpp, par)
            k2 = Ts * fp64_ja_f(Mp + k1 / 2.0, (Hn + Hpv) / 2.0, (Hprime + Hpp) / 2.0, par)
            k3 = Ts * fp64_ja_f(Mp + k2 / 2.0, (Hn + Hpv) / 2.0, (Hprime + Hpp) / 2.0, par)
            k4 = Ts * fp64_ja_f(Mp + k3, Hn, Hprime, par)
            m = Mp + k1 / 6.0 + k2 / 3.0 + k3 / 3.0 + k4 / 6.0
            m = -par[0] if m < -par[0] else (par[0] if m > par[0] else m)
            M[b, n] = m
            Hpv, Hpp, Mp = Hn, Hprime, m
    return M


_Q_RANGE = {"q_tiny": (1e-8, 0.5e-4), "q_edge": (0.5e-4, 2e-4), "lq_edge": (1.5e-4, 6e-4), "lq_small": (6e-4, 1e-2),
            "mid": (1e-2, 30.0), "large": (30.0, 1e4), "hp_zero": (1e-3, 100.0)}


def ja_candidates(cls, n, rng):
    """n candidate points (Mn, Hn, Hp) of one class: |Q| log-uniform in the class's range (Hn is solved from Q and Mn in
    fp64, so the realised Q differs in the last places), Mn small beside Ms L(Q) where Q is small and anywhere in
    +-0.98 Ms otherwise, |Hp| log-uniform over 1e-2 .. 1e11 (dH/dt of an audio-rate field at 768 kHz reaches 1e10)."""
    Ms, A, alpha, _, _ = PARAMS
    sign = lambda: rng.choice([-1.0, 1.0], n)       # noqa: E731
    Hp = sign() * np.exp(rng.uniform(np.log(1e-2), np.log(1e11), n))
    if cls == "origin":
        return np.stack([np.zeros(n), np.zeros(n), Hp], 1)
    lo, hi = _Q_RANGE[cls]
    Q = sign() * np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    if cls in ("mid", "large", "hp_zero"):
        Mn = rng.uniform(-0.98 * Ms, 0.98 * Ms, n)
    else:
        Mn = sign() * np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    if cls == "hp_zero":
        Hp = np.zeros(n)
    return np.stack([Mn, Q * A - alpha * Mn, Hp], 1)


def ja_points(only=None):
    """-> (pts [n,3], class index [n], f [n] mpmath rounded, selectors by mpmath int8 [n,4]); classes in JA_CLASSES
    order, JA_PER_CLASS well-conditioned points each (ill-conditioned candidates are redrawn, see the module text)."""
    pts, cls_idx, fs, sels = [], [], [], []
    for ci, cls in enumerate(JA_CLASSES):
        if only is not None and cls not in only:
            continue
        rng = np.random.default_rng(SEED + 100 + ci)
        kept = 0
        while kept < JA_PER_CLASS:
            for p in ja_candidates(cls, JA_PER_CLASS, rng):
                f, sel, ok = mp_ja_f(*p.tolist(), detail=True)
                if ok and kept < JA_PER_CLASS:
                    pts.append(p), cls_idx.append(ci), fs.append(float(f)), sels.append(sel)
                    kept += 1
    return np.array(pts), np.array(cls_idx, np.int8), np.array(fs), np.array(sels, np.int8)


# ------------------------------------------------------------------------------------------------- trajectories
def family_inputs():
    """name -> H [TRAJ_B, TRAJ_N] fp64."""
    rng = np.random.default_rng(SEED)
    t = np.arange(TRAJ_N) * TS
    ph = np.array([0.0, 0.7, 1.9, 3.1])[:, None]
    # the sines start at 0 (a first sample away from 0 is a step, whose dH/dt alone saturates the 1000 A/m stream)
    s3k = np.array([1.0, -1.0, 0.75, -0.5])[:, None] * np.sin(2 * np.pi * 3000.0 * t[None, :])
    fam = {"sin001": 0.01 * s3k, "sin100": 100.0 * s3k, "sin1000": 1000.0 * s3k,
           "walk_small": 300.0 * np.cumsum(rng.standard_normal((TRAJ_B, TRAJ_N)), axis=1) / 20.0,
           "chain": 8333.0 * np.sin(2 * np.pi * 48e3 * t[None, :]) + 833.0 * np.sin(2 * np.pi * 1e3 * t[None, :] + ph)}
    step = np.zeros((TRAJ_B, TRAJ_N))
    step[0, 50:], step[1, 50:], step[2, 50:], step[3, 50:] = 5e4, -5e4, 5e2, -5e2
    fam["step"] = step
    fam["const"] = np.array([100.0, 1000.0, -1000.0, 8333.0])[:, None] * np.ones((1, TRAJ_N))
    fam["zeros"] = np.zeros((TRAJ_B, TRAJ_N))
    fam["sat"] = 3e6 * s3k
    return {k: np.ascontiguousarray(fam[k], dtype=np.float64) for k in FAMILIES}


def mp_hmag(H, Ts=TS, par=PARAMS, marks=(TRAJ_MID,)):
    """Tape.H_mag (code/tape.py:516-551) in mpmath from zero state, the state kept at full precision between samples
    -> (M [B,N] rounded to fp64, {n: state [B,3] after n samples (and after N)} rounded to fp64)."""
    mp = _mp()
    Ts_, Ms = mp.mpf(Ts), mp.mpf(par[0])
    B, N = H.shape
    M = np.empty((B, N))
    states = {n: np.empty((B, 3)) for n in tuple(marks) + (N,)}
    for b in range(B):
        Mp = Hpv = Hpp = mp.mpf(0)
        for n in range(N):
            Hn = mp.mpf(float(H[b, n]))
            Hprime = 2 * (Hn - Hpv) / Ts_ - Hpp
            k1 = Ts_ * mp_ja_f(Mp, Hpv, Hpp, par)
            k2 = Ts_ * mp_ja_f(Mp + k1 / 2, (Hn + Hpv) / 2, (Hprime + Hpp) / 2, par)
            k3 = Ts_ * mp_ja_f(Mp + k2 / 2, (Hn + Hpv) / 2, (Hprime + Hpp) / 2, par)
            k4 = Ts_ * mp_ja_f(Mp + k3, Hn, Hprime, par)
            m = Mp + k1 / 6 + k2 / 3 + k3 / 3 + k4 / 6
            m = -Ms if m < -Ms else (Ms if m > Ms else m)
            M[b, n] = float(m)
            Hpv, Hpp, Mp = Hn, Hprime, m
            if n + 1 in states:
                states[n + 1][b] = [float(Mp), float(Hpv), float(Hpp)]
    return M, states


def clamped_share(M, Ms=PARAMS[0]):
    """(share of samples equal to +Ms, share equal to -Ms)."""
    return float((M == Ms).mean()), float((M == -Ms).mean())


def g9_walk(rows=2, n=300):
    """The random-walk input of tests/test_gpu_parity.py::test_g9_tape_hmag (first rows / samples)."""
    return (8000.0 * np.cumsum(np.random.default_rng(0).standard_normal((70, 300)), axis=1) / 20.0)[:rows, :n]


def main():
    out = {"dps": DPS, "seed": SEED, "params": np.array(PARAMS), "Ts": TS, "cond": COND, "lp_bins": np.array(LP_BINS),
           "families": np.array(FAMILIES), "ja_classes": np.array(JA_CLASSES), "helpers": np.array(HELPERS)}
    for name, x in helper_points().items():
        want = mp_helper(name, x)
        e = rel_err(lib_helper(name, x), want)
        if name == "langevin_prime_lt1":
            b = lp_bin(x)
            eref = np.array([e[b == k].max() for k in range(len(LP_BINS) - 1)])
        else:
            eref = np.array([e.max()])
        out[f"h_{name}_x"], out[f"h_{name}_y"], out[f"h_{name}_eref"] = x, want, eref
        print(f"{name}: {len(x)} points, E_ref {eref}")
    pts, cls, f, sel = ja_points()
    keep = (fp64_selectors(pts) == sel).all(axis=1)
    e = rel_err(np.array([fp64_ja_f(*p) for p in pts.tolist()]), f)
    eref = np.array([e[(cls == k) & keep].max() for k in range(len(JA_CLASSES))])
    out.update(ja_pts=pts, ja_class=cls, ja_f=f, ja_sel=sel, ja_keep=keep.astype(np.int8), ja_eref=eref)
    print(f"ja_f: {len(pts)} points, left out {(~keep).sum()}, E_ref per class {dict(zip(JA_CLASSES, eref))}")
    assert (~keep).mean() <= 0.01
    for name, H in family_inputs().items():
        M, st = mp_hmag(H)
        Mo = fp64_hmag(H)
        share = clamped_share(M)
        out[f"t_{name}_H"], out[f"t_{name}_M"] = H, M
        out[f"t_{name}_state{TRAJ_MID}"], out[f"t_{name}_state{TRAJ_N}"] = st[TRAJ_MID], st[TRAJ_N]
        out[f"t_{name}_eref"], out[f"t_{name}_clamped"] = float(np.abs(Mo - M).max()), np.array(share)
        mx = np.abs(M).max()
        print(f"{name}: max|M| {mx:.4g} ({mx / PARAMS[0]:.3g} Ms), oracle error {np.abs(Mo - M).max():.3g} "
              f"({np.abs(Mo - M).max() / mx if mx else 0:.2g} of max|M|), clamped {share}")
        assert name not in UNSATURATED or share == (0.0, 0.0), name
        assert name != "sat" or (share[0] > 0 and share[1] > 0)
        assert name != "zeros" or not M.any()
    Mw, _ = mp_hmag(g9_walk(), marks=())
    out["g9_walk_clamped"] = np.array(clamped_share(Mw))
    print("g9's random walk (2 rows x 300): clamped", out["g9_walk_clamped"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
