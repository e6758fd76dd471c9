"""CPU side of the time-domain loss tests (tests/test_gpu_losses.py): the exact references of tests/helpers.py
(numpy.longdouble recursion on the float32 inputs) agree with mpmath at 40 digits and with the same recursion in float64, and the
INPUTS of every GPU case asserted at the 2e-5 bar are well enough conditioned for that bar to mean something: the float32
sequential recursion of the C oracle -- the arithmetic any float32 evaluation of the filter shares -- stays within a tenth
of the bar of the exact sums there.  A case that broke this would be replaced, not the bar."""
import numpy as np
import pytest

import oracle
from helpers import (DCPRE_COND_B, DCPRE_COND_N, DCPRE_COND_POLES, DCPRE_COND_SEED, DCPRE_COND_SKIP, DCPRE_GROWTH_B, DCPRE_GROWTH_FAMILIES,
                     DCPRE_GROWTH_N, DCPRE_GROWTH_SEED, DCPRE_STRUCT_B, DCPRE_STRUCT_N, DCPRE_STRUCT_SEED, DCPRE_STRUCT_SKIP, FLUSH_FAMILIES,
                     FLUSH_POLES, FLUSH_SEED, FLUSH_T, LOSS_BAR, LOSS_FAMILIES, R_BELOW_ONE, dcpre_sums_exact, esr_sums_exact, flush_skips,
                     loss_family, rel_err)

E_REF_MAX = LOSS_BAR / 10


def e_ref(y, t, skip, R):
    return float(rel_err(oracle.esr_dcpre_sums(y, t, skip, R), dcpre_sums_exact(y, t, skip, R)).max(initial=0.0))


def test_the_family_table_is_what_it_says():
    assert tuple(LOSS_FAMILIES) == ("noise_offset", "dc_small_ac", "step", "slow_sine", "const", "tight_fit")
    B, T = 3, 400
    for name in LOSS_FAMILIES:
        y, t = loss_family(name, 1, B, T)
        y2, t2 = loss_family(name, 1, B, T)
        assert y.dtype == t.dtype == np.float32 and y.shape == t.shape == (B, T) and np.array_equal(y, y2) and np.array_equal(t, t2), name
        assert y.flags.c_contiguous and t.flags.c_contiguous and not np.array_equal(y[0], y[1]), name
    _, t = loss_family("noise_offset", 1, 8, 4000)
    assert abs(t.mean() - 0.3) < 0.05 and abs(t.std() - 1.0) < 0.05
    y, t = loss_family("dc_small_ac", 1, B, T)
    assert abs(t.mean() - 1.0) < 1e-3 and 5e-4 < t.std() < 2e-3 and abs(y.mean() - 0.9) < 1e-3
    y, t = loss_family("step", 1, B, T)
    assert (t[:, :T // 2 + 3] == 0).all() and (t[:, T // 2 + 3:] == np.float32(0.7)).all()
    y, t = loss_family("slow_sine", 1, B, 8000)
    assert t.min() >= 0 and t.max() <= 1 and t.max() - t.min() > 0.99 and not np.allclose(t[0], t[1], atol=1e-2)
    y, t = loss_family("const", 1, B, T)
    assert (t == t[:, :1]).all() and (y == y[:, :1]).all() and len(set(t[:, 0].tolist())) == B
    y, t = loss_family("tight_fit", 1, B, T)
    e = np.abs(t - y)
    assert e.max() < 1e-5 and 0 < e.mean() < 2e-6 and abs(t.mean() - 1.0) < 1e-3       # a few ulp(1) = 1.2e-7
    assert np.float32(R_BELOW_ONE) < 1 and np.nextafter(np.float32(R_BELOW_ONE), np.float32(2)) == 1


@pytest.mark.parametrize("name,T,skip,R", [("slow_sine", 64, 0, 0.995), ("dc_small_ac", 40, 7, 0.9999), ("tight_fit", 33, 32, R_BELOW_ONE)])
def test_exact_reference_equals_mpmath_at_40_digits(name, T, skip, R):
    import mpmath
    y, t = loss_family(name, 3, 2, T)
    got = dcpre_sums_exact(y, t, skip, R)
    got_esr = esr_sums_exact(y, t, skip)
    e = t - y
    with mpmath.workdps(40):
        r = mpmath.mpf(float(np.float32(R)))
        for b in range(2):
            for col, u in enumerate((e[b], t[b])):
                f, prev, s, s0 = mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0)
                for n in range(skip, T):
                    cur = mpmath.mpf(float(u[n]))
                    f = (cur - prev) + r * f
                    s += f * f
                    s0 += cur * cur
                    prev = cur
                # longdouble -> mpf without going through float64: high part + remainder, both exact
                for have, want in ((got[b, col], s), (got_esr[b, col], s0)):
                    hi = float(have)
                    have_mp = mpmath.mpf(hi) + mpmath.mpf(float(have - np.longdouble(hi)))
                    assert want > 0 and abs(have_mp - want) <= mpmath.mpf(10) ** -15 * want, (name, b, col)


@pytest.mark.parametrize("name", list(LOSS_FAMILIES))
def test_exact_reference_equals_the_float64_recursion(name):
    for n, skip, poles in ((1025, 5, (0.0, 0.5, 0.995)), (4097, 0, (0.9, 0.9999, R_BELOW_ONE))):
        y, t = loss_family(name, 5, 2, skip + n)
        ld = dcpre_sums_exact(y, t, skip, poles)
        f64 = dcpre_sums_exact(y, t, skip, poles, dtype=np.float64)
        assert ld.dtype == np.longdouble and f64.dtype == np.float64 and ld.shape == f64.shape == (3, 2, 2)
        assert rel_err(f64, ld).max() <= 1e-9, (name, n, rel_err(f64, ld).max())
        for i, R in enumerate(poles):                     # a sequence of poles is the scalar calls stacked
            assert np.array_equal(dcpre_sums_exact(y, t, skip, R), ld[i])
    assert np.finfo(np.longdouble).nmant >= 63            # the extended format, not an alias of float64


def test_exact_reference_definition_edges():
    y, t = loss_family("noise_offset", 7, 2, 50)
    assert (dcpre_sums_exact(y, t, 50, 0.995) == 0).all() and (esr_sums_exact(y, t, 50) == 0).all()
    # one sample: u[skip - 1] := 0, so f = u[skip] whatever stands in front of it
    one = dcpre_sums_exact(y, t, 49, 0.995)
    e = (t - y)[:, 49].astype(np.longdouble)
    assert np.array_equal(one[:, 0], e * e) and np.array_equal(one[:, 1], t[:, 49].astype(np.longdouble) ** 2)
    y2, t2 = y.copy(), t.copy()
    y2[:, 48], t2[:, 48] = np.nan, 1e30
    assert np.array_equal(dcpre_sums_exact(y2, t2, 49, 0.995), one)
    # pole 0 is the first difference
    d = np.diff(np.concatenate([np.zeros((2, 1), np.float32), t[:, 10:]], 1).astype(np.longdouble), axis=1)
    assert rel_err(dcpre_sums_exact(y, t, 10, 0.0)[:, 1], (d * d).sum(1)).max() < 1e-18


def test_oracle_esr_sums_equal_the_exact_ones():
    """The oracle adds n exact float64 products (a product of two float32 is exact in float64) one after the other: at most
    (n - 1) 2^-53 relative, all terms being positive -- 8.8e-15 at n = 80, inside the 1e-14 asked of it; at n = 4097 the same
    bound is 4.5e-13."""
    for name in LOSS_FAMILIES:
        for n, bound in ((80, 1e-14), (4097, 4096 * 2.0 ** -53)):
            y, t = loss_family(name, 9, 3, n + 5)
            assert rel_err(oracle.esr_sums(y, t, 5), esr_sums_exact(y, t, 5)).max() <= bound, (name, n)
    assert (oracle.esr_sums(y, t, 4102) == 0).all()


# ---- the input condition of every GPU case asserted at 2e-5: E_ref = |oracle - exact| / exact <= 2e-6
def test_condition_of_the_structure_cases():
    worst = 0.0
    for n in DCPRE_STRUCT_N:
        for skip in DCPRE_STRUCT_SKIP:
            y, t = loss_family("slow_sine", DCPRE_STRUCT_SEED, DCPRE_STRUCT_B, skip + n)
            worst = max(worst, e_ref(y, t, skip, 0.995))
            if n >= 2:                                    # skip = T - 1 and skip = T of the same signals
                assert e_ref(y, t, skip + n - 1, 0.995) == 0.0
    print(f"E_ref structure cases: {worst:.2e}")
    assert worst <= E_REF_MAX, worst


@pytest.mark.parametrize("name", list(LOSS_FAMILIES))
def test_condition_of_the_conditioning_cases(name):
    worst = {}
    for n in DCPRE_COND_N:
        y, t = loss_family(name, DCPRE_COND_SEED, DCPRE_COND_B, DCPRE_COND_SKIP + n)
        for R in DCPRE_COND_POLES + (0.9999,):
            worst[R] = max(worst.get(R, 0.0), e_ref(y, t, DCPRE_COND_SKIP, R))
    print(f"E_ref {name}: " + ", ".join(f"{R}: {v:.2e}" for R, v in worst.items()))
    assert max(worst.values()) <= E_REF_MAX, worst


@pytest.mark.parametrize("name", DCPRE_GROWTH_FAMILIES)
def test_condition_of_the_growth_cases(name):
    y, t = loss_family(name, DCPRE_GROWTH_SEED, DCPRE_GROWTH_B, DCPRE_GROWTH_N)
    ex = dcpre_sums_exact(y, t, 0, (0.995, 0.9999))
    e = [float(rel_err(oracle.esr_dcpre_sums(y, t, 0, R), ex[i]).max()) for i, R in enumerate((0.995, 0.9999))]
    print(f"E_ref growth {name}: 0.995: {e[0]:.2e}, 0.9999: {e[1]:.2e}")
    assert e[0] <= E_REF_MAX, e


@pytest.mark.parametrize("name", FLUSH_FAMILIES)
def test_condition_of_the_fused_flush_targets(name):
    """Column 1 of the fused-flush cases is a function of the family alone (column 0 needs the model's output: the GPU test
    checks its E_ref where it runs)."""
    worst = 0.0
    for T in FLUSH_T:
        y, t = loss_family(name, FLUSH_SEED, 16, T)
        for skip in flush_skips(T):
            ex = dcpre_sums_exact(y, t, skip, FLUSH_POLES)
            for i, R in enumerate(FLUSH_POLES):
                worst = max(worst, float(rel_err(oracle.esr_dcpre_sums(y, t, skip, R)[:, 1], ex[i][:, 1]).max(initial=0.0)))
    print(f"E_ref fused-flush targets {name}: {worst:.2e}")
    assert worst <= E_REF_MAX, worst
    assert all(s % 4 == 0 and s <= T for T in FLUSH_T for s in flush_skips(T)) and flush_skips(300) == (0, 4, 64, 68, 300)
    assert flush_skips(1) == (0,) and flush_skips(65) == (0, 4, 64)
