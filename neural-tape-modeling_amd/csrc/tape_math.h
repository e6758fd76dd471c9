// fp64 arithmetic of the Jiles-Atherton stage (Tape._f, code/tape.py:587-635): the hand-written replacements of the
// library's tanh and division and the right-hand side ja_f built from them.  Shared by the product kernel
// (tape_kernels.hip, tape_hmag_kernel) and the laboratory's elementwise probe (lab_api.hip, ntm_lab_tape_math), which
// exists so that tests can reach every helper on its own.  The callers compile their bodies under
// `#pragma clang fp contract(off)`.
#pragma once
#include "ntm_common.h"

namespace ntm {

struct JaParams { double Ms, A, alpha, K, c, rA; };   // rA = 1/A

// The recurrence is one wave's dependent fp64 chain (a GPU has far more SIMDs than 4096 streams need waves), so
// what counts is the DEPTH of the per-sample computation, not its instruction count.  The two helpers below
// replace ocml's tanh (165 instructions, mostly serial) and the IEEE division (12).

// 1/x for x != 0 (finite, normal): v_rcp_f64 seed r0 (~2^-23), e = 1 - x r0, result r0 (1 + e)(1 + e^2): error
// e^4, within 1 ulp; dependent depth 4.  Only used where the denominator cannot vanish.
__device__ __forceinline__ double rcp_nr(double x)
{
    const double r0 = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, r0, 1.0);
    const double r1 = fma(e, r0, r0), e2 = e * e;
    return fma(r1, e2, r1);
}

// expm1(x) for x <= 0: x = n ln2 + r, |r| <= ln2/2; expm1(r) = r + r^2 q(r) with the degree-11 Taylor q evaluated by
// Estrin's scheme (depth 5); expm1(x) = 2^n expm1(r) + (2^n - 1).  Relative error ~2e-16 where it matters
// (small |x|, n = 0); x very negative gives -1.
__device__ __forceinline__ double expm1_neg(double x)
{
    const double nf = __builtin_rint(x * 1.4426950408889634);
    double r = fma(-nf, 6.93147180369123816490e-01, x);        // ln2 hi / lo (fdlibm split)
    r = fma(-nf, 1.90821492927058770002e-10, r);
    const int n = (int)nf;
    const double s = __builtin_amdgcn_ldexp(1.0, n < -1080 ? -1080 : n);
    const double sm1 = s - 1.0;
    const double r2 = r * r;
    const double a0 = fma(r, 1.0 / 6, 1.0 / 2), a1 = fma(r, 1.0 / 120, 1.0 / 24), a2 = fma(r, 1.0 / 5040, 1.0 / 720);
    const double a3 = fma(r, 1.0 / 362880, 1.0 / 40320), a4 = fma(r, 1.0 / 39916800, 1.0 / 3628800);
    const double a5 = fma(r, 1.0 / 6227020800.0, 1.0 / 479001600);
    const double r4 = r2 * r2;
    const double b0 = fma(a1, r2, a0), b1 = fma(a3, r2, a2), b2 = fma(a5, r2, a4);
    const double r8 = r4 * r4;
    const double q = fma(b2, r8, fma(b1, r4, b0));
    const double pm = fma(r2, q, r);
    return fma(s, pm, sm1);
}

// coth(x) for |x| > 1e-4 from ONE expm1: with em = expm1(-2|x|) in (-1, 0), coth|x| = (2 + em) / (-em).
__device__ __forceinline__ double coth_gt(double x)
{
    const double em = expm1_neg(-2.0 * fabs(x));
    return copysign((2.0 + em) * rcp_nr(-em), x);
}

// L'(x) = 1/x^2 - coth^2 x + 1 for |x| < 1 (its argument here is L(Q), a Langevin value) as the even Taylor series
// sum_k (2k-1) 2^2k B_2k / (2k)! x^(2k-2), 16 terms by Estrin's scheme: depth 6 and 20 instructions instead of a second
// expm1 + two reciprocals (depth 23, 45 instructions) on the critical path of every RK4 stage; truncation 1e-15 at
// |x| = 1 (ratio of successive terms 1/pi^2), and no cancellation where the closed form loses digits (1/x^2 - coth^2 x
// for small x).  Coefficients: exact rationals rounded to double.
__device__ __forceinline__ double langevin_prime_lt1(double x)
{
    const double z = x * x, z2 = z * z, z4 = z2 * z2, z8 = z4 * z4;
    const double a0 = fma(z, -0.06666666666666667, 0.3333333333333333), a1 = fma(z, -0.0014814814814814814, 0.010582010582010581);
    const double a2 = fma(z, -2.380844708887037e-05, 0.0001924001924001924), a3 = fma(z, -3.332191318496952e-07, 2.8503732207435913e-06);
    const double a4 = fma(z, -4.332978728872515e-09, 3.8263339078575285e-08), a5 = fma(z, -5.3846925685597234e-11, 4.852350845790551e-10);
    const double a6 = fma(z, -6.489292139993081e-13, 5.930254350058414e-12), a7 = fma(z, -7.648843294003344e-15, 7.062066668463177e-14);
    const double b0 = fma(a1, z2, a0), b1 = fma(a3, z2, a2), b2 = fma(a5, z2, a4), b3 = fma(a7, z2, a6);
    const double c0 = fma(b1, z4, b0), c1 = fma(b3, z4, b2);
    return fma(c1, z8, c0);
}

__device__ __forceinline__ double ja_f(double Mn, double Hn, double Hp, const JaParams &p)
{
    const double Q = (Hn + p.alpha * Mn) * p.rA;
    const double LQ = fabs(Q) > 1e-4 ? coth_gt(Q) - rcp_nr(Q) : Q * (1.0 / 3.0);
    double LpQ;
    // (the reference evaluates L' on L(Q), not on Q: code/tape.py:598-603 -- reproduced)
    LpQ = fabs(LQ) > 1e-4 ? langevin_prime_lt1(LQ) : 1.0 / 3.0;        // |LQ| < 1 always: LQ is a Langevin value
    const double M_diff = p.Ms * LQ - Mn;
    const double dS = Hp > 0.0 ? 1.0 : -1.0;
    const double sgn = M_diff > 0.0 ? 1.0 : (M_diff < 0.0 ? -1.0 : 0.0);
    const double dM = (dS == sgn) ? 1.0 : 0.0;
    const double t1n = (1.0 - p.c) * dM * M_diff;
    const double t1d = (1.0 - p.c) * dS * p.K - p.alpha * M_diff;
    const double t1 = (t1n / t1d) * Hp;                  // IEEE division: t1d may vanish (inf, as in the reference)
    const double t2 = p.c * (p.Ms / p.A) * Hp * LpQ;
    const double t3 = 1.0 - p.c * p.alpha * (p.Ms / p.A) * LpQ;     // >= 1 - c alpha Ms / (3 A) > 0 for physical parameters
    return (t1 + t2) * rcp_nr(t3);
}

}  // namespace ntm
