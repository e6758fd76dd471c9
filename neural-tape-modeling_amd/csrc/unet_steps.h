// The steps of the diffusion generators around the fused block, one definition per OUTPUT: the resample + combine steps and the
// sampler's EDM arithmetic as __device__ functions of one output each.  unet_kernels.hip's kernels call them with a thread per
// output over a grid; unet_sampler.hip's one-launch sampler calls them with one workgroup striding over a stream's outputs.
// Which thread computes an output differs, the operations on it and their order do not: equal bits.  The notation is
// unet_kernels.hip's.
#pragma once
#include "unet_block.h"

namespace ntm {

// ---- resample + combine ----------------------------------------------------------------------------------------------------------
struct UDownArgs {
    const float *x, *pyr, *ker, *wc;
    float *x_out, *pyr_out;
    int C, F, Fo, S, width, taps;
};

// output frame j of channel c of stream b (and, from c == 0, of the pyramid)
__device__ __forceinline__ void udown_one(const UDownArgs &a, int64_t b, int c, int j)
{
    const float *xr = a.x + (b * a.C + c) * a.F, *pr = a.pyr + b * a.F;
    const int base = j * a.S - a.width;      // j S < F + S <= 2^31 is checked by the caller
    float xd = 0.0f, pd = 0.0f;
    for (int i = 0; i < a.taps; ++i) {
        const int g = base + i;
        if (g >= 0 && g < a.F) {
            const float k = a.ker[i];
            xd = fmaf(k, xr[g], xd);
            pd = fmaf(k, pr[g], pd);
        }
    }
    a.x_out[(b * a.C + c) * a.Fo + j] = (a.wc[c] * pd + xd) * kRsqrt2;
    if (c == 0) a.pyr_out[b * a.Fo + j] = pd;
}

struct UUpArgs {
    const float *x, *pyr, *ker, *wc;
    float *x_out, *pyr_out;
    int C, F, S, width, taps, pyr_T;
    int64_t Fo;
};

// output n = j S + ph of channel c of x
__device__ __forceinline__ void uup_x_one(const UUpArgs &a, int64_t b, int c, int64_t n, int j, int ph)
{
    const float *xr = a.x + (b * a.C + c) * a.F, *kr = a.ker + ph * a.taps;
    float v = 0.0f;
    for (int i = 0; i < a.taps; ++i) {
        const int g = j + i - a.width;
        if (g >= 0 && g < a.F) v = fmaf(kr[i], xr[g], v);
    }
    a.x_out[(b * a.C + c) * a.Fo + n] = v;
}

// frame g of the combined pyramid, which the filter then reads from LDS: 0 outside [0, F)
__device__ __forceinline__ float uup_combined(const UUpArgs &a, int64_t b, int g)
{
    float v = 0.0f;
    if (g >= 0 && g < a.F) {
        if (a.wc) {
            for (int ch = 0; ch < a.C; ++ch) v = fmaf(a.wc[ch], a.x[(b * a.C + ch) * a.F + g], v);
            if (a.pyr) v = (a.pyr[b * a.pyr_T + g] + v) * kRsqrt2;
        } else {
            v = a.x[b * a.F + g];
        }
    }
    return v;
}

// output n = j S + ph of the pyramid from the staged combined frames: pn[i] is frame j - width + i
__device__ __forceinline__ void uup_pyr_one(const UUpArgs &a, int64_t b, int64_t n, int ph, const float *pn)
{
    float v;
    if (a.S == 1 && a.taps == 0) {
        v = pn[0];
    } else {
        const float *kr = a.ker + ph * a.taps;
        v = 0.0f;
        for (int i = 0; i < a.taps; ++i) v = fmaf(kr[i], pn[i], v);
    }
    a.pyr_out[b * a.Fo + n] = v;
}

// ---- the EDM step around the network ----------------------------------------------------------------------------------------------
struct EdmPreArgs {
    const float *z, *eps, *mask, *x_out, *n;
    float *z_out, *net_in;
    float eps_scale, snoise, sigma0, cin;
    int64_t mask_stride, T, N;
};

// z' = z + eps_scale (eps snoise);  z' = mask (x_out + n sigma0) + (1 - mask) z';  net_in = cin z'   -- each product and sum
// rounded on its own, as the reference's tensor expressions are.  Element i of [B][T].
__device__ __forceinline__ void edm_pre_one(const EdmPreArgs &a, int64_t i)
{
    float z = a.z[i];
    if (a.eps) z = __fadd_rn(z, __fmul_rn(a.eps_scale, __fmul_rn(a.eps[i], a.snoise)));
    if (a.mask) {
        const float m = a.mask[(i / a.T) * a.mask_stride + i % a.T];
        const float xn = __fadd_rn(a.x_out[i], __fmul_rn(a.n[i], a.sigma0));
        z = __fadd_rn(__fmul_rn(m, xn), __fmul_rn(__fsub_rn(1.0f, m), z));
    }
    a.z_out[i] = z;
    a.net_in[i] = __fmul_rn(a.cin, z);
}

// x0 = cskip z + cout F;  score = (x0 - z) / b2;  z <- z - k score
__device__ __forceinline__ void edm_post_one(const float *z, const float *F, float cskip, float cout, float b2, float k, int64_t i,
                                             float *out)
{
    const float zi = z[i];
    const float x0 = __fadd_rn(__fmul_rn(cskip, zi), __fmul_rn(cout, F[i]));
    const float score = __fdiv_rn(__fsub_rn(x0, zi), b2);
    out[i] = __fsub_rn(zi, __fmul_rn(k, score));
}

}  // namespace ntm
