// Training of the diffusion generators' network: the adjoints of the resample + combine steps of unet_kernels.hip
// (unet_down_kernel, unet_up_kernel).  Plain fp32 like the forwards: bound by memory and launches, no matrix pipe.  No atomics, and
// every sum is a GATHER in a fixed order: equal calls give equal bits, and a stream's results never depend on its batch.
//
// unet_down_backward_kernel   forward: pd[j] = sum_i ker[i] pyr[j S - w + i], xd likewise, xo = (wc[c] pd + xd) / sqrt 2, po = pd.
//                     grid (frame tiles of kRTile + 1, C + 1, B).  Plane c < C, tile t: g_x[c][f] = (sum_j ker[f + w - j S]
//                     g_xo[c][j]) / sqrt 2, j ascending over the terms in range.  Plane C: g_pd[j] = g_po[j] + (sum_c wc[c]
//                     g_xo[c][j]) / sqrt 2 for the j under the tile, once, in LDS; then the same gather gives g_pyr.  The extra
//                     tile of a plane c < C is the combiner weight: sum_j g_xo[c][j] pd[j] over the whole stream in fp64 (a
//                     thread adds its frames in ascending order, the 256 sums add as a tree through LDS), times 1 / sqrt 2,
//                     rounded once -> part [B][C].
// unet_up_backward_kernel     forward: p = sum_ch wc[ch] x[ch] (with a pyramid (pyr + p) / sqrt 2), xo[c][j S + ph] = sum_i
//                     ker[ph][i] x[c][j + i - w], po the same filter of p; S = 1 without a filter: po = p.
//                     grid (frame tiles of kRTile, B).  g_p[f] = sum_{ph, i} ker[ph][i] g_po[(f - i + w) S + ph] (/ sqrt 2 with a
//                     pyramid) once per tile, kept in a register and in LDS; then per channel g_x[c][f] = the same gather of
//                     g_xo[c] + wc[c] g_p[f].  g_pyr = g_p, and 0 from F to pyr_T (the last tile writes those).  The combiner
//                     weight of the tile: thread (ch, seg) adds g_p[f] x[ch][f] over the kRSeg frames of its segment in fp64 in
//                     ascending order, the kRTile / kRSeg segment sums add in order, rounded once -> part [B][tiles][C].
// ntm_unet_wgrad_reduce (unet_train.hip) adds either kind of partial over the streams in index order in fp64.
#include "unet_block.h"

namespace ntm {

constexpr int kRTile = 256;                 // frames of a workgroup, one per thread
constexpr int kRStage = kRTile + 64 + 16;   // g_pd under a tile of the down adjoint: (kRTile + taps - 2) / S + 2 <= 320, taps <= 64
constexpr int kRSeg = 32;                   // frames a thread adds for the up adjoint's combiner weight: 8 segments x 32 channels
constexpr double kRsqrt2d = 0.70710678118654752440;

struct UDownBackArgs {
    const float *pd, *ker, *wc, *g_xo, *g_po;
    float *g_x, *g_pyr, *part;
    int C, F, Fo, S, width, taps, tiles;
};

// the outputs j that read input frame f: i = f + w - j S in [0, taps), j in [0, Fo)
__device__ __forceinline__ void down_terms(const UDownBackArgs &a, int f, int &jlo, int &jhi)
{
    const int t = f + a.width - (a.taps - 1);
    jlo = t <= 0 ? 0 : (t + a.S - 1) / a.S;
    jhi = (f + a.width) / a.S;
    if (jhi > a.Fo - 1) jhi = a.Fo - 1;
}

__global__ __launch_bounds__(kRTile) void unet_down_backward_kernel(UDownBackArgs a)
{
    __shared__ float gpd[kRStage];
    __shared__ double red[kRTile];
    const int tid = threadIdx.x, c = blockIdx.y, tile = blockIdx.x;
    const int64_t b = blockIdx.z;
    if (tile == a.tiles) {                                  // the combiner weight of (b, c): block-uniform
        if (c == a.C || !a.part) return;
        double acc = 0.0;
        if (a.g_xo) {
            const float *gr = a.g_xo + (b * a.C + c) * a.Fo, *pr = a.pd + b * a.Fo;
            for (int j = tid; j < a.Fo; j += kRTile) acc += (double)gr[j] * (double)pr[j];
        }
        red[tid] = acc;
        __syncthreads();
        for (int s = kRTile / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) a.part[b * a.C + c] = (float)(red[0] * kRsqrt2d);
        return;
    }
    const int f0 = tile * kRTile, f = f0 + tid;
    if (c < a.C) {                                          // a channel of x
        if (!a.g_x || f >= a.F) return;
        float v = 0.0f;
        if (a.g_xo) {
            const float *gr = a.g_xo + (b * a.C + c) * a.Fo;
            int jlo, jhi;
            down_terms(a, f, jlo, jhi);
            for (int j = jlo; j <= jhi; ++j) v = fmaf(a.ker[f + a.width - j * a.S], gr[j], v);
        }
        a.g_x[(b * a.C + c) * a.F + f] = v * kRsqrt2;
        return;
    }
    // the pyramid: g_pd of the outputs under this tile once, then the gather
    if (!a.g_pyr) return;
    const int fl = f0 + kRTile - 1 < a.F ? f0 + kRTile - 1 : a.F - 1;
    int j0, j1, unused;
    down_terms(a, f0, j0, unused);
    down_terms(a, fl, unused, j1);
    for (int t = tid; t <= j1 - j0; t += kRTile) {          // at most kRStage values
        const int j = j0 + t;
        float s = 0.0f;
        if (a.g_xo) {
            for (int ch = 0; ch < a.C; ++ch) s = fmaf(a.wc[ch], a.g_xo[(b * a.C + ch) * a.Fo + j], s);
            s *= kRsqrt2;
        }
        gpd[t] = a.g_po ? a.g_po[b * a.Fo + j] + s : s;
    }
    __syncthreads();
    if (f >= a.F) return;
    int jlo, jhi;
    down_terms(a, f, jlo, jhi);
    float v = 0.0f;
    for (int j = jlo; j <= jhi; ++j) v = fmaf(a.ker[f + a.width - j * a.S], gpd[j - j0], v);
    a.g_pyr[b * a.F + f] = v;
}

struct UUpBackArgs {
    const float *x, *ker, *wc, *g_xo, *g_po;
    float *g_x, *g_pyr, *part;
    int C, F, S, width, taps, pyr_T, tiles;
    int64_t Fo;
};

// sum_{ph, i} ker[ph][i] g[(f - i + w) S + ph] over the input frames j = f - i + w in [0, F); S = 1 without a filter: g[f]
__device__ __forceinline__ float up_gather(const UUpBackArgs &a, const float *g, int f)
{
    if (a.taps == 0) return g[f];
    float v = 0.0f;
    for (int ph = 0; ph < a.S; ++ph) {
        const float *kr = a.ker + ph * a.taps;
        for (int i = 0; i < a.taps; ++i) {
            const int j = f - i + a.width;
            if (j >= 0 && j < a.F) v = fmaf(kr[i], g[(int64_t)j * a.S + ph], v);
        }
    }
    return v;
}

__global__ __launch_bounds__(kRTile) void unet_up_backward_kernel(UUpBackArgs a)
{
    __shared__ float gps[kRTile];
    __shared__ double seg[32 * (kRTile / kRSeg)];
    const int tid = threadIdx.x, tile = blockIdx.x, f0 = tile * kRTile, f = f0 + tid;
    const int64_t b = blockIdx.y;
    const bool live = f < a.F;
    float gp = 0.0f;
    if (live && a.g_po) {
        gp = up_gather(a, a.g_po + b * a.Fo, f);
        if (a.pyr_T) gp *= kRsqrt2;
    }
    gps[tid] = gp;                                          // 0 past F
    if (a.g_pyr) {
        if (live) a.g_pyr[b * a.pyr_T + f] = gp;
        if (tile == a.tiles - 1)
            for (int g = a.F + tid; g < a.pyr_T; g += kRTile) a.g_pyr[b * a.pyr_T + g] = 0.0f;
    }
    if (a.g_x && live)
        for (int c = 0; c < a.C; ++c) {
            const float v = a.g_xo ? up_gather(a, a.g_xo + (b * a.C + c) * a.Fo, f) : 0.0f;
            a.g_x[(b * a.C + c) * a.F + f] = fmaf(a.wc[c], gp, v);
        }
    if (!a.part) return;                                    // block-uniform
    __syncthreads();
    constexpr int kSegs = kRTile / kRSeg;
    const int ch = tid / kSegs, sg = tid % kSegs;
    if (ch < a.C) {
        const float *xr = a.x + (b * a.C + ch) * a.F;
        double acc = 0.0;
        for (int t = sg * kRSeg; t < (sg + 1) * kRSeg && f0 + t < a.F; ++t) acc += (double)gps[t] * (double)xr[f0 + t];
        seg[tid] = acc;
    }
    __syncthreads();
    if (tid < a.C) {
        double acc = 0.0;
        for (int s = 0; s < kSegs; ++s) acc += seg[tid * kSegs + s];
        a.part[(b * a.tiles + tile) * a.C + tid] = (float)acc;
    }
}

int64_t unet_up_backward_tiles(int64_t F) { return (F + kRTile - 1) / kRTile; }

hipError_t launch_unet_down_backward(const float *pd, const float *ker, const float *wc, const float *g_xo, const float *g_po,
                                     int64_t B, int C, int64_t F, int S, int width, int taps, float *g_x, float *g_pyr, float *part,
                                     hipStream_t stream)
{
    UDownBackArgs a{pd, ker, wc, g_xo, g_po, g_x, g_pyr, part, C, (int)F, (int)((F + S - 1) / S), S, width, taps,
                    (int)((F + kRTile - 1) / kRTile)};
    hipLaunchKernelGGL(unet_down_backward_kernel, dim3((unsigned)a.tiles + 1u, (unsigned)C + 1u, (unsigned)B), dim3(kRTile), 0, stream,
                       a);
    return hipGetLastError();
}

hipError_t launch_unet_up_backward(const float *x, const float *ker, const float *wc, const float *g_xo, const float *g_po, int64_t B,
                                   int C, int64_t F, int S, int width, int taps, int64_t pyr_T, float *g_x, float *g_pyr, float *part,
                                   hipStream_t stream)
{
    UUpBackArgs a{x, ker, wc, g_xo, g_po, g_x, g_pyr, part, C, (int)F, S, width, taps, (int)pyr_T, (int)unet_up_backward_tiles(F),
                  (int64_t)S * F};
    hipLaunchKernelGGL(unet_up_backward_kernel, dim3((unsigned)a.tiles, (unsigned)B), dim3(kRTile), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ntm
