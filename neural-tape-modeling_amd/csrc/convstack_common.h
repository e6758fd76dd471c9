// What the three critic conv stacks share: critic_kernels.hip (spectral critics), convstack_kernels.hip (dilated critic) and
// sconv_kernels.hip (MelGAN critic).  Each is n weight-normed Conv1d layers with a LeakyReLU after every layer but the last --
// forward, data gradient, weight gradient and the weight-norm adjoint.  A family file holds its GEMM kernels (the conv kernel in
// its operand-fetch form and the weight gradient; DESIGN.md 11.6-11.8 say why each form exists), its chunk rule and its drivers;
// the plan record, the weight preparation and the weight-norm adjoint are common to them and live here.
//
// stack_prep_kernel   one launch for all layers, one workgroup per output channel: |v| over (c_in/groups, k), w = v * (g / |v|) in
//                     the two layouts the family's conv kernel reads (a Layout functor says where wF and wB of (co, ci, k) go:
//                     wF for the forward, wB for the data gradient), and 1/|v| for the adjoint.
// stack_wnorm_kernel  one launch for the layers a gradient reaches, one workgroup per output channel: adds the partials of a layer's
//                     weight gradient in order (stream chunk major, segment minor) into the first one, then dg = sum(dW v) / |v|,
//                     dv = (g / |v|) (dW - v sum(dW v) / |v|^2), dbias = the sum of the row partials.
#pragma once
#include "ntm.h"
#include "ntm_common.h"

namespace ntm {

// ---- the plan: what the three planners compute alike ----

inline int64_t stack_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Geometry, weight offsets, rows, frames and the `saved` layout.  frames_out(l, F) -> the frames layer l makes of F.  keep_acts:
// `saved` also holds the output of every layer but the last (else they are tensors of the caller's and gz must hold the last
// one too).  The family then fills dil or stride / pad / reflect, and its chunk rule.
template <class Layer, class FramesOut>
inline void stack_plan_layers(StackPlan &p, int64_t B, int64_t F0, int n, const Layer *L, bool keep_acts, FramesOut frames_out)
{
    p = StackPlan{};
    p.n = n;
    p.F[0] = F0;
    for (int l = 0; l < n; ++l) {
        p.c_in[l] = L[l].c_in, p.c_out[l] = L[l].c_out, p.k[l] = L[l].k, p.groups[l] = L[l].groups;
        p.dil[l] = p.stride[l] = 1;
        p.F[l + 1] = frames_out(l, p.F[l]);
        p.w_off[l] = p.w_total;
        p.w_total += p.w_size(l);
        p.row0[l] = p.rows;
        p.rows += L[l].c_out;
    }
    int64_t at = 2 * p.w_total + p.rows;
    for (int l = 0; l < (keep_acts ? n - 1 : n); ++l) {
        const int64_t sz = B * p.c_out[l] * p.F[l + 1];
        if (keep_acts) p.act_off[l] = at, at += sz;
        if (sz > p.gz_size) p.gz_size = sz;
    }
    p.saved_total = at;
}

// the streams in at most max_chunks contiguous chunks of `per` (the spectral and the dilated family)
inline void stack_stream_chunks(int64_t B, int max_chunks, int &nchunk, int &per)
{
    nchunk = (int)(B < max_chunks ? (B > 0 ? B : 1) : max_chunks);
    per = (int)((B + nchunk - 1) / nchunk);
    if (per < 1) per = 1;
    nchunk = (int)((B + per - 1) / per);
}

// ws = gz ping | gz pong | fold | per layer the partials of dW, then of dbias: nchunk[l] * nseg[l] of each, as the family's chunk
// rule has set them
inline void stack_plan_partials(StackPlan &p)
{
    int64_t w = 2 * p.gz_size + p.fold_size;
    for (int l = 0; l < p.n; ++l) {
        const int64_t parts = (int64_t)p.nchunk[l] * p.nseg[l];
        p.part_off[l] = w;
        w += parts * p.w_size(l);
        p.bpart_off[l] = w;
        w += parts * p.c_out[l];
    }
    p.ws_total = w;
}

// sum over the workgroup in a fixed tree order; every thread gets it
template <int NT>
__device__ __forceinline__ float block_sum(float x, float *red)
{
    const int tid = threadIdx.x;
    red[tid] = x;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// ---- prep ----

struct PrepArgs {
    const float *g[kStackMaxLayers], *v[kStackMaxLayers];
    int c_in[kStackMaxLayers], c_out[kStackMaxLayers], k[kStackMaxLayers], groups[kStackMaxLayers], stride[kStackMaxLayers],
        row0[kStackMaxLayers];
    int64_t w_off[kStackMaxLayers];
    int n;
    float *wF, *wB, *invn;
};

// one output channel of one layer as a Layout sees it
struct PrepRow {
    int co, co_l, grp, cin_g, cout_g, c_in, c_out, K, stride;
};

// the slab and per-tap forms: a step's weights are 4 taps x 16 channels
//   wF[k][ci][CO]   (ci within the group, CO every output channel)                                   -- forward
//   wB[j][co][CI]   (co within the group, CI every input channel) = w[co][ci][K-1-j]                 -- data gradient
struct TapMajorLayout {
    static __device__ __forceinline__ void put(const PrepRow &r, float *wF, float *wB, int j, int ci, int k, float w)
    {
        wF[((int64_t)k * r.cin_g + ci) * r.c_out + r.co] = w;
        wB[((int64_t)(r.K - 1 - k) * r.cout_g + r.co_l) * r.c_in + r.grp * r.cin_g + ci] = w;
    }
};

template <class Layout>
__global__ __launch_bounds__(256) void stack_prep_kernel(PrepArgs a)
{
    __shared__ float red[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    int l = 0;
    while (l + 1 < a.n && row >= a.row0[l + 1]) ++l;
    const int co = row - a.row0[l], K = a.k[l], cin_g = a.c_in[l] / a.groups[l], cout_g = a.c_out[l] / a.groups[l];
    const int n = cin_g * K, grp = co / cout_g;
    const PrepRow r{co, co - grp * cout_g, grp, cin_g, cout_g, a.c_in[l], a.c_out[l], K, a.stride[l]};
    const float *v = a.v[l] + (int64_t)co * n;
    float s = 0.0f;
    for (int j = tid; j < n; j += 256) s = fmaf(v[j], v[j], s);
    const float norm = sqrtf(block_sum<256>(s, red));
    const float scale = a.g[l][co] / norm;
    float *wF = a.wF + a.w_off[l], *wB = a.wB + a.w_off[l];
    for (int j = tid; j < n; j += 256) {
        const int ci = j / K;
        Layout::put(r, wF, wB, j, ci, j - ci * K, v[j] * scale);
    }
    if (tid == 0) a.invn[row] = 1.0f / norm;
}

// saved = wF | wB | 1/|v| | ...
template <class Layout>
inline hipError_t launch_stack_prep(const StackPlan &p, const float *const *g, const float *const *v, float *saved, hipStream_t stream)
{
    PrepArgs a{};
    for (int l = 0; l < p.n; ++l) {
        a.g[l] = g[l], a.v[l] = v[l];
        a.c_in[l] = p.c_in[l], a.c_out[l] = p.c_out[l], a.k[l] = p.k[l], a.groups[l] = p.groups[l], a.stride[l] = p.stride[l];
        a.row0[l] = p.row0[l], a.w_off[l] = p.w_off[l];
    }
    a.n = p.n;
    a.wF = saved, a.wB = saved + p.w_total, a.invn = saved + 2 * p.w_total;
    hipLaunchKernelGGL(stack_prep_kernel<Layout>, dim3((unsigned)p.rows), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---- weight-norm adjoint ----

struct WnormArgs {
    const float *g[kStackMaxLayers], *v[kStackMaxLayers];
    float *dg[kStackMaxLayers], *dv[kStackMaxLayers], *db[kStackMaxLayers];
    float *part[kStackMaxLayers];         // the sum of a row's partials is left in its first partial
    const float *bpart[kStackMaxLayers];
    int c_out[kStackMaxLayers], rowlen[kStackMaxLayers], row0[kStackMaxLayers];
    int64_t nparts[kStackMaxLayers];
    int n;
    const float *invn;
};

// (a template so that the three files share one definition)
template <int NT>
__global__ __launch_bounds__(NT) void stack_wnorm_kernel(WnormArgs a)
{
    __shared__ float red[NT];
    const int row = blockIdx.x, tid = threadIdx.x;
    int l = 0;
    while (l + 1 < a.n && row >= a.row0[l + 1]) ++l;
    const int co = row - a.row0[l], n = a.rowlen[l];
    const int64_t cstride = (int64_t)a.c_out[l] * n, np = a.nparts[l];
    const float *v = a.v[l] + (int64_t)co * n;
    float *p = a.part[l] + (int64_t)co * n;
    float s = 0.0f;
    for (int j = tid; j < n; j += NT) {
        float dw = p[j];
        int64_t c = 1;
        for (; c + 4 <= np; c += 4) {           // four loads in flight, added in chunk order
            const float p0 = p[c * cstride + j], p1 = p[(c + 1) * cstride + j], p2 = p[(c + 2) * cstride + j], p3 = p[(c + 3) * cstride + j];
            dw = (((dw + p0) + p1) + p2) + p3;
        }
        for (; c < np; ++c) dw += p[c * cstride + j];
        p[j] = dw;
        s = fmaf(dw, v[j], s);
    }
    const float dot = block_sum<NT>(s, red);
    const float inv = a.invn[row], scale = a.g[l][co] * inv, proj = dot * inv * inv;
    float *dv = a.dv[l] + (int64_t)co * n;
    for (int j = tid; j < n; j += NT) dv[j] = scale * (p[j] - v[j] * proj);
    if (tid == 0) {
        a.dg[l][co] = dot * inv;
        float sb = a.bpart[l][co];
        for (int64_t c = 1; c < np; ++c) sb += a.bpart[l][c * a.c_out[l] + co];
        a.db[l][co] = sb;
    }
}

// layers 0 .. n_reached - 1 (the strided family: those a gradient reaches; else all of them)
inline hipError_t launch_stack_wnorm(const StackPlan &p, int n_reached, const float *const *g, const float *const *v, float *const *dg,
                                     float *const *dv, float *const *dbias, const float *saved, float *ws, hipStream_t stream)
{
    WnormArgs a{};
    for (int l = 0; l < n_reached; ++l) {
        a.g[l] = g[l], a.v[l] = v[l], a.dg[l] = dg[l], a.dv[l] = dv[l], a.db[l] = dbias[l];
        a.part[l] = ws + p.part_off[l], a.bpart[l] = ws + p.bpart_off[l];
        a.c_out[l] = p.c_out[l], a.rowlen[l] = p.cin_g(l) * p.k[l], a.row0[l] = p.row0[l];
        a.nparts[l] = (int64_t)p.nchunk[l] * p.nseg[l];
    }
    a.n = n_reached, a.invn = saved + 2 * p.w_total;
    const int rows = p.row0[n_reached - 1] + p.c_out[n_reached - 1];
    hipLaunchKernelGGL(stack_wnorm_kernel<256>, dim3((unsigned)rows), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ntm
