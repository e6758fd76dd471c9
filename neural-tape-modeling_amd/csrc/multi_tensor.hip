// The optimiser step over a list of tensors (ntm_multi_* in include/ntm.h): the gradient norm of clip_grad_norm_, torch's
// single-tensor Adam and the EMA of the diffusion trainer.  Plain fp32 elementwise kernels, latency- and launch-bound: the work
// is a hundred small tensors, so the point is few launches and no host synchronisation, not bytes per second.
//
// A launch serves up to NTM_MULTI_MAX_TENSORS tensors.  Their pointers, their sizes and the chunk-to-tensor map travel BY VALUE
// in the kernel arguments (MultiTable, below 4 KB): no host-to-device copy, nothing whose lifetime has to outlast the launch.  The
// map is the prefix sum first[]: tensor k owns the workgroups [first[k], first[k + 1]) of the grid, each a 256-thread workgroup
// on one chunk of NTM_MULTI_CHUNK elements; a workgroup finds its tensor by a uniform binary search.  Tensors of zero elements
// never enter a table.
//
//   multi_sqnorm_kernel         partial[base + chunk] = the chunk's sum of g^2 in fp64: thread i adds the elements of its groups of
//                               four (groups i, i + 256, ..., each in index order) ascending, then a fixed LDS tree over the 256 sums;
//   multi_norm_finalize_kernel  one workgroup: the partials of all launches, added in index order in fp64 ->
//                               norm = (float)sqrt(sum), coef = (float)min(1, max_norm / (sqrt(sum) + 1e-6));
//   multi_adam_kernel           per element torch's single-tensor Adam in torch's order of operations (see adam_element);
//   multi_ema_kernel            dst = dst * s + src * (1 - s): two rounded products, one rounded sum.
// 16-byte accesses where every base pointer of the tensor is 16-byte aligned (a chunk starts a multiple of 16 bytes behind it),
// else the same elements one by one -- a parameter that is a view at an odd element offset is legal.  Which thread handles which
// element does not depend on the path, so neither does a bit of any result.  No atomics, nothing crosses a workgroup within a
// launch: equal calls give equal bits.
//
// No implicit contraction anywhere in this file: a fused multiply-add rounds once where torch's separate kernels round twice.
// Division and sqrtf are the correctly rounded ones (hipcc's default for fp32; no v_rcp_f32 / v_rsq_f32 shortcuts).
#include "ntm_common.h"

#pragma clang fp contract(off)

namespace ntm {

constexpr int kMultiThreads = 256;
constexpr int kMultiChunk = NTM_MULTI_CHUNK;
constexpr int kMultiRounds = kMultiChunk / (4 * kMultiThreads);
static_assert(kMultiChunk % (4 * kMultiThreads) == 0, "a chunk is a whole number of float4 rounds of the workgroup");
static_assert(sizeof(MultiTable<4>) + 64 <= 4096, "the table and the scalars must fit HIP's 4 KB of kernel arguments");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the tensor of workgroup `blk`: the largest k with first[k] <= blk (first[] is strictly increasing, first[0] == 0)
template <int NP>
__device__ __forceinline__ int multi_find(const MultiTable<NP> &t, int blk)
{
    int lo = 0, hi = t.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.first[mid] <= blk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// what a workgroup works on: tensor k, the offset of its chunk, the chunk's length, and whether the 16-byte path is legal
struct MultiChunk {
    int k, n;
    int64_t off;
    bool vec;
};

template <int NP>
__device__ __forceinline__ MultiChunk multi_chunk(const MultiTable<NP> &t)
{
    MultiChunk c;
    c.k = multi_find(t, (int)blockIdx.x);
    c.off = (int64_t)((int)blockIdx.x - t.first[c.k]) * kMultiChunk;
    const int64_t left = t.n[c.k] - c.off;
    c.n = (int)(left < kMultiChunk ? left : kMultiChunk);
    uintptr_t bits = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) bits |= (uintptr_t)t.ptr[j][c.k];
    c.vec = (bits & 15) == 0;
    return c;
}

// up to four floats from p[i...] (cnt of them; the rest 0): one 16-byte load where that is legal
__device__ __forceinline__ f32x4 multi_load(const float *p, int i, int cnt, bool vec)
{
    if (vec && cnt == 4) return *(const f32x4 *)(p + i);
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < cnt) v[j] = p[i + j];
    return v;
}

__device__ __forceinline__ void multi_store(float *p, int i, int cnt, bool vec, f32x4 v)
{
    if (vec && cnt == 4) {
        *(f32x4 *)(p + i) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < cnt) p[i + j] = v[j];
}

__global__ __launch_bounds__(kMultiThreads) void multi_sqnorm_kernel(MultiTable<1> t, double *partials, int64_t base)
{
    __shared__ double red[kMultiThreads];
    const MultiChunk c = multi_chunk(t);
    const float *g = (const float *)t.ptr[0][c.k] + c.off;
    const int tid = threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < kMultiRounds; ++r) {
        const int i = 4 * (tid + r * kMultiThreads);
        if (i >= c.n) break;
        const int cnt = c.n - i < 4 ? c.n - i : 4;
        const f32x4 v = multi_load(g, i, cnt, c.vec);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) acc += (double)v[j] * (double)v[j];
    }
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int w = kMultiThreads / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) partials[base + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kMultiThreads) void multi_norm_finalize_kernel(const double *partials, int64_t n, float max_norm,
                                                                            float *norm_coef)
{
    __shared__ double tile[kMultiThreads];
    const int tid = threadIdx.x;
    double sum = 0.0;                                            // thread 0's: the partials in index order
    for (int64_t p0 = 0; p0 < n; p0 += kMultiThreads) {
        if (p0 + tid < n) tile[tid] = partials[p0 + tid];
        __syncthreads();
        if (tid == 0) {
            const int m = (int)(n - p0 < kMultiThreads ? n - p0 : kMultiThreads);
            for (int i = 0; i < m; ++i) sum += tile[i];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double norm = sqrt(sum);
        const double c = (double)max_norm / (norm + 1e-6);
        norm_coef[0] = (float)norm;
        norm_coef[1] = (float)(c > 1.0 ? 1.0 : c);               // a NaN stays a NaN, as torch's clamp keeps it
    }
}

// torch.optim.Adam, the single-tensor form, on one element:
//   exp_avg.lerp_(grad, 1 - beta1)                     m + w (g - m) for w < 0.5, else g - (g - m)(1 - w): ATen's lerp
//   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
//   denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps);  param.addcdiv_(exp_avg, denom, value=-step_size)
// every operation rounded on its own
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const MultiAdamScalars &s)
{
    const float d = g - m;
    m = s.one_minus_beta1 < 0.5f ? m + s.one_minus_beta1 * d : g - d * (1.0f - s.one_minus_beta1);
    v = v * s.beta2 + (s.one_minus_beta2 * g) * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p + s.neg_step_size * (m / denom);
}

__global__ __launch_bounds__(kMultiThreads) void multi_adam_kernel(MultiTable<4> t, const float *norm_coef, MultiAdamScalars s)
{
    const MultiChunk c = multi_chunk(t);
    float *p = (float *)t.ptr[0][c.k] + c.off, *g = (float *)t.ptr[1][c.k] + c.off;
    float *m = (float *)t.ptr[2][c.k] + c.off, *v = (float *)t.ptr[3][c.k] + c.off;
    const bool clip = norm_coef != nullptr;
    const float coef = clip ? norm_coef[1] : 1.0f;
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < kMultiRounds; ++r) {
        const int i = 4 * (tid + r * kMultiThreads);
        if (i >= c.n) break;
        const int cnt = c.n - i < 4 ? c.n - i : 4;
        f32x4 pv = multi_load(p, i, cnt, c.vec), gv = multi_load(g, i, cnt, c.vec);
        f32x4 mv = multi_load(m, i, cnt, c.vec), vv = multi_load(v, i, cnt, c.vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (clip) gv[j] = gv[j] * coef;
            float pj = pv[j], mj = mv[j], vj = vv[j];
            adam_element(pj, gv[j], mj, vj, s);
            pv[j] = pj, mv[j] = mj, vv[j] = vj;
        }
        if (clip) multi_store(g, i, cnt, c.vec, gv);             // the clipped gradient, as clip_grad_norm_ leaves it
        multi_store(m, i, cnt, c.vec, mv);
        multi_store(v, i, cnt, c.vec, vv);
        multi_store(p, i, cnt, c.vec, pv);
    }
}

__global__ __launch_bounds__(kMultiThreads) void multi_ema_kernel(MultiTable<2> t, float s, float one_minus_s)
{
    const MultiChunk c = multi_chunk(t);
    float *dst = (float *)t.ptr[0][c.k] + c.off;
    const float *src = (const float *)t.ptr[1][c.k] + c.off;
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < kMultiRounds; ++r) {
        const int i = 4 * (tid + r * kMultiThreads);
        if (i >= c.n) break;
        const int cnt = c.n - i < 4 ? c.n - i : 4;
        f32x4 dv = multi_load(dst, i, cnt, c.vec);
        const f32x4 sv = multi_load(src, i, cnt, c.vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = dv[j] * s, b = sv[j] * one_minus_s;
            dv[j] = a + b;
        }
        multi_store(dst, i, cnt, c.vec, dv);
    }
}

hipError_t launch_multi_sqnorm(const MultiTable<1> &t, double *partials, int64_t base, hipStream_t stream)
{
    hipLaunchKernelGGL(multi_sqnorm_kernel, dim3((unsigned)t.first[t.count]), dim3(kMultiThreads), 0, stream, t, partials, base);
    return hipGetLastError();
}

hipError_t launch_multi_norm_finalize(const double *partials, int64_t n, float max_norm, float *norm_coef, hipStream_t stream)
{
    hipLaunchKernelGGL(multi_norm_finalize_kernel, dim3(1), dim3(kMultiThreads), 0, stream, partials, n, max_norm, norm_coef);
    return hipGetLastError();
}

hipError_t launch_multi_adam(const MultiTable<4> &t, const float *norm_coef, const MultiAdamScalars &s, hipStream_t stream)
{
    hipLaunchKernelGGL(multi_adam_kernel, dim3((unsigned)t.first[t.count]), dim3(kMultiThreads), 0, stream, t, norm_coef, s);
    return hipGetLastError();
}

hipError_t launch_multi_ema(const MultiTable<2> &t, float s, float one_minus_s, hipStream_t stream)
{
    hipLaunchKernelGGL(multi_ema_kernel, dim3((unsigned)t.first[t.count]), dim3(kMultiThreads), 0, stream, t, s, one_minus_s);
    return hipGetLastError();
}

}  // namespace ntm
