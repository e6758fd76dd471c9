// The hinge / mean heads of the adversarial losses (code/critics.py train_crit / train_gen) on the K outputs of a critic, as two
// entry points: ntm_adv_head_forward (the loss) and ntm_adv_head_backward (its gradient at every output).  Streaming kernels,
// 16 B per lane, no MFMA, no atomics.
//
// An output k is a contiguous [rows, elems[k]] fp32 tensor.  The critic mode cuts it at row n_fake into a fake half with the
// terms relu(fp32(1 + o)) and a real half with relu(fp32(1 - o)), each with a mean of its own; the generator mode takes the
// mean of o over all rows and negates it.  A (half, output) pair is a SEGMENT: a contiguous run of floats with one kind of
// term.  Segments are numbered in the order the reference adds their means: the fake halves by k, then the real halves by k.
//
//   adv_head_partial_kernel   grid (chunks, segments): a 256-thread workgroup sums one chunk of NTM_ADV_HEAD_CHUNK terms of one
//                             segment in fp64 -- thread i takes the float4 groups i, i + 256, ... of the chunk in that order and
//                             the four lanes of a group in index order, then a fixed LDS tree -- into ws[segment][chunk];
//   adv_head_final_kernel     one workgroup: per segment the chunk sums in the same fixed way, one fp64 division by the segment's
//                             size, one rounding to fp32; thread 0 adds the fp32 means in segment order.
//   adv_head_backward_kernel  grid (chunks, segments): grad = sign * coef * [term > 0] with coef formed once per workgroup.
// The 16-byte accesses are made at 4-byte alignment (a real half starts wherever n_fake * elems[k] floats end), so the order of
// the sums -- and with it every bit of the result -- does not depend on where a tensor lies.
#include "ntm_common.h"

namespace ntm {

typedef float f32x4a __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte access at 4-byte alignment

constexpr int kAdvThreads = 256;
constexpr int kAdvChunk = NTM_ADV_HEAD_CHUNK;
static_assert(kAdvChunk % (4 * kAdvThreads) == 0, "a chunk is a whole number of float4 rounds of the workgroup");

enum { ADV_FAKE = 0, ADV_REAL = 1, ADV_GEN = 2 };

// segment s -> its output k, the kind of its terms, its first float within output k and its length in floats
__device__ __forceinline__ void adv_segment(const AdvHeadArgs &a, int s, int &k, int &kind, int64_t &start, int64_t &len)
{
    k = s % a.K;
    const int64_t e = a.elems[k];
    if (a.mode == NTM_ADV_HEAD_GEN) {
        kind = ADV_GEN;
        start = 0;
        len = a.rows * e;
    } else {
        kind = s / a.K;
        start = kind == ADV_REAL ? a.n_fake * e : 0;
        len = (kind == ADV_REAL ? a.rows - a.n_fake : a.n_fake) * e;
    }
}

// the term as torch forms it: the sum rounded to fp32, then relu (a NaN stays a NaN)
__device__ __forceinline__ float adv_term(float o, int kind)
{
    if (kind == ADV_GEN) return o;
    const float t = kind == ADV_FAKE ? 1.0f + o : 1.0f - o;
    return t <= 0.0f ? 0.0f : t;
}

// red[0] <- the 256 values in a fixed tree order; every thread of the workgroup calls it
__device__ __forceinline__ double adv_block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int w = kAdvThreads / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();            // red is free again
    return total;
}

__global__ __launch_bounds__(kAdvThreads) void adv_head_partial_kernel(AdvHeadArgs a, double *ws, int64_t max_chunks)
{
    __shared__ double red[kAdvThreads];
    int k, kind;
    int64_t start, len;
    const int s = blockIdx.y;
    adv_segment(a, s, k, kind, start, len);
    const int64_t c0 = (int64_t)blockIdx.x * kAdvChunk;
    if (c0 >= len) return;                                       // the same for the whole workgroup
    const int n = (int)(len - c0 < kAdvChunk ? len - c0 : kAdvChunk);
    const float *p = a.o[k] + start + c0;
    const int tid = threadIdx.x, nv = n >> 2;
    double acc = 0.0;
#pragma unroll 4
    for (int i = tid; i < nv; i += kAdvThreads) {
        const f32x4a v = *(const f32x4a *)(p + 4 * i);
        acc += (double)adv_term(v[0], kind);
        acc += (double)adv_term(v[1], kind);
        acc += (double)adv_term(v[2], kind);
        acc += (double)adv_term(v[3], kind);
    }
    const int i = 4 * nv + tid;                                  // the scalar tail: at most 3 floats
    if (i < n) acc += (double)adv_term(p[i], kind);
    const double total = adv_block_sum(acc, red);
    if (tid == 0) ws[(int64_t)s * max_chunks + blockIdx.x] = total;
}

__global__ __launch_bounds__(kAdvThreads) void adv_head_final_kernel(AdvHeadArgs a, const double *ws, int64_t max_chunks, float *loss)
{
    __shared__ double red[kAdvThreads];
    __shared__ float means[2 * NTM_ADV_HEAD_MAX_K];
    const int tid = threadIdx.x;
    const int nseg = a.mode == NTM_ADV_HEAD_GEN ? a.K : 2 * a.K;
    for (int s = 0; s < nseg; ++s) {
        int k, kind;
        int64_t start, len;
        adv_segment(a, s, k, kind, start, len);
        const int64_t nc = (len + kAdvChunk - 1) / kAdvChunk;
        double acc = 0.0;
        for (int64_t c = tid; c < nc; c += kAdvThreads) acc += ws[(int64_t)s * max_chunks + c];
        const double total = adv_block_sum(acc, red);
        if (tid == 0) means[s] = (float)(total / (double)len);   // the mean, rounded to fp32 once
    }
    __syncthreads();
    if (tid == 0) {
        // loss = 0; loss += mean (or -mean) for every segment in the reference's order, in fp32
        const bool gen = a.mode == NTM_ADV_HEAD_GEN;
        float l = gen ? -means[0] : means[0];
        for (int s = 1; s < nseg; ++s) l += gen ? -means[s] : means[s];
        loss[0] = l;
    }
}

__global__ __launch_bounds__(kAdvThreads) void adv_head_backward_kernel(AdvHeadArgs a, const float *gout)
{
    int k, kind;
    int64_t start, len;
    adv_segment(a, blockIdx.y, k, kind, start, len);
    const int64_t c0 = (int64_t)blockIdx.x * kAdvChunk;
    if (c0 >= len) return;
    const int n = (int)(len - c0 < kAdvChunk ? len - c0 : kAdvChunk);
    const float *p = a.o[k] + start + c0;
    float *g = a.g[k] + start + c0;
    // the mean's adjoint as torch's division of a tensor by a host scalar forms it: gout times the fp32 reciprocal of the size
    const float coef = gout[0] * (1.0f / (float)len);
    const float sc = kind == ADV_FAKE ? coef : -coef;
    const int tid = threadIdx.x, nv = n >> 2;
#pragma unroll 4
    for (int i = tid; i < nv; i += kAdvThreads) {
        const f32x4a v = *(const f32x4a *)(p + 4 * i);
        f32x4a r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = kind == ADV_FAKE ? 1.0f + v[j] : 1.0f - v[j];
            r[j] = (kind != ADV_GEN && t <= 0.0f) ? 0.0f : sc;       // torch's mask: zero at a term of exactly 0
        }
        *(f32x4a *)(g + 4 * i) = r;
    }
    const int i = 4 * nv + tid;
    if (i < n) {
        const float t = kind == ADV_FAKE ? 1.0f + p[i] : 1.0f - p[i];
        g[i] = (kind != ADV_GEN && t <= 0.0f) ? 0.0f : sc;
    }
}

int64_t adv_head_chunks(const AdvHeadArgs &a)
{
    int64_t most = 0;
    for (int k = 0; k < a.K; ++k) {
        const int64_t f = a.mode == NTM_ADV_HEAD_GEN ? a.rows : a.n_fake, r = a.mode == NTM_ADV_HEAD_GEN ? 0 : a.rows - a.n_fake;
        const int64_t len = (f > r ? f : r) * a.elems[k];
        const int64_t c = (len + kAdvChunk - 1) / kAdvChunk;
        most = c > most ? c : most;
    }
    return most;
}

hipError_t launch_adv_head_forward(const AdvHeadArgs &a, double *ws, float *loss, hipStream_t stream)
{
    const int64_t chunks = adv_head_chunks(a);
    const int nseg = a.mode == NTM_ADV_HEAD_GEN ? a.K : 2 * a.K;
    hipLaunchKernelGGL(adv_head_partial_kernel, dim3((unsigned)chunks, (unsigned)nseg), dim3(kAdvThreads), 0, stream, a, ws, chunks);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(adv_head_final_kernel, dim3(1), dim3(kAdvThreads), 0, stream, a, ws, chunks, loss);
    return hipGetLastError();
}

hipError_t launch_adv_head_backward(const AdvHeadArgs &a, const float *gout, hipStream_t stream)
{
    const int64_t chunks = adv_head_chunks(a);
    const int nseg = a.mode == NTM_ADV_HEAD_GEN ? a.K : 2 * a.K;
    hipLaunchKernelGGL(adv_head_backward_kernel, dim3((unsigned)chunks, (unsigned)nseg), dim3(kAdvThreads), 0, stream, a, gout);
    return hipGetLastError();
}

}  // namespace ntm
