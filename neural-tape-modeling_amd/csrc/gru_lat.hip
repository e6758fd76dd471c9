// K1e: low-latency GRU kernel for SMALL batches (NTM_GRU_LAT; NTM_GRU_AUTO picks it when there are too few
// streams to fill the matrix-pipe kernel: the warm-start of predict() -- ONE stream, code/model.py:58-65 -- and
// evaluation batches like BASELINE configs[0], 16 x 8192, or the reference's real test sets: dozens of 10-second segments).
//
// The MFMA2 kernel spends 2012 cycles per step on 16 streams at once and needs 16 streams per workgroup to be
// efficient; with B streams only ceil(B/16) CUs work.  Here ONE workgroup (4 waves) advances ONE stream, so B
// streams occupy B workgroups (several per CU); gru_lat_step.h says how the step is cut and holds its pieces, which the
// training forward (gru_train.hip) shares.
// Exact fp32 like the other exact kernels (different summation order: K split in four).
#include "gru_lat_step.h"

namespace ntm {
namespace {

using namespace lat;

// HEADW: a fifth wave does the head (B <= the number of CUs: a workgroup has a CU to itself); without it the head is a duty
// that rotates among the four compute waves (more streams than CUs: a fifth wave per workgroup costs occupancy)
//
// REP (ntm_gru_forward_replicas): R models in one launch.  The streams are stacked replica-major, stream s belongs to replica
// s / a.bper, and the six parameter pointers are the [R, ...] stacks gru_train_fwd_kernel<true> takes -- the workgroup moves them
// to its replica's slice before the weight load (a scalar division and six scalar adds, once); everything behind that is the
// same code, so every replica's y and h_state are the bits of the REP = false kernel on its slice.  REP = false reads no bper.
template <bool HEADW, bool REP = false>
__global__ __launch_bounds__(HEADW ? 320 : 256) void gru_lat_kernel(GruArgs a)
{
#pragma clang fp contract(off)
    if constexpr (REP) {
        const size_t rep = blockIdx.x / a.bper;
        a.w_ih += rep * (3 * kH); a.w_hh += rep * (3 * kH * kH); a.b_ih += rep * (3 * kH); a.b_hh += rep * (3 * kH);
        a.w_o += rep * kH;
        if (a.b_o) a.b_o += rep;
    }
    __shared__ __attribute__((aligned(16))) float hb[2][kH];            // h by step parity
    __shared__ float xt[2][LT];
    __shared__ float yt[2][LT];

    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ul = l >> 2, kq = l & 3;
    const bool head_wave = HEADW && w == 4;                             // the fifth wave: head + nothing else (see the step)
    const int u = 16 * (w & 3) + ul;                                    // this quad's hidden unit (the head wave: unused)
    const int64_t s = blockIdx.x;
    const int64_t T = a.T;
    const float *xs = a.x + s * a.xs;
    float *ys = a.y + s * a.ys;

    Lane c;
    c.load(a, u, kq);
    Head hd;
    hd.load(a, l);                                                      // head weights by LANE: the wave on duty sums all 64 units
    float hold = a.h_state ? a.h_state[s * kH + u] : 0.0f;

    if (kq == 0 && !head_wave) hb[0][u] = hold;
    if (tid < LT && tid < T) xt[0][tid] = xs[tid];
    float xnext = (tid < LT && LT + tid < T) ? xs[LT + tid] : 0.0f;
    __syncthreads();

    // step t = tile + ph: hb[t & 1] holds h_{t-1}; tb = tile parity (of the x / y buffers)
    const float *const hq_rd = &hb[0][16 * kq];                         // this lane's K quarter / unit in buffer 0
    float *const hu_wr = &hb[0][u];                                     // (buffer 1: a compile-time + kH in the unrolled loop)
    auto step = [&](const int ph, auto par_c, const int tb) {
        constexpr int par = decltype(par_c)::value;                     // == t & 1 (tiles are 256 steps): compile time
        if constexpr (HEADW) {
            if (head_wave) {             // on a wave of its own, off the compute waves' critical path: 246 ns per step instead of 287
                hd.sample_before(hb[par], l, yt, tb, ph);
                __syncthreads();
                return;
            }
        }
        const f32x4 h0 = *(const f32x4 *)(hq_rd + par * kH + 0), h1 = *(const f32x4 *)(hq_rd + par * kH + 4);
        const f32x4 h2 = *(const f32x4 *)(hq_rd + par * kH + 8), h3 = *(const f32x4 *)(hq_rd + par * kH + 12);
        const float x = xt[tb][ph];
        if constexpr (!HEADW) {          // as a duty that rotates among the compute waves, in the shadow of the reads above
            if ((ph & 3) == w) hd.sample_before(hb[par], l, yt, tb, ph);
        }
        float r, z, n, gh;
        gates(c, h0, h1, h2, h3, x, r, z, n, gh);
        hold = __builtin_fmaf(z, hold - n, n);
        hu_wr[(par ^ 1) * kH] = hold;                      // all four lanes of the quad store the same bits to the same word
        __syncthreads();                                   // the step's only barrier
    };

    for (int64_t tile0 = 0; tile0 < T; tile0 += LT) {
        const int ns = (int)((T - tile0) < LT ? (T - tile0) : LT);
        const int tb = (int)((tile0 >> 8) & 1);
        run(0, ns < 3 ? ns : 3, step, tb);
        if (ns > 2 && tile0 >= LT && tid < LT) ys[tile0 - LT + tid] = yt[tb ^ 1][tid];      // previous y tile is complete
        run(3, ns < 129 ? ns : 129, step, tb);
        if (ns > 128 && tid < LT) {
            xt[tb ^ 1][tid] = xnext;
            const int64_t nx = tile0 + 2 * LT + tid;
            xnext = nx < T ? xs[nx] : 0.0f;
        }
        run(129, ns, step, tb);
    }
    finish(a, hd, hb, yt, HEADW ? head_wave : w == 0);
    if (a.h_state && kq == 0 && !head_wave) a.h_state[s * kH + u] = hold;
}

}   // namespace

hipError_t launch_gru_lat(const GruArgs &a, hipStream_t stream)
{
    if (a.B == 0) return hipSuccess;
    if (a.B <= device_cus()) hipLaunchKernelGGL(gru_lat_kernel<true>, dim3((unsigned)a.B), dim3(320), 0, stream, a);
    else hipLaunchKernelGGL(gru_lat_kernel<false>, dim3((unsigned)a.B), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// R * bper streams of R stacked replicas: HEADW by the TOTAL stream count, as above (a workgroup has a CU to itself or not
// whichever replica it belongs to)
hipError_t launch_gru_lat_replicas(const GruArgs &a, hipStream_t stream)
{
    if (a.B == 0) return hipSuccess;
    if (a.bper == 0) return hipErrorInvalidValue;
    if (a.B <= device_cus()) hipLaunchKernelGGL((gru_lat_kernel<true, true>), dim3((unsigned)a.B), dim3(320), 0, stream, a);
    else hipLaunchKernelGGL((gru_lat_kernel<false, true>), dim3((unsigned)a.B), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}   // namespace ntm
