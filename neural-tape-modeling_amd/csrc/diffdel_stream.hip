// K1s: one block of DiffDelRNN(1, 64, 1, skip=False) for block-by-block streaming (harness.BlockStreamer): the low-latency
// recurrence and the time-varying delay line in ONE launch, one workgroup per stream, with the delay line's history in a
// per-stream RING in device memory instead of the reference's shifted buffer -- a call moves O(block) floats of delay state
// per stream where ntm_delay_forward rewrites all D of them.
//
// Recurrence: the step of gru_lat_step.h (Lane, Head, gates, run, finish) with gru_lat_kernel's glue around it -- the same
// barrier, the same head duty (a fifth wave when the workgroup has a CU to itself), the same x / y tiles -- so pre_d and h_T
// are the bits of kernel_variant "lat".  The head has no bias.
//
// Delay line: ring[s][C], C a power of two >= D + block, and a sample counter pos[s] (int64, on the device) that only the
// stream's own workgroup reads and advances -- the host passes no position, so the launch can be captured and replayed.  Sample
// i of the stream (counted from the ring's origin) lives at ring[i & (C - 1)]; the block's pre_d goes to pos .. pos + block - 1
// and the tap the reference reads at z[D + n - m], z = [buffer, pre_d], is sample pos + n - m.  y[n] is delay_math.h's
// delay_sample_at() -- the general form, with the mf > D cut, the tap order and the zero-weight skip -- behind a ring fetch:
// the bits of ntm_delay_forward.
//
// Ordering inside the workgroup: the ring is WRITTEN, then fenced and barriered, then READ.  Every y tile leaves LDS for the
// ring (and for pre_d) where gru_lat_kernel flushes it; the last one or two tiles are copied from LDS behind finish()'s
// barrier; one workgroup-scope release fence, the barrier and an acquire fence (ring_written_barrier() below: what
// __syncthreads() is) separate those stores from the tap loads.  All waves of a workgroup run on one CU and share its vector
// L1, which takes that CU's accesses in the order they were issued, and no ring line is read in a launch before that barrier,
// so plain loads behind it see the new samples (for this target the compiler's release at workgroup scope is the barrier
// itself: it adds no wait for the stores' acknowledgements, and none is needed).  No other workgroup ever touches this ring, so
// nothing wider than workgroup scope is involved: no atomics, no spin waits, no grid-wide synchronisation.  (Taps in LDS would
// save the round trip through L2 only while block <= 512 and would still need the ring for the history.)
// Where the caller wants no pre_d, finish() parks the last tile(s) in the stream's y row; the delay phase overwrites them
// behind the same barrier.
#include "gru_lat_step.h"
#include "delay_math.h"

namespace ntm {
namespace {

using namespace lat;

// global stores of this workgroup (the ring, the pre_d rows) before it, loads and stores of the same words after it
__device__ __forceinline__ void ring_written_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool HEADW>
__global__ __launch_bounds__(HEADW ? 320 : 256) void diffdel_stream_kernel(StreamArgs sa)
{
#pragma clang fp contract(off)
    const GruArgs &a = sa.g;
    __shared__ __attribute__((aligned(16))) float hb[2][kH];            // h by step parity
    __shared__ float xt[2][LT];
    __shared__ float yt[2][LT];

    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ul = l >> 2, kq = l & 3;
    const bool head_wave = HEADW && w == 4;
    const int u = 16 * (w & 3) + ul;
    const int64_t s = blockIdx.x;
    const int64_t T = a.T;
    const float *xs = a.x + s * a.xs;
    float *ys = a.y + s * a.ys;                                         // pre_d rows
    const int64_t mask = sa.mask;
    float *const ring = sa.ring + s * (mask + 1);
    const int64_t p0 = sa.pos[s];                                       // sample index of the block's first sample
    const float *db = a.dd + s * sa.ds;
    const float d_first = tid < T ? db[tid] : 0.0f;                     // the delay phase's first load, under the recurrence

    Lane c;
    c.load(a, u, kq);
    Head hd;
    hd.load(a, l);
    float hold = a.h_state[s * kH + u];

    if (kq == 0 && !head_wave) hb[0][u] = hold;
    if (tid < LT && tid < T) xt[0][tid] = xs[tid];
    float xnext = (tid < LT && LT + tid < T) ? xs[LT + tid] : 0.0f;
    __syncthreads();

    // gru_lat_kernel's step: hb[t & 1] holds h_{t-1}; tb = tile parity (of the x / y buffers)
    const float *const hq_rd = &hb[0][16 * kq];
    float *const hu_wr = &hb[0][u];
    auto step = [&](const int ph, auto par_c, const int tb) {
        constexpr int par = decltype(par_c)::value;
        if constexpr (HEADW) {
            if (head_wave) {
                hd.sample_before(hb[par], l, yt, tb, ph);
                __syncthreads();
                return;
            }
        }
        const f32x4 h0 = *(const f32x4 *)(hq_rd + par * kH + 0), h1 = *(const f32x4 *)(hq_rd + par * kH + 4);
        const f32x4 h2 = *(const f32x4 *)(hq_rd + par * kH + 8), h3 = *(const f32x4 *)(hq_rd + par * kH + 12);
        const float x = xt[tb][ph];
        if constexpr (!HEADW) {
            if ((ph & 3) == w) hd.sample_before(hb[par], l, yt, tb, ph);
        }
        float r, z, n, gh;
        gates(c, h0, h1, h2, h3, x, r, z, n, gh);
        hold = __builtin_fmaf(z, hold - n, n);
        hu_wr[(par ^ 1) * kH] = hold;
        __syncthreads();
    };

    for (int64_t tile0 = 0; tile0 < T; tile0 += LT) {
        const int ns = (int)((T - tile0) < LT ? (T - tile0) : LT);
        const int tb = (int)((tile0 >> 8) & 1);
        run(0, ns < 3 ? ns : 3, step, tb);
        if (ns > 2 && tile0 >= LT && tid < LT) {                        // previous y tile is complete: to pre_d and to the ring
            const float v = yt[tb ^ 1][tid];
            ys[tile0 - LT + tid] = v;
            ring[(p0 + tile0 - LT + tid) & mask] = v;
        }
        run(3, ns < 129 ? ns : 129, step, tb);
        if (ns > 128 && tid < LT) {
            xt[tb ^ 1][tid] = xnext;
            const int64_t nx = tile0 + 2 * LT + tid;
            xnext = nx < T ? xs[nx] : 0.0f;
        }
        run(129, ns, step, tb);
    }
    finish(a, hd, hb, yt, HEADW ? head_wave : w == 0);
    if (kq == 0 && !head_wave) a.h_state[s * kH + u] = hold;

    // finish()'s barrier is behind every thread: yt holds the last tile and, whole, the one before it.  The last tile goes to
    // the ring here; the one before it too (again, if the loop above already sent it: the same values)
    if (tid < LT) {
        const int64_t last0 = ((T - 1) >> 8) * LT;
        const int lb = (int)((last0 >> 8) & 1);
        if (last0 + tid < T) ring[(p0 + last0 + tid) & mask] = yt[lb][tid];
        if (last0 >= LT) ring[(p0 + last0 - LT + tid) & mask] = yt[lb ^ 1][tid];
    }
    ring_written_barrier();                                             // see the file header

    // delay phase: the workgroup's threads stride over the block; d in, y out, both coalesced
    float *yb = a.yd + s * a.ys;
    const bool own_pre = a.y != a.yd;                                   // else the y row already holds pre_d (what a warm-up returns)
    const float Dmax = (float)a.D;
    const int nthr = HEADW ? 320 : 256;
    bool bad = false;
    for (int64_t n = tid; n < T; n += nthr) {
        const float dn = n == tid ? d_first : db[n];
        bad |= !(dn <= Dmax);                                           // NaN too
        if (!a.warmup) yb[n] = delay_sample_ring(ring, mask, a.D, p0 + n, dn);
        else if (own_pre) yb[n] = ring[(p0 + n) & mask];
    }
    if (bad && a.dl_flag) *a.dl_flag = 1;                               // every writer stores the same word
    if (tid == 0) sa.pos[s] = p0 + T;
}

// ring <- the reference's buffer (oldest sample first) as samples 0 .. D-1, pos <- D
__global__ __launch_bounds__(256) void diffdel_stream_seed_kernel(const float *buf, float *ring, int64_t *pos, int D, int64_t mask)
{
    const int64_t s = blockIdx.x;
    for (int i = threadIdx.x; i < D; i += 256) ring[s * (mask + 1) + i] = buf[s * D + i];
    if (threadIdx.x == 0) pos[s] = D;
}

// the reference's buffer back: the D samples before pos
__global__ __launch_bounds__(256) void diffdel_stream_export_kernel(const float *ring, const int64_t *pos, float *buf, int D, int64_t mask)
{
    const int64_t s = blockIdx.x;
    const int64_t first = pos[s] - D;
    for (int i = threadIdx.x; i < D; i += 256) buf[s * D + i] = ring[s * (mask + 1) + ((first + i) & mask)];
}

}   // namespace

// HEADW by the stream count, as launch_gru_lat chooses it
hipError_t launch_diffdel_stream(const StreamArgs &sa, hipStream_t stream)
{
    if (sa.g.B == 0 || sa.g.T == 0) return hipSuccess;
    if (sa.g.B <= device_cus()) hipLaunchKernelGGL(diffdel_stream_kernel<true>, dim3((unsigned)sa.g.B), dim3(320), 0, stream, sa);
    else hipLaunchKernelGGL(diffdel_stream_kernel<false>, dim3((unsigned)sa.g.B), dim3(256), 0, stream, sa);
    return hipGetLastError();
}

hipError_t launch_diffdel_stream_seed(const float *dl_state, float *ring, int64_t *pos, int64_t B, int D, int64_t C, hipStream_t stream)
{
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(diffdel_stream_seed_kernel, dim3((unsigned)B), dim3(256), 0, stream, dl_state, ring, pos, D, C - 1);
    return hipGetLastError();
}

hipError_t launch_diffdel_stream_export(const float *ring, const int64_t *pos, float *dl_state, int64_t B, int D, int64_t C,
                                        hipStream_t stream)
{
    if (B == 0 || D == 0) return hipSuccess;
    hipLaunchKernelGGL(diffdel_stream_export_kernel, dim3((unsigned)B), dim3(256), 0, stream, ring, pos, dl_state, D, C - 1);
    return hipGetLastError();
}

}   // namespace ntm
