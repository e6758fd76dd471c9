// The low-latency exact-fp32 GRU-HS[64] step, defined ONCE for gru_lat_kernel (gru_lat.hip: inference) and
// gru_train_fwd_kernel (gru_train.hip: the forward that saves its activations).  Both kernels build their step from the
// pieces below -- the pre-scaled lane constants, the gate evaluation, the head sum, the parity unroller and the epilogue --
// so their y and final h are the same bits because they are the same code.  What a kernel adds around them is its own:
// which barrier closes the step, who does the head, how the x tiles arrive, and the saves.
//
// Rounds 1-4 cut the step four ways along K BETWEEN the waves (wave w, lane u = unit u: columns 16w .. 16w+15 of all 192 rows):
// that needs TWO LDS round trips per step -- the partial sums out / in around the barrier, then each wave's private copy of h
// out / in (every wave evaluated all 64 gates redundantly) -- 342 ns per step.  Round 5: wave w owns units 16w .. 16w+15
// outright: lane l = 4 ul + kq holds the K quarter kq of unit 16w + ul for the three gates (48 weights, as before), the four quarters of a unit meet by two DPP quad_perm adds (every
// lane of the quad gets the same bits), the quad evaluates the gates redundantly and lane kq = 0 publishes h_t -- ONE LDS
// round trip per step: write h_t -> barrier -> four broadcast ds_read_b128 of the K quarter (h double-buffered by step parity,
// so one barrier orders both the reads of h_{t-1} and the writes of h_t).  The head: the wave on duty (t mod 4) reads all 64
// values of h_{t-1} from the same buffer (lane = unit) and sums w_o . h by DPP in the shadow of the K-quarter reads, one sample
// behind the recurrence -- on a fifth wave of its own when the workgroup has a CU to itself.  242-246 ns per step for B <= 256
// (342-344 before), 352 at B = 512 (426), 578 at B = 1024 (692).
// x and y move in 256-sample tiles through LDS (coalesced global accesses); the tile housekeeping sits between runs of steps.
#pragma once
#include "ntm_common.h"

#include <type_traits>

namespace ntm {

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace lat {

constexpr int LT = 256;                  // samples per x / y tile
constexpr float LOG2E = 1.44269504088896340736f;
constexpr float SRZ = -LOG2E, SN = 2.0f * LOG2E;   // scale of the r and z rows (sigma on exp2) / of the n rows (tanh on exp2)

// A workgroup barrier that orders LDS only: global stores and loads in flight (the flush of the training forward's saves, the
// backward's prefetch) are not drained by it, as they would be by the vmcnt(0) of a full __syncthreads().
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_shift_add(float v)
{
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false);
    return v + __builtin_bit_cast(float, moved);
}

// Sum over the 64 lanes on the VALU (row_shr / row_bcast scan, no LDS round trips); total valid in lane 63.
__device__ __forceinline__ float wave_sum_lane63(float v)
{
    v = dpp_shift_add<0x111, 0xf>(v);  // row_shr:1
    v = dpp_shift_add<0x112, 0xf>(v);  // row_shr:2
    v = dpp_shift_add<0x114, 0xf>(v);  // row_shr:4
    v = dpp_shift_add<0x118, 0xf>(v);  // row_shr:8
    v = dpp_shift_add<0x142, 0xa>(v);  // row_bcast:15 -> rows 1,3
    v = dpp_shift_add<0x143, 0xc>(v);  // row_bcast:31 -> rows 2,3
    return v;
}

template <int PERM>
__device__ __forceinline__ float quad_add(float v)
{
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), PERM, 0xf, 0xf, true);
    return v + __builtin_bit_cast(float, o);
}

// What lane kq of unit u's quad keeps in registers: its K quarter of the three W_hh rows and the unit's input weights and
// biases, pre-scaled so that the gates need no multiply in front of v_exp_f32.
struct Lane {
    f32x2 Wr[8], Wz[8], Wn[8];
    float wir, wiz, win, br, bz, bin_, bhn;

    __device__ __forceinline__ void load(const GruArgs &a, const int u, const int kq)
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float *pr = a.w_hh + (size_t)(0 * kH + u) * kH + 16 * kq + 2 * k;
            const float *pz = a.w_hh + (size_t)(1 * kH + u) * kH + 16 * kq + 2 * k;
            const float *pn = a.w_hh + (size_t)(2 * kH + u) * kH + 16 * kq + 2 * k;
            Wr[k] = (f32x2){pr[0] * SRZ, pr[1] * SRZ};
            Wz[k] = (f32x2){pz[0] * SRZ, pz[1] * SRZ};
            Wn[k] = (f32x2){pn[0] * SN, pn[1] * SN};
        }
        wir = a.w_ih[u] * SRZ, wiz = a.w_ih[kH + u] * SRZ, win = a.w_ih[2 * kH + u] * SN;
        br = (a.b_ih[u] + a.b_hh[u]) * SRZ, bz = (a.b_ih[kH + u] + a.b_hh[kH + u]) * SRZ;
        bin_ = a.b_ih[2 * kH + u] * SN, bhn = a.b_hh[2 * kH + u] * SN;
    }
};

// The gates of the lane's unit at one step from the K quarter h0 .. h3 of h_{t-1} and the sample x: r, z, n and the scaled
// gh_n = SN (W_hn h_{t-1} + b_hn) that the training forward saves.  The caller forms h_t = fma(z, h_{t-1} - n, n).
__device__ __forceinline__ void gates(const Lane &c, const f32x4 &h0, const f32x4 &h1, const f32x4 &h2, const f32x4 &h3, const float x,
                                      float &r, float &z, float &n, float &gh)
{
#pragma clang fp contract(off)
    const f32x2 hq[8] = {{h0[0], h0[1]}, {h0[2], h0[3]}, {h1[0], h1[1]}, {h1[2], h1[3]},
                         {h2[0], h2[1]}, {h2[2], h2[3]}, {h3[0], h3[1]}, {h3[2], h3[3]}};
    f32x2 ar0 = c.Wr[0] * hq[0], ar1 = c.Wr[1] * hq[1], az0 = c.Wz[0] * hq[0], az1 = c.Wz[1] * hq[1];
    f32x2 an0 = c.Wn[0] * hq[0], an1 = c.Wn[1] * hq[1];
#pragma unroll
    for (int k = 2; k < 8; k += 2) {
        ar0 = __builtin_elementwise_fma(c.Wr[k], hq[k], ar0); ar1 = __builtin_elementwise_fma(c.Wr[k + 1], hq[k + 1], ar1);
        az0 = __builtin_elementwise_fma(c.Wz[k], hq[k], az0); az1 = __builtin_elementwise_fma(c.Wz[k + 1], hq[k + 1], az1);
        an0 = __builtin_elementwise_fma(c.Wn[k], hq[k], an0); an1 = __builtin_elementwise_fma(c.Wn[k + 1], hq[k + 1], an1);
    }
    const f32x2 sr = ar0 + ar1, sz = az0 + az1, sn = an0 + an1;
    // the unit's four K quarters: quad_perm [1,0,3,2] then [2,3,0,1] -- ((q0 + q1) + (q2 + q3)) in every lane of the quad
    const float qr = quad_add<0x4E>(quad_add<0xB1>(sr[0] + sr[1]));
    const float qz = quad_add<0x4E>(quad_add<0xB1>(sz[0] + sz[1]));
    const float qn = quad_add<0x4E>(quad_add<0xB1>(sn[0] + sn[1]));
    const float cr = __builtin_fmaf(c.wir, x, c.br), cz = __builtin_fmaf(c.wiz, x, c.bz), gi = __builtin_fmaf(c.win, x, c.bin_);
    const float pr_ = cr + qr, pz_ = cz + qz;
    gh = c.bhn + qn;
    r = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(pr_));
    z = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(pz_));
    const float en = __builtin_amdgcn_exp2f(__builtin_fmaf(r, gh, gi));
    n = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + en), 1.0f);
}

// The head y = w_o . h + b_o, evaluated by ONE wave (head weights by LANE: lane = unit) one sample behind the recurrence.
// Its arithmetic does not depend on which wave evaluates it.
struct Head {
    float wo_l, bo;

    __device__ __forceinline__ void load(const GruArgs &a, const int l)
    {
        bo = a.b_o ? a.b_o[0] : 0.0f;
        wo_l = a.w_o[l];
    }
    // all 64 values of h from the exchange buffer, DPP sum: valid in lane 63
    __device__ __forceinline__ float value(const float *h, const int l) const
    {
#pragma clang fp contract(off)
        return wave_sum_lane63(wo_l * h[l]) + bo;
    }
    // during step ph of the tile in buffer tb, h = h_{t-1}: y of sample t-1 (for ph = 0 the last of the previous tile)
    __device__ __forceinline__ void sample_before(const float *h, const int l, float (*yt)[LT], const int tb, const int ph) const
    {
        const float yv = value(h, l);
        if (l == 63) { if (ph > 0) yt[tb][ph - 1] = yv; else yt[tb ^ 1][LT - 1] = yv; }
    }
};

using P0 = std::integral_constant<int, 0>;
using P1 = std::integral_constant<int, 1>;

// steps [p0, p1) of a tile, two at a time with the step parity known at compile time (tiles are 256 steps, so the parity
// of t is that of p): step(p, P0{} or P1{}, args...)
template <class Step, class... Args>
__device__ __forceinline__ void run(int p0, const int p1, Step &step, const Args... args)
{
    if (p0 < p1 && (p0 & 1)) { step(p0, P1{}, args...); ++p0; }
    for (; p0 + 1 < p1; p0 += 2) { step(p0, P0{}, args...); step(p0 + 1, P1{}, args...); }
    if (p0 < p1) step(p0, P0{}, args...);
}

// After the last step, by the whole workgroup: the head of the last sample on the wave `last_head` (h_{T-1} sits in
// hb[T & 1]) and the y tile(s) not yet written out.  The h_state write-back stays one line in each kernel: formed in here,
// its lane predicate was computed ahead of the step loop and the compiler scheduled gru_lat_kernel<true>'s step differently.
__device__ __forceinline__ void finish(const GruArgs &a, const Head &hd, const float (*hb)[kH], float (*yt)[LT], const bool last_head)
{
    const int tid = threadIdx.x, l = tid & 63;
    const int64_t s = blockIdx.x;
    const int64_t T = a.T;
    float *ys = a.y + s * a.ys;
    if (T > 0 && last_head) {
        const float yv = hd.value(hb[(int)(T & 1)], l);
        if (l == 63) yt[(int)(((T - 1) >> 8) & 1)][(int)((T - 1) & (LT - 1))] = yv;
    }
    __syncthreads();
    const int64_t last0 = ((T - 1) >> 8) * LT;
    if (T > 0 && tid < LT) {
        if (last0 + tid < T) ys[last0 + tid] = yt[(last0 >> 8) & 1][tid];
        if (last0 >= LT && (T - 1 - last0) < 2) ys[last0 - LT + tid] = yt[((last0 >> 8) & 1) ^ 1][tid];
    }
}

}   // namespace lat
}   // namespace ntm
