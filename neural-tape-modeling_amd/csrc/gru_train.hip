// Training kernels for GRU-HS[64] (input_size = output_size = 1, no skip, exact fp32): what RNN.train_epoch needs
// (code/model.py:90-161) -- the forward with its activations saved, the backward through time (BPTT), the deterministic
// reduction of the per-stream gradients, and the adjoints of the ESR / DCPreESR losses (code/train.py:173-176).  The reduction
// and the loss adjoints exist once, for R stacked replicas; one model is their R = 1 (one grid row, bper = B).
//
// GRU as torch defines it, with gh_n = W_hn h_{t-1} + b_hn:
//   r, z = sigma(.),  n = tanh(W_in x + b_in + r o gh_n),  h_t = n + z o (h_{t-1} - n),  y_t = w_o . h_t + b_o.
//
// Workspace of the forward (and input of the backward): ws[s][t][j][u], j = 0..4 = h_{t-1}, r, z, n, gh_n (unscaled), fp32.
// Per-stream gradient partials: part[s][NTM_TRAIN_GRAD_FLOATS] in the order w_ih | w_hh | b_ih | b_hh | w_o | b_o (12929).
#include "gru_lat_step.h"

namespace ntm {
namespace {

using namespace lat;                     // the low-latency step and its DPP helpers, shared with gru_lat.hip

constexpr int NSAVE = 5;                 // h_{t-1}, r, z, n, gh_n
constexpr int OFF_WHH = 3 * kH, OFF_BIH = OFF_WHH + 3 * kH * kH, OFF_BHH = OFF_BIH + 3 * kH, OFF_WO = OFF_BHH + 3 * kH,
              OFF_BO = OFF_WO + kH, NGRAD = OFF_BO + 1;
static_assert(NGRAD == 12929, "w_ih + w_hh + b_ih + b_hh + w_o + b_o of GRU(1, 64) + Linear(64, 1)");

// (a) Forward with saved activations: gru_lat_kernel<true> (gru_lat.hip) built from the same pieces of gru_lat_step.h -- the
// lane constants, the gate evaluation, the head on a fifth wave, the parity unroller, the epilogue -- so y and the final h
// are bit-identical to kernel_variant "lat" for every B because they are computed by the same code (the head's arithmetic
// does not depend on which wave evaluates it).  In addition lane kq of each quad writes one of the saved values of
// its unit per step (kq = 0 also gh_n) to an LDS stage of SC steps, which the whole workgroup flushes to the workspace with
// coalesced 16-byte stores after every SC steps.  (Stored straight from the step, each global store made the compiler wait
// for its completion before the step's registers were reused: a store round trip inside the recurrence, every step.  The
// flush's stores are waited for the same way, in the first step after the flush: one round trip per SC steps.)
constexpr int SC = 32;                   // steps per LDS stage of the saves (divides the tile, 40 KB)
//
// REP (the replica entry points): the streams are stacked replica-major, stream s belongs to replica s / bper, and the six
// parameter pointers are the [R, ...] stacks -- the workgroup moves them to its replica's slice before the weight load (a scalar
// division and six scalar adds, once); everything behind that is the same code.  REP = false reads no bper.
template <bool REP>
__global__ __launch_bounds__(320) void gru_train_fwd_kernel(GruArgs a, float *__restrict__ ws, const unsigned bper)
{
#pragma clang fp contract(off)
    if constexpr (REP) {
        const size_t rep = blockIdx.x / bper;
        a.w_ih += rep * (3 * kH); a.w_hh += rep * (3 * kH * kH); a.b_ih += rep * (3 * kH); a.b_hh += rep * (3 * kH);
        a.w_o += rep * kH;
        if (a.b_o) a.b_o += rep;
    }
    __shared__ __attribute__((aligned(16))) float stg[SC * NSAVE * kH];   // saves of steps c0 .. c0 + SC - 1: [step][j][u]
    __shared__ __attribute__((aligned(16))) float hb[2][kH];
    __shared__ float xt[2][LT];
    __shared__ float yt[2][LT];

    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ul = l >> 2, kq = l & 3;
    const bool head_wave = w == 4;
    const int u = 16 * (w & 3) + ul;
    const int64_t s = blockIdx.x;
    const int64_t T = a.T;
    const float *xs = a.x + s * a.xs;
    float *ys = a.y + s * a.ys;
    float *const stg_l = stg + kq * kH + u;                              // this lane's save slot in the stage's step 0

    constexpr float INV_SN = 1.0f / SN;
    Lane c;
    c.load(a, u, kq);
    Head hd;
    hd.load(a, l);
    float hold = a.h_state ? a.h_state[s * kH + u] : 0.0f;

    if (kq == 0 && !head_wave) hb[0][u] = hold;
    if (tid < LT && tid < T) xt[0][tid] = xs[tid];
    __syncthreads();

    const float *const hq_rd = &hb[0][16 * kq];
    float *const hu_wr = &hb[0][u];
    auto step = [&](const int ph, auto par_c, const int tb) {
        constexpr int par = decltype(par_c)::value;
        if (head_wave) {
            hd.sample_before(hb[par], l, yt, tb, ph);
            lds_barrier();
            return;
        }
        const f32x4 h0 = *(const f32x4 *)(hq_rd + par * kH + 0), h1 = *(const f32x4 *)(hq_rd + par * kH + 4);
        const f32x4 h2 = *(const f32x4 *)(hq_rd + par * kH + 8), h3 = *(const f32x4 *)(hq_rd + par * kH + 12);
        const float x = xt[tb][ph];
        float r, z, n, gh;
        gates(c, h0, h1, h2, h3, x, r, z, n, gh);
        // saves of the step (SC divides the tile): lane kq writes row kq (h_{t-1}, r, z, n), lane 0 of the quad also row 4 (gh_n, unscaled)
        float *wt = stg_l + (ph & (SC - 1)) * (NSAVE * kH);
        wt[0] = kq == 0 ? hold : kq == 1 ? r : kq == 2 ? z : n;
        if (kq == 0) wt[(NSAVE - 1) * kH] = gh * INV_SN;
        hold = __builtin_fmaf(z, hold - n, n);
        hu_wr[(par ^ 1) * kH] = hold;
        lds_barrier();
    };

    for (int64_t tile0 = 0; tile0 < T; tile0 += LT) {
        const int ns = (int)((T - tile0) < LT ? (T - tile0) : LT);
        const int tb = (int)((tile0 >> 8) & 1);
        for (int c0 = 0; c0 < ns; c0 += SC) {
            const int c1 = ns < c0 + SC ? ns : c0 + SC;
            if (c0 == 0) {
                run(0, c1 < 3 ? c1 : 3, step, tb);
                if (ns > 2 && tile0 >= LT && tid < LT) ys[tile0 - LT + tid] = yt[tb ^ 1][tid];      // previous y tile is complete
                run(c1 < 3 ? c1 : 3, c1, step, tb);
            } else {
                // the next x tile into its buffer (read from step 0 of the next tile on), loaded and written here: a load kept in
                // flight in a register across the steps (as gru_lat.hip does) made the compiler wait for it at every copy of that
                // register inside the step loop, i.e. in every step of the tile's second half
                if (c0 == 128 && tid < LT) {
                    const int64_t nx = tile0 + LT + tid;
                    xt[tb ^ 1][tid] = nx < T ? xs[nx] : 0.0f;
                }
                run(c0, c1, step, tb);
            }
            // flush the stage: steps [c0, c1) are one contiguous run of the stream's workspace (the last step's barrier has
            // ordered every write to it); the barrier behind orders these reads before the next stage's writes
            const int nf = (c1 - c0) * (NSAVE * kH);
            float *dst = ws + (s * T + tile0 + c0) * (NSAVE * kH);
            for (int i = 4 * tid; i < nf; i += 4 * 320) *(f32x4 *)(dst + i) = *(const f32x4 *)(stg + i);
            lds_barrier();
        }
    }
    finish(a, hd, hb, yt, head_wave);
    if (a.h_state && kq == 0 && !head_wave) a.h_state[s * kH + u] = hold;
}

// (b) Backward through time, one workgroup (4 waves) per stream, t = T-1 down to 0: the transpose of the forward's layout.
// Lane l = 4 kl + uq of wave w owns column k = 16 w + kl of W_hh and the output-unit quarter uq: it holds
// W_hh[g][16 uq + i][k] (g = r, z, n; i < 16: 48 registers) and accumulates the same 48 entries of dW_hh.  Per step:
//   * each quad evaluates the elementwise adjoints of unit k redundantly from the saved h_{t-1}, r, z, n, gh_n and
//     g = dh_t + w_o dy_t;  lane uq = 0 publishes a_r, a_z, a_nh of unit k to LDS (double-buffered by step parity);
//   * behind ONE barrier each lane reads the 48 adjoints of its quarter (12 broadcast ds_read_b128), does 48 FMAs for
//     W_hh^T a and 48 for dW_hh += a h_{t-1}[k], and a DPP quad sum gives dh_{t-1}[k] = g z + W_hr^T a_r + W_hz^T a_z + W_hn^T a_nh.
// The saved values of step t - PF are loaded while step t runs (a register ring, PF steps deep), so the global latency sits
// behind the recurrence; the barrier orders LDS only and does not drain them.
constexpr int PF = 4;
// REP: as in the forward -- w_hh and w_o are the [R, ...] stacks and the workgroup of stream s reads replica s / bper's.
template <bool REP>
__global__ __launch_bounds__(256) void gru_train_bwd_kernel(const float *__restrict__ w_hh, const float *__restrict__ w_o,
                                                             const float *__restrict__ x, int64_t xs, const float *__restrict__ ws,
                                                             const float *__restrict__ dy, int64_t dys,
                                                             const float *__restrict__ dh_T, int64_t T, float *__restrict__ dh0,
                                                             float *__restrict__ part, const unsigned bper)
{
#pragma clang fp contract(off)
    if constexpr (REP) {
        const size_t rep = blockIdx.x / bper;
        w_hh += rep * (3 * kH * kH);
        w_o += rep * kH;
    }
    __shared__ __attribute__((aligned(16))) float ab[2][3][kH];       // a_r, a_z, a_nh of the step, by step parity

    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kl = l >> 2, uq = l & 3;
    const int k = 16 * w + kl;
    const int64_t s = blockIdx.x;
    const float *xs_ = x + s * xs;
    const float *dys_ = dy ? dy + s * dys : nullptr;
    const float *wsk = ws + s * T * (NSAVE * kH) + k;

    float W[3][16], dW[3][16];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            W[g][i] = w_hh[(size_t)(g * kH + 16 * uq + i) * kH + k];
            dW[g][i] = 0.0f;
        }
    const float wo = w_o[k];
    float dh = dh_T ? dh_T[s * kH + k] : 0.0f;
    // the per-unit sums over time (one of each per quad) in fp64: b_o's gradient alone is the sum of all T values of dy
    double dwir = 0.0, dwiz = 0.0, dwin = 0.0, dbr = 0.0, dbz = 0.0, dbin = 0.0, dbhn = 0.0, dwo = 0.0, dbo = 0.0;

    // the ring: slot j holds step values of t = (T - 1 - j) mod PF positions; indices below 0 are clamped (never consumed)
    float rh[PF], rr[PF], rz[PF], rn[PF], rg[PF], rx[PF], rd[PF];
    auto fetch = [&](const int j, int64_t t) {
        t = t < 0 ? 0 : t;
        const float *p = wsk + t * (NSAVE * kH);
        rh[j] = p[0 * kH]; rr[j] = p[1 * kH]; rz[j] = p[2 * kH]; rn[j] = p[3 * kH]; rg[j] = p[4 * kH];
        rx[j] = xs_[t];
        rd[j] = dys_ ? dys_[t] : 0.0f;
    };
    if (T > 0) {
#pragma unroll
        for (int j = 0; j < PF; ++j) fetch(j, T - 1 - j);
    }

    const float *const aq = &ab[0][0][16 * uq];
    auto step = [&](const int j, const int64_t t, auto par_c) {
        constexpr int par = decltype(par_c)::value;
        const float hp = rh[j], r = rr[j], z = rz[j], n = rn[j], ghn = rg[j], xv = rx[j], dyv = rd[j];
        fetch(j, t - PF);
        const float g = __builtin_fmaf(wo, dyv, dh);
        const float dn = g * (1.0f - z), dz = g * (hp - n);
        const float an = dn * (1.0f - n * n);
        const float az = dz * (z * (1.0f - z));
        const float ar = (an * ghn) * (r * (1.0f - r));
        const float anh = an * r;
        const float ht = __builtin_fmaf(z, hp - n, n);                  // h_t exactly as the forward formed it
        dwir += (double)ar * xv; dwiz += (double)az * xv; dwin += (double)an * xv;
        dbr += ar; dbz += az; dbin += an; dbhn += anh;
        dwo += (double)dyv * ht; dbo += dyv;
        if (uq == 0) { ab[par][0][k] = ar; ab[par][1][k] = az; ab[par][2][k] = anh; }
        lds_barrier();
        float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
        for (int gg = 0; gg < 3; ++gg)
#pragma unroll
            for (int i = 0; i < 16; i += 4) {
                const f32x4 av = *(const f32x4 *)(aq + par * 3 * kH + gg * kH + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e & 1) p1 = __builtin_fmaf(W[gg][i + e], av[e], p1);
                    else p0 = __builtin_fmaf(W[gg][i + e], av[e], p0);
                    dW[gg][i + e] = __builtin_fmaf(av[e], hp, dW[gg][i + e]);
                }
            }
        const float q = quad_add<0x4E>(quad_add<0xB1>(p0 + p1));
        dh = __builtin_fmaf(g, z, q);
    };
    // steps in groups of PF (the ring slot and the LDS parity known at compile time: PF is even)
    int64_t t = T - 1;
    for (; t - (PF - 1) >= 0; t -= PF) {
        step(0, t, P0{}); step(1, t - 1, P1{}); step(2, t - 2, P0{}); step(3, t - 3, P1{});
    }
    if (t >= 0) step(0, t, P0{});
    if (t >= 1) step(1, t - 1, P1{});
    if (t >= 2) step(2, t - 2, P0{});

    float *ps = part + s * NGRAD;
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int i = 0; i < 16; ++i) ps[OFF_WHH + (g * kH + 16 * uq + i) * kH + k] = dW[g][i];
    if (uq == 0) {
        ps[0 * kH + k] = (float)dwir; ps[1 * kH + k] = (float)dwiz; ps[2 * kH + k] = (float)dwin;
        ps[OFF_BIH + 0 * kH + k] = (float)dbr; ps[OFF_BIH + 1 * kH + k] = (float)dbz; ps[OFF_BIH + 2 * kH + k] = (float)dbin;
        ps[OFF_BHH + 0 * kH + k] = (float)dbr; ps[OFF_BHH + 1 * kH + k] = (float)dbz; ps[OFF_BHH + 2 * kH + k] = (float)dbhn;
        ps[OFF_WO + k] = (float)dwo;
        if (dh0) dh0[s * kH + k] = dh;
    }
    if (tid == 0) ps[OFF_BO] = (float)dbo;
}

// (c) The parameter gradients of R models of bper streams each (grid row = model; the single model is R = 1, bper = B): every
// entry adds its model's bper per-stream partials in stream order, in fp64 (no atomics).  bper = 0 writes zeros.
__global__ __launch_bounds__(256) void gru_train_reduce_replicas_kernel(const float *__restrict__ part, int64_t bper,
                                                                        float *__restrict__ grad)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NGRAD) return;
    const int64_t r = blockIdx.y;
    const float *p = part + r * bper * NGRAD;
    double acc = 0.0;
    for (int64_t b = 0; b < bper; ++b) acc += (double)p[b * NGRAD + e];
    grad[r * NGRAD + e] = (float)acc;
}

// (d) Loss adjoints, for R losses at once (the single loss is R = 1, bper = B).  ESR (code/train.py:176): L = (S_e / n) /
// (S_t / n + eps) with whole-batch sums S (sums2 = [S_e, S_t], fp64, from ntm_esr_sums) -> dL/dy = 2 (y - t) / (n (S_t / n + eps)),
// times the upstream gradient.  Grid row = replica r: its N = bper * T elements with ITS sums2[r], gout[r] and n.
__global__ __launch_bounds__(256) void esr_grad_replicas_kernel(const float *__restrict__ y, const float *__restrict__ t, int64_t N,
                                                                const double *__restrict__ sums2, const float *__restrict__ gout,
                                                                double eps, float *__restrict__ dy)
{
    const int64_t r = blockIdx.y;
    const double n = (double)N;
    const double c = (double)gout[r] * 2.0 / (n * (sums2[2 * r + 1] / n + eps));
    const float *yr = y + r * N, *tr = t + r * N;
    float *dr = dy + r * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
        dr[i] = (float)(c * ((double)yr[i] - (double)tr[i]));
}

// DCPreESR (code/train.py:174): the same on the DC-blocked signals, f = (1 - z^-1)/(1 - R z^-1), R = pole, from zero state.  With
// e_f = f(y - t) and v = 2 e_f / (n (S_tf / n + eps)), dL/dy = f^T v: the anti-causal one-pole q[t] = v[t] + R q[t+1] followed
// by the adjoint first difference dy[t] = q[t] - q[t+1].  One thread per stream, fp64 recursions; e_f is parked in dy between
// the causal and the anti-causal pass.  The B streams are replicas of bper each: stream b takes sums2 [.,2], gout [.] and
// n = bper * T of replica b / bper (the single loss: bper = B, replica 0).
__global__ __launch_bounds__(64) void esr_dcpre_grad_kernel(const float *__restrict__ y, const float *__restrict__ t, int64_t B,
                                                            int64_t T, float pole, const double *__restrict__ sums2,
                                                            const float *__restrict__ gout, double eps, float *__restrict__ dy,
                                                            const int64_t bper)
{
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int64_t rep = b / bper;
    sums2 += 2 * rep;
    gout += rep;
    const float *yb = y + b * T, *tb = t + b * T;
    float *db = dy + b * T;
    const double Rd = (double)pole;
    double prev = 0.0, ef = 0.0;
#pragma unroll 8
    for (int64_t i = 0; i < T; ++i) {
        const double wv = (double)yb[i] - (double)tb[i];
        ef = (wv - prev) + Rd * ef;
        prev = wv;
        db[i] = (float)ef;
    }
    const double n = (double)(bper * T);
    const double c = (double)gout[0] * 2.0 / (n * (sums2[1] / n + eps));
    double q1 = 0.0;                               // q[t + 1]
#pragma unroll 8
    for (int64_t i = T - 1; i >= 0; --i) {
        const double q = c * (double)db[i] + Rd * q1;
        db[i] = (float)(q - q1);
        q1 = q;
    }
}

// (d') The whole-batch sums of R losses from the per-stream rows of esr_sums_kernel / esr_dcpre_kernel: rows [R][bper][splits][2]
// fp64 -> out [R][2].  The single-model losses add these rows with torch's sum() (model.py: the `splits` partial rows of a
// stream, then the streams), and a loss of this path must have THEIR bits, so this kernel adds in the order torch's reduction
// takes for a column of n < 256 values -- four accumulators, value i into accumulator i mod 4, then ((a0 + a1) + a2) + a3 (for
// n <= 4 that is index order) -- and for n >= 256: thread y of 256 that way over values y, y + 256, ..., then the LDS tree
// 128, 64, .., 1.  Fixed, free of atomics; tests/test_gpu_train_replicas.py holds it to the single-model losses bit for bit.
__device__ __forceinline__ double sum4_strided(const double *p, const int64_t n, const int64_t stride)
{
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t i = 0;
    for (; i + 3 < n; i += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += p[(i + k) * stride];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (i + k < n) a[k] += p[(i + k) * stride];
    return ((a[0] + a[1]) + a[2]) + a[3];
}

constexpr int LS_T = 256;

__global__ __launch_bounds__(LS_T) void loss_sums_replicas_kernel(const double *__restrict__ rows, int64_t bper, int splits,
                                                                  double *__restrict__ out)
{
    __shared__ double red[2][LS_T];
    const int y = threadIdx.x;
    const double *rr = rows + (int64_t)blockIdx.x * bper * splits * 2;
    // the sum of stream b's partial rows, column c
    auto stream = [&](const int64_t b, const int c) { return splits == 1 ? rr[2 * b + c] : sum4_strided(rr + b * splits * 2 + c, splits, 2); };
    const int bh = bper < LS_T ? 1 : LS_T;
    double v[2] = {0.0, 0.0};
    if (y < bh) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            double a[4] = {0.0, 0.0, 0.0, 0.0};
            int64_t i = y;
            for (; i + 3 * bh < bper; i += 4 * bh) {
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] += stream(i + (int64_t)k * bh, c);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (i + (int64_t)k * bh < bper) a[k] += stream(i + (int64_t)k * bh, c);
            v[c] = ((a[0] + a[1]) + a[2]) + a[3];
        }
    }
    if (bh == 1) {
        if (y == 0) { out[2 * blockIdx.x] = v[0]; out[2 * blockIdx.x + 1] = v[1]; }
        return;
    }
    red[0][y] = v[0]; red[1][y] = v[1];
    __syncthreads();
    for (int off = LS_T / 2; off > 0; off >>= 1) {
        if (y < off) { red[0][y] += red[0][y + off]; red[1][y] += red[1][y + off]; }
        __syncthreads();
    }
    if (y == 0) { out[2 * blockIdx.x] = red[0][0]; out[2 * blockIdx.x + 1] = red[1][0]; }
}

// (e) Adjoint of the time-varying fractional delay line (TimeVaryingDelayLine.forward, code/model.py:269-320) over one call.
// With z = [buffer (D), pre (L)] the forward is y[n] = sum over the taps m in {k+1, k} that delay_sample() counts of
// w_m(n) z[D + n - m], and the new buffer is z[L : L + D].  So
//     gz[i] = g_newbuf[i - L] (i >= L) + sum over ascending n of w_m(n) gy[n] where D + n - m = i,
// gbuf = gz[:D], gpre = gz[D:].  Warm-up: y = pre, gz[D + n] adds gy[n].  No gradient flows to d (the trajectory is data).
// One workgroup per stream.  Target i belongs to thread i % DB_T in every phase (its initial value, then one read-modify-write
// per tile of samples), and it adds its terms in ascending n: no atomics on floats, the bits do not depend on scheduling.
// Per tile of DB_NT samples the taps are staged in LDS: the target of tap a (m = k) D + q with q = n - k, of tap b (m = k + 1)
// D + q - 1, -1 where delay_sample() skips the tap, and the products w gy (rounded as the reference's autograd rounds them).
//   * gather: every d of the tile in [0, D] and q non-decreasing (a delay that never grows by 1 sample or more within one
//     sample, as every wow / flutter trajectory): the terms of target i are the run of n with q = i - D (tap a), followed by
//     the run with q = i - D + 1 (tap b).  A binary search over the tile's tap-a targets and a walk over those runs.
//   * scan (any other tile, or DB_SCAN): every owner looks at every sample of the tile in ascending n.
// Both add the same terms in the same order, so they give the same bits.
constexpr int DB_T = 256, DB_NT = 2048;

__global__ __launch_bounds__(DB_T) void delay_bwd_kernel(const float *__restrict__ gy, const float *__restrict__ d,
                                                         const float *__restrict__ gnb, float *__restrict__ gpre,
                                                         float *__restrict__ gbuf, int L, int D, int warmup, int force_scan)
{
#pragma clang fp contract(off)
    __shared__ int ta[DB_NT], tb[DB_NT];
    __shared__ float pa[DB_NT], pb[DB_NT];
    __shared__ int red[3];                  // lowest and highest target of the tile, scan needed

    const int t = threadIdx.x;
    const int64_t s = blockIdx.x;
    const float *gys = gy ? gy + s * L : nullptr;
    const float *ds = d ? d + s * L : nullptr;
    const float *gn = gnb ? gnb + s * D : nullptr;
    float *gp = gpre + s * L;
    float *gb = gbuf ? gbuf + s * D : nullptr;
    const int R = D + L;

    for (int i = t; i < R; i += DB_T) {     // the initial value of every target
        const float v = (gn && i >= L) ? gn[i - L] : 0.0f;
        if (i < D) {
            if (gb) gb[i] = v;
        } else {
            gp[i - D] = (warmup && gys) ? v + gys[i - D] : v;
        }
    }
    if (warmup || !gys) return;

    const float Dmax = (float)D;
    for (int n0 = 0; n0 < L; n0 += DB_NT) {
        const int nt = L - n0 < DB_NT ? L - n0 : DB_NT;
        if (t == 0) { red[0] = 0x7fffffff; red[1] = -1; red[2] = force_scan; }
        __syncthreads();
        int lo = 0x7fffffff, hi = -1, bad = 0;
        for (int j = t; j < nt; j += DB_T) {
            const int n = n0 + j;
            const float dn = ds[n], g = gys[n];
            const float kf = floorf(dn);
            int tg[2];
            float pr[2];
#pragma unroll
            for (int tap = 1; tap >= 0; --tap) {     // the tests of delay_sample()
                const float mf = kf + (float)tap;
                const float w = 1.0f - fabsf(mf - dn);
                const bool on = !(mf < 0.0f || mf > Dmax) && w > 0.0f;
                tg[tap] = on ? D + n - (int)mf : -1;
                pr[tap] = w * g;
            }
            tb[j] = tg[1]; pb[j] = pr[1];
            ta[j] = tg[0]; pa[j] = pr[0];
            bad |= !(dn >= 0.0f && dn <= Dmax);     // NaN too; in [0, D] tap a always counts
            if (tg[1] >= 0) { lo = min(lo, tg[1]); hi = max(hi, tg[1]); }
            if (tg[0] >= 0) { lo = min(lo, tg[0]); hi = max(hi, tg[0]); }
        }
        atomicMin(&red[0], lo);
        atomicMax(&red[1], hi);
        __syncthreads();
        for (int j = t; j + 1 < nt; j += DB_T) bad |= ta[j] > ta[j + 1];
        if (bad) red[2] = 1;
        __syncthreads();
        const int tlo = red[0], thi = red[1];
        const bool scan = red[2] != 0;
        for (int i = (tlo & ~(DB_T - 1)) + t; i <= thi; i += DB_T) {       // empty when no tap of the tile counts
            if (i < tlo || (i < D && !gb)) continue;
            float acc = i < D ? gb[i] : gp[i - D];
            if (scan) {
                for (int j = 0; j < nt; ++j) {
                    if (tb[j] == i) acc = acc + pb[j];
                    if (ta[j] == i) acc = acc + pa[j];
                }
            } else {
                int a = 0, b = nt;                  // first j with ta[j] >= i
                while (a < b) {
                    const int m = (a + b) >> 1;
                    if (ta[m] < i) a = m + 1; else b = m;
                }
                for (int j = a; j < nt && ta[j] <= i + 1; ++j) {
                    if (ta[j] == i) acc = acc + pa[j];
                    else if (tb[j] == i) acc = acc + pb[j];
                }
            }
            if (i < D) gb[i] = acc; else gp[i - D] = acc;
        }
        __syncthreads();                        // the stage and red[] are rewritten by the next tile
    }
}

}   // namespace

int64_t train_grad_floats() { return NGRAD; }

hipError_t launch_delay_bwd(const float *gy, const float *d, const float *g_newbuf, float *gpre, float *gbuf, int64_t B, int64_t L,
                            int D, int warmup, int force_scan, hipStream_t stream)
{
    if (B == 0 || L + D == 0) return hipSuccess;
    hipLaunchKernelGGL(delay_bwd_kernel, dim3((unsigned)B), dim3(DB_T), 0, stream, gy, d, g_newbuf, gpre, gbuf, (int)L, D, warmup,
                       force_scan);
    return hipGetLastError();
}

// bper = 0: one model (a's parameters as they are); else a.B = R * bper streams of R stacked replicas
hipError_t launch_gru_train_fwd(const GruArgs &a, float *ws, int64_t bper, hipStream_t stream)
{
    if (a.B == 0) return hipSuccess;
    if (bper == 0) hipLaunchKernelGGL(gru_train_fwd_kernel<false>, dim3((unsigned)a.B), dim3(320), 0, stream, a, ws, 0u);
    else hipLaunchKernelGGL(gru_train_fwd_kernel<true>, dim3((unsigned)a.B), dim3(320), 0, stream, a, ws, (unsigned)bper);
    return hipGetLastError();
}

hipError_t launch_gru_train_bwd(const float *w_hh, const float *w_o, const float *x, int64_t xs, const float *ws, const float *dy,
                                int64_t dys, const float *dh_T, int64_t B, int64_t T, float *dh0, float *part, int64_t bper,
                                hipStream_t stream)
{
    if (B == 0) return hipSuccess;
    if (bper == 0)
        hipLaunchKernelGGL(gru_train_bwd_kernel<false>, dim3((unsigned)B), dim3(256), 0, stream, w_hh, w_o, x, xs, ws, dy, dys, dh_T, T,
                           dh0, part, 0u);
    else
        hipLaunchKernelGGL(gru_train_bwd_kernel<true>, dim3((unsigned)B), dim3(256), 0, stream, w_hh, w_o, x, xs, ws, dy, dys, dh_T, T,
                           dh0, part, (unsigned)bper);
    return hipGetLastError();
}

// the launchers of (c) and (d): R models / losses of bper streams each; the single-model entry points pass R = 1, bper = B
hipError_t launch_gru_train_reduce_replicas(const float *part, int64_t R, int64_t bper, float *grad, hipStream_t stream)
{
    if (R == 0) return hipSuccess;      // bper = 0 is launched: grad <- 0
    hipLaunchKernelGGL(gru_train_reduce_replicas_kernel, dim3((NGRAD + 255) / 256, (unsigned)R), dim3(256), 0, stream, part, bper, grad);
    return hipGetLastError();
}

// N = bper * T elements per replica
hipError_t launch_esr_grad_replicas(const float *y, const float *t, int64_t R, int64_t N, const double *sums2, const float *gout,
                                    double eps, float *dy, hipStream_t stream)
{
    if (R == 0 || N == 0) return hipSuccess;
    const int64_t want = (N + 255) / 256, cap = (4096 + R - 1) / R;
    hipLaunchKernelGGL(esr_grad_replicas_kernel, dim3((unsigned)(want < cap ? want : cap), (unsigned)R), dim3(256), 0, stream, y, t, N,
                       sums2, gout, eps, dy);
    return hipGetLastError();
}

hipError_t launch_esr_dcpre_grad_replicas(const float *y, const float *t, int64_t R, int64_t bper, int64_t T, float pole,
                                          const double *sums2, const float *gout, double eps, float *dy, hipStream_t stream)
{
    const int64_t B = R * bper;
    if (B == 0 || T == 0) return hipSuccess;
    hipLaunchKernelGGL(esr_dcpre_grad_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, y, t, B, T, pole, sums2, gout, eps,
                       dy, bper);
    return hipGetLastError();
}

hipError_t launch_loss_sums_replicas(const double *rows, int64_t R, int64_t bper, int splits, double *out, hipStream_t stream)
{
    if (R == 0) return hipSuccess;
    hipLaunchKernelGGL(loss_sums_replicas_kernel, dim3((unsigned)R), dim3(LS_T), 0, stream, rows, bper, splits, out);
    return hipGetLastError();
}

}   // namespace ntm
