// N4 ("next" row): Jiles-Atherton magnetisation stage of the reference's white-box tape simulator,
// code/tape.py:516-551 (Tape.H_mag) + :587-635 (Tape._f): per stream a strictly sequential fp64 recurrence
// (trapezoidal dH/dt, 4th-order Runge-Kutta of the hysteresis ODE, clamp to +-Ms), the same archetype as the
// GRU path: streams are the only parallel axis.  One lane per stream; H and M tiles of 64 streams x 64
// samples go through LDS so that global accesses are 512-B row segments.
#include "ntm_common.h"
#include "tape_math.h"   // JaParams, rcp_nr, expm1_neg, coth_gt, langevin_prime_lt1, ja_f

namespace ntm {

constexpr int JT = 64;   // tile: 64 streams x 64 samples

__global__ __launch_bounds__(64) void tape_hmag_kernel(const double *H, double *M, int64_t B, int64_t N, double *state,
                                                       double Ts, JaParams p)
{
#pragma clang fp contract(off)   // only the explicit fma() calls of the helpers fuse
    __shared__ double tile[JT][JT + 1];
    const int l = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * JT;
    const int64_t b = s0 + l;
    const bool valid = b < B;
    double Mp = valid ? state[3 * b] : 0.0, Hpv = valid ? state[3 * b + 1] : 0.0, Hpp = valid ? state[3 * b + 2] : 0.0;
    for (int64_t n0 = 0; n0 < N; n0 += JT) {
        const int nt = (int)((N - n0) < JT ? (N - n0) : JT);
        for (int r = 0; r < JT; ++r)
            tile[r][l] = (s0 + r < B && l < nt) ? H[(s0 + r) * N + n0 + l] : 0.0;
        __syncthreads();
        for (int n = 0; n < nt; ++n) {
            const double Hn = tile[l][n];
            const double Hprime = 2.0 * (Hn - Hpv) / Ts - Hpp;
            const double k1 = Ts * ja_f(Mp, Hpv, Hpp, p);
            const double k2 = Ts * ja_f(Mp + k1 / 2.0, (Hn + Hpv) / 2.0, (Hprime + Hpp) / 2.0, p);
            const double k3 = Ts * ja_f(Mp + k2 / 2.0, (Hn + Hpv) / 2.0, (Hprime + Hpp) / 2.0, p);
            const double k4 = Ts * ja_f(Mp + k3, Hn, Hprime, p);
            double m = Mp + k1 * (1.0 / 6.0) + k2 * (1.0 / 3.0) + k3 * (1.0 / 3.0) + k4 * (1.0 / 6.0);
            m = m < -p.Ms ? -p.Ms : (m > p.Ms ? p.Ms : m);
            tile[l][n] = m;
            Hpv = Hn; Hpp = Hprime; Mp = m;
        }
        __syncthreads();
        for (int r = 0; r < JT; ++r)
            if (s0 + r < B && l < nt) M[(s0 + r) * N + n0 + l] = tile[r][l];
        __syncthreads();
    }
    if (valid) { state[3 * b] = Mp; state[3 * b + 1] = Hpv; state[3 * b + 2] = Hpp; }
}

// Record-head field of the reference's chain: I_rec = I_in + bias (code/tape.py:476-510), H = (N E I_rec) / G (:512-514),
// one fp64 pass, same operation order (bit-identical to the reference's torch ops).  bias [N] is shared by the streams.
__global__ __launch_bounds__(256) void tape_record_field_kernel(const double *I, const double *bias, double *H, int64_t B,
                                                                int64_t N, double gain, double gap)
{
#pragma clang fp contract(off)
    const int64_t total = B * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const double irec = bias ? I[i] + bias[i % N] : I[i];
        H[i] = (gain * irec) / gap;
    }
}

hipError_t launch_tape_record_field(const double *I, const double *bias, double *H, int64_t B, int64_t N, double gain,
                                    double gap, hipStream_t stream)
{
    if (B == 0 || N == 0) return hipSuccess;
    const int64_t total = B * N;
    const unsigned grid = (unsigned)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
    hipLaunchKernelGGL(tape_record_field_kernel, dim3(grid), dim3(256), 0, stream, I, bias, H, B, N, gain, gap);
    return hipGetLastError();
}

// The two resamplers of Tape.__call__ (code/tape.py:330-332, 471-474, 553-558: torchaudio.transforms.Resample, sinc
// interpolation with a Hann window -- the polyphase kernel table is built on the host, tape.py of this package): one thread
// per output sample,
//   y[i * up + p] = sum_k ker[p][k] * xpad[i * down + k],   xpad[j] = x[j - width]  (zero outside [0, N))
// fp64, taps = 2 width + down (15 when oversampling by 16, 210 when coming back).  HBM / L2 bound streaming.
__global__ __launch_bounds__(256) void resample_fir_kernel(const double *x, double *y, int64_t N, int64_t M, int up, int down,
                                                           int width, const double *ker)
{
    const int64_t b = blockIdx.y;
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= M) return;
    const int64_t i = o / up;
    const int p = (int)(o - i * up);
    const int taps = 2 * width + down;
    const double *xb = x + b * N;
    const double *kp = ker + (size_t)p * taps;
    const int64_t j0 = i * down - width;
    double acc = 0.0;
    for (int k = 0; k < taps; ++k) {
        const int64_t j = j0 + k;
        if (j >= 0 && j < N) acc = __builtin_fma(kp[k], xb[j], acc);
    }
    y[b * M + o] = acc;
}

hipError_t launch_resample_fir(const double *x, double *y, int64_t B, int64_t N, int64_t M, int up, int down, int width,
                               const double *ker, hipStream_t stream)
{
    if (B == 0 || M == 0) return hipSuccess;
    hipLaunchKernelGGL(resample_fir_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)B), dim3(256), 0, stream, x, y, N, M, up,
                       down, width, ker);
    return hipGetLastError();
}

// The playback-loss filter of Tape.H_play (code/tape.py:565-574: torchaudio.functional.lfilter with a = [1, 0, ...],
// i.e. a FIR, output clamped to [-1, 1] like lfilter's default clamp=True; no state carried, as in the reference):
//   y[n] = sum_{k < taps} h[k] x[n - k]
__global__ __launch_bounds__(256) void fir_f64_kernel(const double *x, double *y, int64_t N, const double *h, int taps, int clamp)
{
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const double *xb = x + b * N;
    double acc = 0.0;
    for (int k = 0; k < taps && k <= n; ++k) acc = __builtin_fma(h[k], xb[n - k], acc);
    if (clamp) acc = acc < -1.0 ? -1.0 : (acc > 1.0 ? 1.0 : acc);
    y[b * N + n] = acc;
}

hipError_t launch_fir_f64(const double *x, double *y, int64_t B, int64_t N, const double *h, int taps, int clamp, hipStream_t stream)
{
    if (B == 0 || N == 0) return hipSuccess;
    hipLaunchKernelGGL(fir_f64_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, stream, x, y, N, h, taps, clamp);
    return hipGetLastError();
}

hipError_t launch_tape_hmag(const double *H, double *M, int64_t B, int64_t N, double *state, double Ts, const double *par,
                            hipStream_t stream)
{
    if (B == 0 || N == 0) return hipSuccess;
    const JaParams p{par[0], par[1], par[2], par[3], par[4], 1.0 / par[1]};
    hipLaunchKernelGGL(tape_hmag_kernel, dim3((unsigned)((B + JT - 1) / JT)), dim3(64), 0, stream, H, M, B, N, state, Ts, p);
    return hipGetLastError();
}

}  // namespace ntm
