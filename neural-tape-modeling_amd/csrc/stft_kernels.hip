// "Next" row N1: the spectral part of the evaluation metrics that follow the path in
// code/test-model.py:250-254,386-388 -- `MultiResolutionSTFTLoss()` of the un-vendored auraloss submodule
// (code/test-model.py:25).  One kernel per resolution produces, per stream, the sums the loss is made of;
// the host (model.py MRSTFTLoss) divides and averages.
//
// Arithmetic (auraloss.freq.STFTLoss at its defaults): X = torch.stft(x, n_fft, hop, win_length,
// hann_window(win_length)) -- centred frames, reflect padding of n_fft/2, window zero-padded to n_fft on both
// sides -- and mag = sqrt(clamp(re^2 + im^2, min = eps)).
//
// Mapping: one 64-lane wave transforms one frame PAIR: z = w*(y + i t) goes through ONE complex n_fft-point
// FFT, and the two real spectra are separated afterwards (Y[k] = (Z[k] + conj Z[N-k])/2,
// T[k] = (Z[k] - conj Z[N-k])/(2i)).  The FFT is a Stockham autosort FFT in three passes of radix 16/8/4
// (256 = 4.4.4.4, 512 = 8.8.8, 1024 = 16.4.16, 2048 = 16.8.16): each lane holds n_fft/64 points in registers
// and runs whole radix-R butterflies on them; passes exchange through the wave's own padded
// LDS buffer, so no workgroup barrier is needed inside the frame loop (LDS operations of one wave are
// processed in issue order).  Window values and pass twiddles are per-lane, frame-invariant constants kept
// in registers (computed once with sincospi).  A workgroup = 4 waves works on one (stream, frame chunk);
// sums are accumulated in fp64 per lane and written per (stream, chunk, wave) -- the host adds them in a
// fixed order (deterministic, no atomics).
//
// Bound: VALU (about 5 n log2 n flop per frame pair); the signals are read once from HBM per resolution
// (frames overlap 5x in L1/L2), 8 B/sample algorithmic.
#include "ntm_common.h"

namespace ntm {

struct StftArgs {
    const float *y, *t;
    int64_t B, T, skip;
    int hop, win, chunks, frames_per_chunk, n_frames, mode;
    float eps;
    double *out;
    // mode 2 (mel): row-compressed mel filter bank (device): filter m = mel_w[mel_start[m] .. mel_start[m+1]) on the
    // bins mel_first[m] ...
    const int *mel_first, *mel_start;
    const float *mel_w;
    int n_mels;
};

typedef float f2 __attribute__((ext_vector_type(2)));

// Complex arithmetic on packed fp32 pairs with the operand-select / negate modifiers of the VOP3P encoding written out:
// hipcc builds a complex product from v_pk_mul + TWO v_pk_fma (one per sign pattern) + a v_mov that splices their halves,
// and a multiplication by -i from v_xor + v_mov -- 90 of the ~660 vector instructions of a 1024-point frame pair, in a
// kernel that is bound by vector issue.
__device__ __forceinline__ f2 cmul(f2 a, f2 b)
{
    f2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));                     // (ax bx, ax by)
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"             // (- ay by, + ay bx)
        : "+v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ f2 mul_mi(f2 a) { return (f2){a.y, -a.x}; }             // a * (-i)
// The two real spectra inside Z = FFT(y + i t), UNSCALED:  2 Y[k] = Z[k] + conj Z[N-k],  2 T[k] = (Z[k] - conj Z[N-k]) / i,
// one packed add each.  (The factor 1/2 -- 1/4 on the powers -- is a power of two: it is applied once to the frame
// sums, with the clamp floor scaled the other way; results are bit-identical to scaling every bin.)
__device__ __forceinline__ void split_spectra(f2 zk, f2 zn, f2 &Y2, f2 &T2)
{
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(Y2) : "v"(zk), "v"(zn));                                   // (zk.x + zn.x, zk.y - zn.y)
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,0] neg_hi:[1,0]" : "=v"(T2) : "v"(zk), "v"(zn));      // (zk.y + zn.y, zn.x - zk.x)
}
// a + (-i) d  and  a - (-i) d  in one packed add each (the half swap and the sign ride on the second operand)
__device__ __forceinline__ f2 add_mi(f2 a, f2 d)
{
    f2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(d));   // (a.x + d.y, a.y - d.x)
    return r;
}
__device__ __forceinline__ f2 sub_mi(f2 a, f2 d)
{
    f2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(d));   // (a.x - d.y, a.y + d.x)
    return r;
}

__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- in-register DFTs (forward, e^{-2 pi i nk/R}), natural order in and out -------------------------------
__device__ __forceinline__ void dft2(f2 &a, f2 &b) { const f2 t = a; a = t + b; b = t - b; }

__device__ __forceinline__ void dft4(f2 &x0, f2 &x1, f2 &x2, f2 &x3)
{
    const f2 s02 = x0 + x2, d02 = x0 - x2, s13 = x1 + x3, d13 = x1 - x3;
    x0 = s02 + s13; x1 = add_mi(d02, d13); x2 = s02 - s13; x3 = sub_mi(d02, d13);
}

// the same with x2 standing for (-i) x2 (the W16^4 twiddle of the radix-16 butterfly, folded into the first adds)
__device__ __forceinline__ void dft4_x2mi(f2 &x0, f2 &x1, f2 &x2, f2 &x3)
{
    const f2 s02 = add_mi(x0, x2), d02 = sub_mi(x0, x2), s13 = x1 + x3, d13 = x1 - x3;
    x0 = s02 + s13; x1 = add_mi(d02, d13); x2 = s02 - s13; x3 = sub_mi(d02, d13);
}

constexpr float C8 = 0.70710678118654752f;                       // cos(pi/4)
constexpr float C16 = 0.92387953251128674f, S16 = 0.38268343236508977f;   // cos, sin(pi/8)

template <int R> __device__ __forceinline__ void dft(f2 (&x)[R]);

template <> __device__ __forceinline__ void dft<2>(f2 (&x)[2]) { dft2(x[0], x[1]); }
template <> __device__ __forceinline__ void dft<4>(f2 (&x)[4]) { dft4(x[0], x[1], x[2], x[3]); }

// R = 8 = 4 x 2:  n = 2 n1 + n2,  k = k1 + 4 k2
template <> __device__ __forceinline__ void dft<8>(f2 (&x)[8])
{
    dft4(x[0], x[2], x[4], x[6]);                                 // n2 = 0: a[0][k1] in x[2 k1]
    dft4(x[1], x[3], x[5], x[7]);                                 // n2 = 1: a[1][k1] in x[2 k1 + 1]
    x[3] = add_mi(x[3], x[3]) * (f2){C8, C8};                     // * W8^1 = (c, -c):  c (x + y, y - x)
    // (x[5] * W8^2 = x[5] * (-i) is folded into the last stage below)
    x[7] = sub_mi(x[7], x[7]) * (f2){-C8, -C8};                   // * W8^3 = (-c, -c): -c (x - y, x + y)
    f2 y[8];
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {
        if (k1 == 2) { y[k1] = add_mi(x[4], x[5]); y[k1 + 4] = sub_mi(x[4], x[5]); }
        else { y[k1] = x[2 * k1] + x[2 * k1 + 1]; y[k1 + 4] = x[2 * k1] - x[2 * k1 + 1]; }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = y[i];
}

// R = 16 = 4 x 4:  n = 4 n1 + n2,  k = k1 + 4 k2
template <> __device__ __forceinline__ void dft<16>(f2 (&x)[16])
{
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) dft4(x[n2], x[4 + n2], x[8 + n2], x[12 + n2]);    // a[n2][k1] in x[4 k1 + n2]
    // twiddles W16^(n2 k1)
    const f2 w1 = {C16, -S16}, w2 = {C8, -C8}, w3 = {S16, -C16}, w6 = {-C8, -C8}, w9 = {-C16, S16};
    x[4 * 1 + 1] = cmul(x[4 * 1 + 1], w1); x[4 * 1 + 2] = cmul(x[4 * 1 + 2], w2); x[4 * 1 + 3] = cmul(x[4 * 1 + 3], w3);
    x[4 * 2 + 1] = cmul(x[4 * 2 + 1], w2); /* x[10] * (-i): inside dft4_x2mi below */ x[4 * 2 + 3] = cmul(x[4 * 2 + 3], w6);
    x[4 * 3 + 1] = cmul(x[4 * 3 + 1], w3); x[4 * 3 + 2] = cmul(x[4 * 3 + 2], w6); x[4 * 3 + 3] = cmul(x[4 * 3 + 3], w9);
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {                                                              // X[k1 + 4 k2] in x[4 k1 + k2]
        if (k1 == 2) dft4_x2mi(x[8], x[9], x[10], x[11]);
        else dft4(x[4 * k1], x[4 * k1 + 1], x[4 * k1 + 2], x[4 * k1 + 3]);
    }
    f2 y[16];
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) y[k1 + 4 * k2] = x[4 * k1 + k2];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = y[i];
}

// exchange-buffer index: one float2 of padding per 16 takes the strided Stockham stores from 32-way to two-way
// bank conflicts (PMC: the conflicts that remain cost 6-7 % of the wave cycles)
__device__ __forceinline__ constexpr int padi(int i) { return i + (i >> 4); }

// Frames of n_fft >= 256 use all 64 lanes of a wave (n_fft/64 points per lane); smaller frames use SUB = n_fft/4
// lanes each (4 points per lane) and a wave transforms 64/SUB frames side by side.
template <int N> struct Geo {
    static constexpr int SUB = N >= 256 ? 64 : N / 4;     // lanes per frame
    static constexpr int P = N / SUB;                     // points per lane
    static constexpr int FPW = 64 / SUB;                  // frames per wave and iteration
    static constexpr int NPAD = N + N / 16;               // padded exchange buffer of one frame (float2)
};

// Per-lane twiddles of one Stockham pass, radix R with sub-transform size Ns: butterfly b of this lane is
// j = sl + SUB b (sl = lane within the frame), k = j mod Ns, and input t is multiplied by
// exp(-2 pi i t k / (Ns R)).  Frame-invariant.
template <int N, int R, int Ns> struct PassTw {
    static constexpr int SUB = Geo<N>::SUB;
    static constexpr int NB = N / R / SUB;
    static constexpr int NBW = Ns <= SUB ? 1 : NB;     // Ns <= SUB: k = sl mod Ns is the same for every butterfly of the lane
    f2 w[Ns > 1 ? NBW * (R - 1) : 1];
    __device__ __forceinline__ void init(int sl)
    {
        if constexpr (Ns > 1) {
#pragma unroll
            for (int b = 0; b < NBW; ++b)
#pragma unroll
                for (int t = 1; t < R; ++t) {
                    const int k = (sl + SUB * b) & (Ns - 1);
                    float sn, cs;
                    sincospif(-2.0f * (float)(t * k) / (float)(Ns * R), &sn, &cs);
                    w[b * (R - 1) + t - 1] = (f2){cs, sn};
                }
        }
    }
    __device__ __forceinline__ f2 get(int b, int t) const { return w[(NBW == 1 ? 0 : b) * (R - 1) + t - 1]; }
};

// One Stockham pass over a frame's N points: v[q] holds point sl + SUB q; buf is the frame's exchange buffer.
template <int N, int R, int Ns, bool FIRST>
__device__ __forceinline__ void stockham_pass(f2 (&v)[Geo<N>::P], f2 *buf, const PassTw<N, R, Ns> &tw, int sl)
{
    constexpr int SUB = Geo<N>::SUB, P = Geo<N>::P, NB = N / R / SUB;
    static_assert(NB >= 1, "radix too large for the points a lane holds");
    if constexpr (!FIRST) {
        wave_lds_fence();
#pragma unroll
        for (int q = 0; q < P; ++q) v[q] = buf[padi(sl + SUB * q)];
        wave_lds_fence();
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = sl + SUB * b;
        const int k = j & (Ns - 1);
        f2 x[R];
#pragma unroll
        for (int t = 0; t < R; ++t) x[t] = v[b + t * NB];
        if constexpr (Ns > 1) {
#pragma unroll
            for (int t = 1; t < R; ++t) x[t] = cmul(x[t], tw.get(b, t));
        }
        dft<R>(x);
        const int o = (j - k) * R + k;
#pragma unroll
        for (int m = 0; m < R; ++m) buf[padi(o + m * Ns)] = x[m];
    }
}

// radix plans: 256 = 4.4.4.4, 512 = 8.8.8, 1024 = 16.4.16, 2048 = 16.8.16 (the small radix in the middle pass,
// where every butterfly of a lane shares its twiddles: fewer twiddle registers)
template <int LOG2N> struct Plan;
template <> struct Plan<6> { static constexpr int R0 = 4, R1 = 4, R2 = 4, R3 = 1; };      // 16 lanes per frame
template <> struct Plan<7> { static constexpr int R0 = 4, R1 = 4, R2 = 4, R3 = 2; };      // 32 lanes per frame
template <> struct Plan<8> { static constexpr int R0 = 4, R1 = 4, R2 = 4, R3 = 4; };
template <> struct Plan<9> { static constexpr int R0 = 8, R1 = 8, R2 = 8, R3 = 1; };
template <> struct Plan<10> { static constexpr int R0 = 16, R1 = 4, R2 = 16, R3 = 1; };
template <> struct Plan<11> { static constexpr int R0 = 16, R1 = 8, R2 = 16, R3 = 1; };

template <int LOG2N, int MODE>
__global__ __launch_bounds__(256, (LOG2N <= 10 ? 2 : 1)) void stft_sums_kernel(StftArgs a)
{
    constexpr int N = 1 << LOG2N;
    using G = Geo<N>;
    constexpr int SUB = G::SUB, P = G::P, FPW = G::FPW, NPAD = G::NPAD;
    using PL = Plan<LOG2N>;
    constexpr int R0 = PL::R0, R1 = PL::R1, R2 = PL::R2, R3 = PL::R3;
    static_assert(R0 * R1 * R2 * R3 == N, "radix plan");
    extern __shared__ f2 stft_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sl = lane & (SUB - 1), fs = lane / SUB;          // lane within the frame, frame slot within the wave
    f2 *buf = stft_smem + (wave * FPW + fs) * NPAD;            // this frame slot's exchange buffer

    PassTw<N, R1, R0> tw1;
    PassTw<N, R2, R0 * R1> tw2;
    PassTw<N, (R3 > 1 ? R3 : 2), R0 * R1 * R2 / (R3 > 1 ? 1 : 2)> tw3;      // (unused when R3 == 1)
    tw1.init(sl);
    tw2.init(sl);
    if constexpr (R3 > 1) tw3.init(sl);

    // window value of this lane's points n = sl + SUB q  (periodic Hann of `win` samples, centred in n_fft)
    const int left = (N - a.win) / 2;
    float wreg[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const int n = sl + SUB * q - left;
        wreg[q] = (n >= 0 && n < a.win) ? 0.5f - 0.5f * cospif(2.0f * (float)n / (float)a.win) : 0.0f;
    }

    const int64_t stream = blockIdx.x / a.chunks;
    const int chunk = blockIdx.x % a.chunks;
    const int L = (int)(a.T - a.skip);
    const float *ys = a.y + stream * a.T + a.skip;
    const float *ts = a.t + stream * a.T + a.skip;
    const int f_begin = chunk * a.frames_per_chunk;
    const int f_end = min(f_begin + a.frames_per_chunk, a.n_frames);
    constexpr int FSTEP = 4 * FPW;                             // frames per workgroup and iteration

    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const float eps4 = 4.0f * a.eps;                           // floor of the unscaled (4 x) powers, see split_spectra
    // raw samples of the frame pair, fetched one frame ahead: ry/rt[q] = (y, t)[f hop + sl + SUB q - N/2],
    // reflected at the ends (torch.stft center=True, pad_mode="reflect"); frame slots past the end read frame 0
    float ry[P], rt[P];
    auto fetch = [&](int f) {
        if (f >= f_end) f = f_begin;                        // idle slot of a multi-frame wave: harmless reload
        const int start = f * a.hop - N / 2;                // (T - skip < 2^31 - n_fft: checked by the API)
        if (FPW == 1 && start >= 0 && start + N <= L) {     // interior frame (wave-uniform): no index math per load
            const float *py = ys + start + sl, *pt = ts + start + sl;
#pragma unroll
            for (int q = 0; q < P; ++q) { ry[q] = py[SUB * q]; rt[q] = pt[SUB * q]; }
        } else {
#pragma unroll
            for (int q = 0; q < P; ++q) {
                int i = start + sl + SUB * q;
                i = i < 0 ? -i : i;
                i = i >= L ? 2 * (L - 1) - i : i;
                ry[q] = ys[i]; rt[q] = ts[i];
            }
        }
    };
    const int f_first = f_begin + wave * FPW;                  // this wave's first frame (slot 0)
    if (f_first < f_end) fetch(f_first + fs);
    for (int f0 = f_first; f0 < f_end; f0 += FSTEP) {
        const int f = f0 + fs;
        const bool live = f < f_end;                           // (only a multi-frame wave can have idle slots)
        f2 v[P];
#pragma unroll
        for (int q = 0; q < P; ++q) v[q] = (f2){wreg[q] * ry[q], wreg[q] * rt[q]};
        // ---- Stockham autosort FFT, the frame slot's own LDS buffer between passes ----
        {
            PassTw<N, R0, 1> tw0;
            stockham_pass<N, R0, 1, true>(v, buf, tw0, sl);
        }
        stockham_pass<N, R1, R0, false>(v, buf, tw1, sl);
        // the next frame's samples are fetched here, when the biggest butterflies are done and their registers are
        // free again (fetching at the top of the frame cost n_fft = 2048 spills and 0.7 ms)
        if (f0 + FSTEP < f_end) fetch(f + FSTEP);
        stockham_pass<N, R2, R0 * R1, false>(v, buf, tw2, sl);
        if constexpr (R3 > 1) stockham_pass<N, R3, R0 * R1 * R2, false>(v, buf, tw3, sl);
        wave_lds_fence();
        // ---- separate the two real spectra; distance terms for bins k = 0 .. N/2 ----
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        auto bin = [&](int k) {
            const f2 zk = buf[padi(k)], zn = buf[padi((N - k) & (N - 1))];
            f2 Y2, T2;
            split_spectra(zk, zn, Y2, T2);
            const f2 ysq = Y2 * Y2, tsq = T2 * T2;
            const float py0 = ysq.x + ysq.y, pt0 = tsq.x + tsq.y;                 // 4 x the powers
            const float py = fmaxf(py0, eps4), pt = fmaxf(pt0, eps4);
            if constexpr (MODE == 0) {
                // auraloss.freq.STFTLoss terms: magnitudes sqrt(clamp(power, eps))
                const float my = __builtin_amdgcn_sqrtf(py), mt = __builtin_amdgcn_sqrtf(pt);
                const float d = mt - my;
                s0 += d * d;
                s1 += pt;
                s2 += fabsf(__builtin_amdgcn_logf(py) - __builtin_amdgcn_logf(pt));   // log2 of the POWERS
                s3 += fabsf(d);
            } else {
                // power-spectrogram terms (torchaudio Spectrogram(power=2) as used by code/evaluation.py:75-84):
                // |P_y - P_t|, |log2 max(P_y, floor) - log2 max(P_t, floor)| (floor = eps), P_t, P_y
                s0 += fabsf(py0 - pt0);
                s1 += fabsf(__builtin_amdgcn_logf(py) - __builtin_amdgcn_logf(pt));
                s2 += pt0;
                s3 += py0;
            }
        };
        if constexpr (MODE != 2) {
            if (live) {
#pragma unroll
                for (int i = 0; i < P / 2; ++i) bin(sl + SUB * i);
                if (sl == 0) bin(N / 2);
            }
        } else {
            // mel entries of code/evaluation.py:86-92: mel = mel_basis @ power spectrogram (code/utilities/utilities.py:
            // 666), per frame.  The two power spectra (N/2 + 1 bins each) take the frame's exchange buffer over -- every
            // lane first reads its bins out of it -- and lane m then walks the bins of filters m, m + 64, ... (a triangle
            // spans 2 .. ~50 bins).  One frame per wave here (n_fft >= 256).
            static_assert(MODE != 2 || FPW == 1, "mel mode: one frame per wave");
            float py_[P / 2], pt_[P / 2], pyn = 0.0f, ptn = 0.0f;
            auto power = [&](int k, float &py0, float &pt0) {
                const f2 zk = buf[padi(k)], zn = buf[padi((N - k) & (N - 1))];
                f2 Y2, T2;
                split_spectra(zk, zn, Y2, T2);
                const f2 ysq = Y2 * Y2, tsq = T2 * T2;
                py0 = ysq.x + ysq.y;                                              // 4 x the powers
                pt0 = tsq.x + tsq.y;
            };
#pragma unroll
            for (int i = 0; i < P / 2; ++i) power(sl + SUB * i, py_[i], pt_[i]);
            if (sl == 0) power(N / 2, pyn, ptn);
            wave_lds_fence();                                   // every lane has read its bins: the buffer is free
            float *pw = reinterpret_cast<float *>(buf);         // [0 .. N/2] P_y, [N/2 + 1 .. N + 1] P_t
#pragma unroll
            for (int i = 0; i < P / 2; ++i) { pw[sl + SUB * i] = py_[i]; pw[N / 2 + 1 + sl + SUB * i] = pt_[i]; }
            if (sl == 0) { pw[N / 2] = pyn; pw[N + 1] = ptn; }
            wave_lds_fence();
            if (live) {
                for (int m = sl; m < a.n_mels; m += 64) {
                    const int b0 = a.mel_first[m], w0 = a.mel_start[m], nw = a.mel_start[m + 1] - w0;
                    float my = 0.0f, mt = 0.0f;
                    for (int q = 0; q < nw; ++q) {
                        const float wq = a.mel_w[w0 + q];
                        my = __builtin_fmaf(wq, pw[b0 + q], my);
                        mt = __builtin_fmaf(wq, pw[N / 2 + 1 + b0 + q], mt);
                    }
                    s0 += fabsf(my - mt);
                    s1 += fabsf(__builtin_amdgcn_logf(fmaxf(my, eps4)) - __builtin_amdgcn_logf(fmaxf(mt, eps4)));
                    s2 += mt;
                    s3 += my;
                }
            }
        }
        acc[0] += s0; acc[1] += s1; acc[2] += s2; acc[3] += s3;
        wave_lds_fence();
    }
    // mode 0: |ln mag_y - ln mag_t| = (ln 2 / 2) |log2 p_y - log2 p_t|;  mode 1: log10 = log10(2) log2
    // undo the factor 4 of the powers (2 of the magnitudes); the log differences do not carry it
    if constexpr (MODE == 0) { acc[0] *= 0.25; acc[1] *= 0.25; acc[3] *= 0.5; }
    else { acc[0] *= 0.25; acc[2] *= 0.25; acc[3] *= 0.25; }
    if constexpr (MODE == 0) acc[2] *= 0.34657359027997264;
    else acc[1] *= 0.30102999566398120;                       // modes 1 and 2: log10 = log10(2) log2
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double s = acc[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) a.out[(((size_t)stream * a.chunks + chunk) * 4 + wave) * 4 + c] = s;
    }
}

template <int LOG2N, int MODE>
static hipError_t launch_mode(const StftArgs &a, hipStream_t stream)
{
    constexpr int N = 1 << LOG2N;
    const size_t smem = (size_t)4 * Geo<N>::FPW * Geo<N>::NPAD * sizeof(f2);
    auto k = stft_sums_kernel<LOG2N, MODE>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)(a.B * a.chunks)), dim3(256), smem, stream, a);
    return hipGetLastError();
}

template <int LOG2N>
static hipError_t launch_one(const StftArgs &a, hipStream_t stream)
{
    if constexpr (LOG2N >= 10) {             // the mel projection is compiled for the frame sizes it is used with
        if (a.mode == 2) return launch_mode<LOG2N, 2>(a, stream);
    }
    if (a.mode == 2) return hipErrorInvalidValue;
    return a.mode == 0 ? launch_mode<LOG2N, 0>(a, stream) : launch_mode<LOG2N, 1>(a, stream);
}

hipError_t launch_stft_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop,
                            int win, float eps, int chunks, int mode, double *out, hipStream_t stream, int n_mels,
                            const int *mel_first, const int *mel_start, const float *mel_w)
{
    StftArgs a;
    a.mode = mode;
    a.n_mels = n_mels; a.mel_first = mel_first; a.mel_start = mel_start; a.mel_w = mel_w;
    a.y = y; a.t = t; a.B = B; a.T = T; a.skip = skip; a.hop = hop; a.win = win; a.chunks = chunks; a.eps = eps; a.out = out;
    a.n_frames = (int)(1 + (T - skip) / hop);
    a.frames_per_chunk = (a.n_frames + chunks - 1) / chunks;
    switch (n_fft) {
    case 64: return launch_one<6>(a, stream);
    case 128: return launch_one<7>(a, stream);
    case 256: return launch_one<8>(a, stream);
    case 512: return launch_one<9>(a, stream);
    case 1024: return launch_one<10>(a, stream);
    case 2048: return launch_one<11>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

// ---- adjoint of the mode 0 sums (ntm_stft_grad): d/dy of
//   sum_cells ( 1/2 c_sc (my - mt)^2 + c_log |ln my - ln mt| + c_lin |my - mt| ),   (c_sc, c_log, c_lin) = coef[stream],
// in two kernels.
//
// stft_grad_frames_kernel -- the mapping of stft_sums_kernel (a frame pair per wave, 64/SUB pairs for n_fft 64 / 128): the
// pair goes through the same transform; per bin k = 0 .. N/2
//   G = c_sc (my - mt) + sgn(my - mt) (c_log / my + c_lin)        (sgn(0) = 0: torch's abs backward; ln is monotonic)
//   c_k = G Y_k / my   where the unclamped power is above the floor, else 0 (the clamp has zero derivative),
// and the frame gradient g[n] = w[n] Re sum_{k=0}^{N/2} c_k e^{+2 pi i k n / N} = w[n] Re FFT(conj c)[n] -- every bin of
// 0 .. N/2 once, no 1/N, no doubling: the adjoint of the one-sided transform -- comes out of the SAME forward passes run
// on conj c (bins above N/2 zero).  A lane's bins k = sl + SUB i, i < P/2, are its points q < P/2 of that second
// transform, so c never touches memory.  The spectra in the exchange buffer are 2 Y and 2 T (split_spectra): with
// my2 = 2 my,  c_k = G Y2_k / my2,  G = c_sc/2 (my2 - mt2) + sgn (2 c_log / my2 + c_lin), floor 4 eps on the powers.
// The windowed frame gradients go to the workspace ws[stream][frame][n] (fp32); an idle frame slot of a multi-frame wave
// transforms a reloaded frame like the forward and stores nothing.
//
// stft_grad_gather_kernel -- the overlap-add back through the reflection as a gather, one thread per output sample, no
// atomics.  ORDER OF ADDITION for sample i of [0, L), L = T - skip, in fp32 from 0:
//   1. the direct position p = i:                        frames f ascending,  + ws[f][p + N/2 - f hop]
//   2. the left mirror p = -i        (1 <= i <= N/2):    frames ascending
//   3. the right mirror p = 2(L-1)-i (i < L-1, p < L + N/2): frames ascending
// (a frame holds p when 0 <= p + N/2 - f hop < N).  With accumulate the sum is then added to dy[i]: dy[i] = dy[i] + sum.
// Samples before `skip` get 0 (accumulate: stay as they are).
struct StftGradArgs {
    const float *y, *t, *coef;
    float *ws;
    int64_t B, T, skip;
    int hop, win, chunks, frames_per_chunk, n_frames;
    float eps;
};

// Periodic Hann value 0.5 - 0.5 cos(2 pi n / win) = sin^2(pi n / win), 0 <= n < win, correctly rounded to fp32: the gradient of
// the log-magnitude term goes with 1/mag^2 at small-magnitude cells, where every absolute error of the spectrum counts, and
// the fp32 argument 2n/win of stft_sums_kernel's window (exact for a power-of-two win only) costs 2e-7 of the window's peak --
// twice the roundoff of the transform itself.  sin by symmetry on [0, pi/4] (m = min(n, win - n); beyond win/4 the cosine of
// the complement), Taylor series in fp64 (truncation below 1e-12); step = pi / (2 win).
__device__ __forceinline__ float hann_rounded(int n, int win, double step)
{
    const int m = min(n, win - n);
    const bool upper = 4 * m > win;
    const double y = step * (double)(upper ? win - 2 * m : 2 * m), y2 = y * y;
    const double sn = y * (1.0 + y2 * (-1.0 / 6 + y2 * (1.0 / 120 + y2 * (-1.0 / 5040 + y2 * (1.0 / 362880 + y2 * (-1.0 / 39916800
                      + y2 * (1.0 / 6227020800.0)))))));
    const double cs = 1.0 + y2 * (-0.5 + y2 * (1.0 / 24 + y2 * (-1.0 / 720 + y2 * (1.0 / 40320 + y2 * (-1.0 / 3628800
                      + y2 * (1.0 / 479001600 + y2 * (-1.0 / 87178291200.0)))))));
    const double s = upper ? cs : sn;
    return (float)(s * s);
}

template <int LOG2N>
__global__ __launch_bounds__(256, (LOG2N <= 10 ? 2 : 1)) void stft_grad_frames_kernel(StftGradArgs a)
{
    constexpr int N = 1 << LOG2N;
    using G = Geo<N>;
    constexpr int SUB = G::SUB, P = G::P, FPW = G::FPW, NPAD = G::NPAD;
    using PL = Plan<LOG2N>;
    constexpr int R0 = PL::R0, R1 = PL::R1, R2 = PL::R2, R3 = PL::R3;
    static_assert(R0 * R1 * R2 * R3 == N, "radix plan");
    extern __shared__ f2 stft_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sl = lane & (SUB - 1), fs = lane / SUB;
    f2 *buf = stft_smem + (wave * FPW + fs) * NPAD;

    PassTw<N, R1, R0> tw1;
    PassTw<N, R2, R0 * R1> tw2;
    PassTw<N, (R3 > 1 ? R3 : 2), R0 * R1 * R2 / (R3 > 1 ? 1 : 2)> tw3;      // (unused when R3 == 1)
    tw1.init(sl);
    tw2.init(sl);
    if constexpr (R3 > 1) tw3.init(sl);

    const int left = (N - a.win) / 2;
    const double hann_step = 1.5707963267948966 / (double)a.win;
    float wreg[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const int n = sl + SUB * q - left;
        wreg[q] = (n >= 0 && n < a.win) ? hann_rounded(n, a.win, hann_step) : 0.0f;
    }

    const int64_t stream = blockIdx.x / a.chunks;
    const int chunk = blockIdx.x % a.chunks;
    const int L = (int)(a.T - a.skip);
    const float *ys = a.y + stream * a.T + a.skip;
    const float *ts = a.t + stream * a.T + a.skip;
    float *wss = a.ws + (size_t)stream * a.n_frames * N;
    const int f_begin = chunk * a.frames_per_chunk;
    const int f_end = min(f_begin + a.frames_per_chunk, a.n_frames);
    constexpr int FSTEP = 4 * FPW;

    const float csc_half = 0.5f * a.coef[stream * 3], clog2 = 2.0f * a.coef[stream * 3 + 1], clin = a.coef[stream * 3 + 2];
    const float eps4 = 4.0f * a.eps;                           // floor of the unscaled (4 x) powers, see split_spectra
    float ry[P], rt[P];
    auto fetch = [&](int f) {
        if (f >= f_end) f = f_begin;                        // idle slot of a multi-frame wave: reload, nothing is stored for it
        const int start = f * a.hop - N / 2;
        if (FPW == 1 && start >= 0 && start + N <= L) {
            const float *py = ys + start + sl, *pt = ts + start + sl;
#pragma unroll
            for (int q = 0; q < P; ++q) { ry[q] = py[SUB * q]; rt[q] = pt[SUB * q]; }
        } else {
#pragma unroll
            for (int q = 0; q < P; ++q) {
                int i = start + sl + SUB * q;
                i = i < 0 ? -i : i;
                i = i >= L ? 2 * (L - 1) - i : i;
                ry[q] = ys[i]; rt[q] = ts[i];
            }
        }
    };
    const int f_first = f_begin + wave * FPW;
    if (f_first < f_end) fetch(f_first + fs);
    for (int f0 = f_first; f0 < f_end; f0 += FSTEP) {
        const int f = f0 + fs;
        const bool live = f < f_end;
        f2 v[P];
#pragma unroll
        for (int q = 0; q < P; ++q) v[q] = (f2){wreg[q] * ry[q], wreg[q] * rt[q]};
        PassTw<N, R0, 1> tw0;
        stockham_pass<N, R0, 1, true>(v, buf, tw0, sl);
        stockham_pass<N, R1, R0, false>(v, buf, tw1, sl);
        if (f0 + FSTEP < f_end) fetch(f + FSTEP);              // (placed as in stft_sums_kernel)
        stockham_pass<N, R2, R0 * R1, false>(v, buf, tw2, sl);
        if constexpr (R3 > 1) stockham_pass<N, R3, R0 * R1 * R2, false>(v, buf, tw3, sl);
        wave_lds_fence();
        // ---- conj c_k of this lane's bins: its points q < P/2 of the second transform (bin N/2: point P/2 of lane 0) ----
        auto cbin = [&](int k) -> f2 {
            const f2 zk = buf[padi(k)], zn = buf[padi((N - k) & (N - 1))];
            f2 Y2, T2;
            split_spectra(zk, zn, Y2, T2);
            const f2 ysq = Y2 * Y2, tsq = T2 * T2;
            const float py0 = ysq.x + ysq.y, pt0 = tsq.x + tsq.y;                 // 4 x the powers
            const float my2 = __builtin_amdgcn_sqrtf(fmaxf(py0, eps4)), mt2 = __builtin_amdgcn_sqrtf(fmaxf(pt0, eps4));
            const float d = my2 - mt2;
            const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            const float inv = 1.0f / my2;
            const float g = csc_half * d + sg * (clog2 * inv + clin);
            const float s = py0 > eps4 ? g * inv : 0.0f;
            return (f2){s * Y2.x, -(s * Y2.y)};
        };
#pragma unroll
        for (int q = 0; q < P / 2; ++q) v[q] = cbin(sl + SUB * q);
        v[P / 2] = (f2){0.0f, 0.0f};
        if (sl == 0) v[P / 2] = cbin(N / 2);
#pragma unroll
        for (int q = P / 2 + 1; q < P; ++q) v[q] = (f2){0.0f, 0.0f};
        wave_lds_fence();                                      // every lane has read its bins: the buffer is free
        stockham_pass<N, R0, 1, true>(v, buf, tw0, sl);
        stockham_pass<N, R1, R0, false>(v, buf, tw1, sl);
        stockham_pass<N, R2, R0 * R1, false>(v, buf, tw2, sl);
        if constexpr (R3 > 1) stockham_pass<N, R3, R0 * R1 * R2, false>(v, buf, tw3, sl);
        wave_lds_fence();
        if (live) {
            float *o = wss + (size_t)f * N + sl;
#pragma unroll
            for (int q = 0; q < P; ++q) o[SUB * q] = wreg[q] * buf[padi(sl + SUB * q)].x;
        }
        wave_lds_fence();
    }
}

__global__ __launch_bounds__(256) void stft_grad_gather_kernel(const float *ws, float *dy, int64_t B, int64_t T, int64_t skip,
                                                               int N, int hop, int n_frames, int accumulate)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * T) return;
    const int64_t b = idx / T, j = idx - b * T;
    if (j < skip) {
        if (!accumulate) dy[idx] = 0.0f;
        return;
    }
    const int64_t i = j - skip, L = T - skip;
    const float *w = ws + (size_t)b * n_frames * N;
    float s = 0.0f;
    auto add = [&](int64_t p) {                     // every frame that holds padded position p, ascending
        const int64_t q = p + N / 2;                // position in the padded signal, >= 0
        const int64_t f_lo = q >= N ? (q - N) / hop + 1 : 0;
        const int64_t f_hi = min(q / hop, (int64_t)n_frames - 1);
        for (int64_t f = f_lo; f <= f_hi; ++f) s += w[f * N + (q - f * hop)];
    };
    add(i);
    if (i >= 1 && i <= N / 2) add(-i);
    const int64_t pr = 2 * (L - 1) - i;
    if (i < L - 1 && pr < L + N / 2) add(pr);
    dy[idx] = accumulate ? dy[idx] + s : s;
}

template <int LOG2N>
static hipError_t launch_grad_frames(StftGradArgs &a, hipStream_t stream)
{
    constexpr int N = 1 << LOG2N, FSTEP = 4 * Geo<N>::FPW;
    // whole iterations of a workgroup per chunk, about 1024 workgroups; every frame is written once by one wave, so the
    // result does not depend on the split
    const int iters = (a.n_frames + FSTEP - 1) / FSTEP;
    const int want = (int)min((int64_t)iters, max((int64_t)1, (1024 + a.B - 1) / a.B));
    a.frames_per_chunk = (iters + want - 1) / want * FSTEP;
    a.chunks = (a.n_frames + a.frames_per_chunk - 1) / a.frames_per_chunk;
    const size_t smem = (size_t)4 * Geo<N>::FPW * Geo<N>::NPAD * sizeof(f2);
    auto k = stft_grad_frames_kernel<LOG2N>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)(a.B * a.chunks)), dim3(256), smem, stream, a);
    return hipGetLastError();
}

hipError_t launch_stft_grad(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop, int win,
                            float eps, const float *coef, float *ws, float *dy, int accumulate, hipStream_t stream)
{
    StftGradArgs a;
    a.y = y; a.t = t; a.coef = coef; a.ws = ws; a.B = B; a.T = T; a.skip = skip; a.hop = hop; a.win = win; a.eps = eps;
    a.n_frames = (int)(1 + (T - skip) / hop);
    hipError_t e;
    switch (n_fft) {
    case 64: e = launch_grad_frames<6>(a, stream); break;
    case 128: e = launch_grad_frames<7>(a, stream); break;
    case 256: e = launch_grad_frames<8>(a, stream); break;
    case 512: e = launch_grad_frames<9>(a, stream); break;
    case 1024: e = launch_grad_frames<10>(a, stream); break;
    case 2048: e = launch_grad_frames<11>(a, stream); break;
    default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stft_grad_gather_kernel, dim3((unsigned)((B * T + 255) / 256)), dim3(256), 0, stream, ws, dy, B, T, skip,
                       n_fft, hop, a.n_frames, accumulate);
    return hipGetLastError();
}

// ---- the power spectrogram itself (ntm_spectrogram) and its adjoint (ntm_spectrogram_grad): the front end of the
// reference's spectral critics (TimeFreqConverter, code/utilities/utilities.py:627-672), whose output a network reads and
// whose input gets a gradient.
//
//   P[b][k][f] = |STFT(y_b)[k, f]|^2,   k = 0 .. N/2,  f = 0 .. T / hop       (frames, padding, window placement: stft_sums_kernel's)
//   g_f[n] = w[n] Re sum_{k=0}^{N/2} conj(c_k) e^{-2 pi i k n / N},   c_k = 2 gP[b][k][f] Y_k
//
// ARITHMETIC: fp64 inside (window, twiddles, transform, powers, c), fp32 at the interfaces (y, P, gP, the workspace).  A
// network behind P divides by it -- the critics take log10(P + 1e-5) -- so a cell of small power multiplies the ABSOLUTE error
// of Y, which in an fp32 transform is the roundoff of the frame's largest bins, by up to 1/(P + 1e-5): the fp32 form of this
// kernel (the packed-fp32 passes of stft_sums_kernel) was within a quarter of the bar on the spectrogram and on its adjoint and
// 8 x above it on the gradient of such a head.  In fp64 the error of a cell is its own rounding to fp32.  The
// vector unit runs fp64 at the rate of unpacked fp32, and the calls are short, so the passes are plain: Stockham autosort,
// radix 4 (one radix-2 pass at the end for an odd log2 N), the lane / point / exchange-buffer mapping of stockham_pass
// (v[q] = point sl + SUB q, one padded buffer per frame slot, wave-level fences), twiddles from one table
// e^{-2 pi i j / N}, j < N, that the workgroup fills in LDS at its start (sincospi in fp64).
//
// Mapping: ONE signal, so a frame slot packs two FRAMES of the stream, z = w (y_f + i y_{f+1}), f even, into the one complex
// transform and separates them afterwards (2 Y_a[k] = Z[k] + conj Z[N-k], 2 Y_b[k] = (Z[k] - conj Z[N-k]) / i); the exact factor
// 1/4 of the powers is applied to each stored value.  The pairs are (2j, 2j + 1) of the stream whatever the split into chunks
// (a chunk is whole iterations), and a last frame without a partner is paired with ITSELF, so a cell's bits depend neither on
// the batch nor on the chunk count.  A slot with no frame at all reloads the chunk's first frame and stores nothing.  The
// frame loop is uniform over the workgroup (it holds two workgroup barriers, see the tile); a workgroup of WAVES waves and
// iteration covers TF = 2 * WAVES * 64/SUB consecutive frames (WAVES = 4; 2 at n_fft 2048, where four fp64 buffers, the
// table and the tile do not fit the LDS).
//
// The tile: P and gP are [B][bins][frames] (torch's layout: bins are the channels of the critics' Conv1d), and a lane owns
// bins sl + SUB i of its two frames -- a direct access is 64 runs of 8 bytes `frames` floats apart per instruction.  The
// workgroup stages [bins][TF] floats (row stride TF + 1) in LDS behind the exchange buffers instead: the waves write / read
// their columns there, and all threads move the tile with f running along the lanes (runs of TF floats).
//
// Adjoint (ADJ): Re FFT(conj c_a + i conj c_b) does not separate two frames, so c is extended Hermitian-symmetrically:
// d_k = conj(c_k) / 2, d_{N-k} = c_k / 2 (0 < k < N/2), d_0 = Re c_0, d_{N/2} = Re c_{N/2}.  FFT(d) is then real and equal
// to the sum above (every bin of 0 .. N/2 once, no 1/N, no doubling), so FFT(d_a + i d_b) = g_a / w + i g_b / w: two frames
// share the second transform as they share the first -- two transforms per frame pair where a transform per frame would take
// three.  The lane that owns bin k writes z_k and z_{N-k} into the exchange buffer in place (nobody else reads those two),
// and the first pass of the second transform reads its points like every later pass.  With 2 Y from the separation,
// conj(c_k) / 2 = (gP / 2) conj(2 Y_k): the halving is exact.  The windowed frame gradients go, rounded to fp32, to
// ws[stream][frame][n]; stft_grad_gather_kernel (skip 0) adds them up in its fixed order.
struct SpecArgs {
    const float *y, *gp;     // gp: the upstream gradient (ADJ)
    float *out;              // P, or ws (ADJ)
    int64_t B, T;
    int hop, win, chunks, frames_per_chunk, n_frames;
};

typedef double d2 __attribute__((ext_vector_type(2)));

template <int N> struct SpecGeo {
    static constexpr int WAVES = N >= 2048 ? 2 : 4;
    static constexpr int NT = 64 * WAVES;                  // threads of a workgroup
    static constexpr int NB = N / 2 + 1;                   // bins
    static constexpr int TF = 2 * WAVES * Geo<N>::FPW;     // frames per workgroup and iteration: WAVES x FPW slots x 2
    static constexpr int TS = TF + 1;                      // tile row stride (floats): odd, the column accesses spread over the banks
    static constexpr int SLOTS = WAVES * Geo<N>::FPW;
    static constexpr size_t smem = ((size_t)SLOTS * Geo<N>::NPAD + N) * sizeof(d2) + (size_t)NB * TS * sizeof(float);
};

__device__ __forceinline__ d2 cmul_d(d2 a, d2 b) { return (d2){a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// One Stockham pass in fp64, radix R in {2, 4}, sub-transform size Ns: stockham_pass's mapping (v[q] = point sl + SUB q; butterfly b
// of a lane is j = sl + SUB b, k = j mod Ns, input t times e^{-2 pi i t k / (Ns R)} = tab[t k N / (Ns R)]).
template <int N, int R, int Ns, bool FIRST>
__device__ __forceinline__ void spec_pass(d2 (&v)[Geo<N>::P], d2 *buf, const d2 *tab, int sl)
{
    constexpr int SUB = Geo<N>::SUB, P = Geo<N>::P, NB = N / R / SUB;
    static_assert(NB >= 1 && (R == 2 || R == 4), "radix");
    if constexpr (!FIRST) {
        wave_lds_fence();
#pragma unroll
        for (int q = 0; q < P; ++q) v[q] = buf[padi(sl + SUB * q)];
        wave_lds_fence();
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = sl + SUB * b;
        const int k = j & (Ns - 1);
        d2 x[R];
#pragma unroll
        for (int t = 0; t < R; ++t) x[t] = v[b + t * NB];
        if constexpr (Ns > 1) {
#pragma unroll
            for (int t = 1; t < R; ++t) x[t] = cmul_d(x[t], tab[t * k * (N / (Ns * R))]);
        }
        if constexpr (R == 2) {
            const d2 t0 = x[0];
            x[0] = t0 + x[1]; x[1] = t0 - x[1];
        } else {
            const d2 s02 = x[0] + x[2], d02 = x[0] - x[2], s13 = x[1] + x[3], d13 = x[1] - x[3];
            x[0] = s02 + s13; x[1] = (d2){d02.x + d13.y, d02.y - d13.x};
            x[2] = s02 - s13; x[3] = (d2){d02.x - d13.y, d02.y + d13.x};
        }
        const int o = (j - k) * R + k;
#pragma unroll
        for (int m = 0; m < R; ++m) buf[padi(o + m * Ns)] = x[m];
    }
}

// the passes from sub-transform size Ns up: radix 4 while it fits, then one radix 2.  FIRST: the points are in v (else in buf)
template <int N, int Ns, bool FIRST>
__device__ __forceinline__ void spec_fft(d2 (&v)[Geo<N>::P], d2 *buf, const d2 *tab, int sl)
{
    if constexpr (Ns < N) {
        constexpr int R = N / Ns >= 4 ? 4 : 2;
        spec_pass<N, R, Ns, FIRST>(v, buf, tab, sl);
        spec_fft<N, Ns * R, false>(v, buf, tab, sl);
    }
}

template <int LOG2N, bool ADJ>
__global__ __launch_bounds__(SpecGeo<(1 << LOG2N)>::NT) void spectrogram_kernel(SpecArgs a)
{
    constexpr int N = 1 << LOG2N;
    using G = Geo<N>;
    using SG = SpecGeo<N>;
    constexpr int SUB = G::SUB, P = G::P, FPW = G::FPW, NPAD = G::NPAD;
    constexpr int NB = SG::NB, TF = SG::TF, TS = SG::TS, NT = SG::NT;
    extern __shared__ f2 stft_smem[];
    d2 *smem = reinterpret_cast<d2 *>(stft_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sl = lane & (SUB - 1), fs = lane / SUB;
    d2 *buf = smem + (wave * FPW + fs) * NPAD;                               // this frame slot's exchange buffer
    d2 *tab = smem + SG::SLOTS * NPAD;                                       // e^{-2 pi i j / N}, j < N
    float *tile = reinterpret_cast<float *>(tab + N);                        // [NB][TS]
    const int col = 2 * (wave * FPW + fs);                                   // this slot's two columns of the tile

    for (int j = tid; j < N; j += NT) {
        double sn, cs;
        sincospi(-2.0 * (double)j / (double)N, &sn, &cs);
        tab[j] = (d2){cs, sn};
    }
    // periodic Hann of `win` samples, centred in n_fft: sin^2(pi n / win) in fp64
    const int left = (N - a.win) / 2;
    double wreg[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const int n = sl + SUB * q - left;
        const double sn = sinpi((double)n / (double)a.win);
        wreg[q] = (n >= 0 && n < a.win) ? sn * sn : 0.0;
    }
    __syncthreads();                                                         // the table is complete

    const int64_t stream = blockIdx.x / a.chunks;
    const int chunk = blockIdx.x % a.chunks;
    const int L = (int)a.T;
    const float *ys = a.y + stream * a.T;
    const int f_begin = chunk * a.frames_per_chunk;                          // (a multiple of TF)
    const int f_end = min(f_begin + a.frames_per_chunk, a.n_frames);
    const size_t cells = (size_t)stream * NB * a.n_frames;                   // this stream's [NB][n_frames] of P / gP

    for (int fb = f_begin; fb < f_end; fb += TF) {          // uniform over the workgroup
        int fa = fb + col;
        const bool live_a = fa < f_end, live_b = fa + 1 < f_end;
        if (!live_a) fa = f_begin;                          // idle slot: reload a valid frame, nothing is stored for it
        const int fp = live_b ? fa + 1 : fa;                // no partner (odd frame count): the frame itself
        if constexpr (ADJ) {                                // the iteration's gP cells, f along the lanes (zero past the end)
            for (int idx = tid; idx < NB * TF; idx += NT) {
                const int k = idx / TF, fi = idx % TF;
                tile[k * TS + fi] = fb + fi < f_end ? a.gp[cells + (size_t)k * a.n_frames + fb + fi] : 0.0f;
            }
        }
        // z = w (y_fa + i y_fp), samples reflected at the ends (torch.stft center=True, pad_mode="reflect")
        d2 v[P];
        const int sa = fa * a.hop - N / 2 + sl, sp = fp * a.hop - N / 2 + sl;    // (T < 2^31 - n_fft: checked by the API)
#pragma unroll
        for (int q = 0; q < P; ++q) {
            int ia = sa + SUB * q, ip = sp + SUB * q;
            ia = ia < 0 ? -ia : ia;
            ia = ia >= L ? 2 * (L - 1) - ia : ia;
            ip = ip < 0 ? -ip : ip;
            ip = ip >= L ? 2 * (L - 1) - ip : ip;
            v[q] = (d2){wreg[q] * (double)ys[ia], wreg[q] * (double)ys[ip]};
        }
        spec_fft<N, 1, true>(v, buf, tab, sl);
        if constexpr (!ADJ) {
            wave_lds_fence();
            auto bin = [&](int k) {                         // 4 x the powers of the slot's two frames -> its tile columns
                const d2 zk = buf[padi(k)], zn = buf[padi((N - k) & (N - 1))];
                const d2 A2 = {zk.x + zn.x, zk.y - zn.y}, B2 = {zk.y + zn.y, zn.x - zk.x};
                tile[k * TS + col] = (float)(0.25 * (A2.x * A2.x + A2.y * A2.y));
                tile[k * TS + col + 1] = (float)(0.25 * (B2.x * B2.x + B2.y * B2.y));
            };
#pragma unroll
            for (int i = 0; i < P / 2; ++i) bin(sl + SUB * i);
            if (sl == 0) bin(N / 2);
            __syncthreads();                                // the tile is complete
            for (int idx = tid; idx < NB * TF; idx += NT) {
                const int k = idx / TF, fi = idx % TF;
                if (fb + fi < f_end) a.out[cells + (size_t)k * a.n_frames + fb + fi] = tile[k * TS + fi];
            }
        } else {
            __syncthreads();                                // the tile is complete; every lane's transform is in its buffer
            auto bin = [&](int k) {                         // z_k and z_{N-k} of d_a + i d_b, in place
                const int kn = (N - k) & (N - 1);
                const d2 zk = buf[padi(k)], zn = buf[padi(kn)];
                const d2 A2 = {zk.x + zn.x, zk.y - zn.y}, B2 = {zk.y + zn.y, zn.x - zk.x};
                const double h = (k == 0 || k == N / 2) ? 1.0 : 0.5;        // (there A2.y = B2.y = 0 exactly, and kn = k)
                const double ga = h * (double)tile[k * TS + col], gb = h * (double)tile[k * TS + col + 1];
                const d2 da = {ga * A2.x, -(ga * A2.y)}, db = {gb * B2.x, -(gb * B2.y)};
                buf[padi(k)] = (d2){da.x - db.y, da.y + db.x};              // d_a + i d_b
                buf[padi(kn)] = (d2){da.x + db.y, db.x - da.y};             // conj d_a + i conj d_b
            };
#pragma unroll
            for (int i = 0; i < P / 2; ++i) bin(sl + SUB * i);
            if (sl == 0) bin(N / 2);
            spec_fft<N, 1, false>(v, buf, tab, sl);
            wave_lds_fence();
            if (live_a) {
                float *o = a.out + ((size_t)stream * a.n_frames + fa) * N + sl;
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    const d2 g = buf[padi(sl + SUB * q)];
                    o[SUB * q] = (float)(wreg[q] * g.x);
                    if (live_b) o[N + SUB * q] = (float)(wreg[q] * g.y);
                }
            }
        }
        __syncthreads();                                    // tile and exchange buffers are free for the next iteration
    }
}

template <int LOG2N, bool ADJ>
static hipError_t launch_spec(SpecArgs &a, hipStream_t stream)
{
    constexpr int N = 1 << LOG2N, TF = SpecGeo<N>::TF;
    // whole iterations of a workgroup per chunk, about 1024 workgroups; every cell is written once, from a frame pair that
    // does not depend on the split
    const int iters = (a.n_frames + TF - 1) / TF;
    const int want = (int)min((int64_t)iters, max((int64_t)1, (1024 + a.B - 1) / a.B));
    a.frames_per_chunk = (iters + want - 1) / want * TF;
    a.chunks = (a.n_frames + a.frames_per_chunk - 1) / a.frames_per_chunk;
    auto k = spectrogram_kernel<LOG2N, ADJ>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SpecGeo<N>::smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)(a.B * a.chunks)), dim3(SpecGeo<N>::NT), SpecGeo<N>::smem, stream, a);
    return hipGetLastError();
}

template <bool ADJ>
static hipError_t launch_spec_n(int n_fft, SpecArgs &a, hipStream_t stream)
{
    switch (n_fft) {
    case 64: return launch_spec<6, ADJ>(a, stream);
    case 128: return launch_spec<7, ADJ>(a, stream);
    case 256: return launch_spec<8, ADJ>(a, stream);
    case 512: return launch_spec<9, ADJ>(a, stream);
    case 1024: return launch_spec<10, ADJ>(a, stream);
    case 2048: return launch_spec<11, ADJ>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_spectrogram(const float *y, int64_t B, int64_t T, int n_fft, int hop, int win, float *P, hipStream_t stream)
{
    SpecArgs a;
    a.y = y; a.gp = nullptr; a.out = P; a.B = B; a.T = T; a.hop = hop; a.win = win;
    a.n_frames = (int)(1 + T / hop);
    return launch_spec_n<false>(n_fft, a, stream);
}

hipError_t launch_spectrogram_grad(const float *y, const float *gP, int64_t B, int64_t T, int n_fft, int hop, int win, float *ws,
                                   float *dy, int accumulate, hipStream_t stream)
{
    SpecArgs a;
    a.y = y; a.gp = gP; a.out = ws; a.B = B; a.T = T; a.hop = hop; a.win = win;
    a.n_frames = (int)(1 + T / hop);
    hipError_t e = launch_spec_n<true>(n_fft, a, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stft_grad_gather_kernel, dim3((unsigned)((B * T + 255) / 256)), dim3(256), 0, stream, ws, dy, B, T,
                       (int64_t)0, n_fft, hop, a.n_frames, accumulate);
    return hipGetLastError();
}

}   // namespace ntm
