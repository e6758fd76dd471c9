// The conv stack of the reference's spectral critics (SpecCrit, code/critics.py:181-259) behind the spectrogram: n weight-normed
// Conv1d(c_in, c_out, k, groups) layers, stride 1, dilation 1, no padding, LeakyReLU(0.2) after every layer but the last.  What it
// shares with the dilated and the MelGAN family (the plan, weight preparation, weight-norm adjoint) is convstack_common.h; this
// file holds its GEMM kernels: the SLAB fetch form of the conv kernel with the log head, its weight gradient, and the chunk rule.
// Tile shapes as in convstack_kernels.hip.
//
// crit_conv_kernel     the implicit GEMM along the frames: out[b][m][f] = sum_{c,j} W[j][c][m] in[b][c][f + j + off], one workgroup
//                      per (stream, group, tile of output channels, tile of frames).  A slab of 16 input channels x (tile + K - 1)
//                      frames sits in LDS once and every tap reads it shifted (the im2col matrix never exists); the weights follow
//                      4 taps at a time (TapMajorLayout).  A wave's MFMA takes 4 consecutive input channels of one tap as its K = 4.
//                        forward        off = 0,  W = wF; the HEAD form reads log10(max(x, floor)) as it fills the slab
//                        data gradient  the same sum with the roles of the channels swapped: in = gz (the gradient at the layer's
//                                       pre-activation), off = -(K-1) with zeros outside, W = wB; the epilogue of the first layer
//                                       under a log head is EPI_HEAD
//                      Epilogues: forward, bias -> LeakyReLU(0.2) (the last layer: bias).  Data gradient: times the LeakyReLU
//                      slope of the layer below, recovered from the sign of its saved output (y > 0 <=> pre > 0 as slope > 0;
//                      y == 0 takes the slope, torch's choice), so every stored gz is already a pre-activation gradient;
//                      EPI_HEAD, the first layer under the log head: 1 / (x ln 10) where x >= floor, else 0.
//                      Order of addition of one output: per slab of 16 input channels a sum from 0, taps ascending and per tap
//                      the channels in fours (one MFMA each, its K = 4 an fmaf chain); the slab sums are then added in ascending
//                      order -- a function of the layer alone, so a stream's result does not depend on its batch.  The loads of
//                      the next step (slab, 4 taps) are in flight during the MFMAs of the current one.
// crit_wgrad_kernel    dW[co][ci][k] = sum_{b,f} gz[b][co][f] in[b][ci][f + k]: GEMM with M = co, N = (ci, k) flattened as dW is
//                      stored, reduction over the frames (64 per step, the MFMA's K = 4 consecutive frames), the X operand a slab
//                      in LDS (every column a shifted read of it) and a SINGLE-level sum over the frames.
//                      Chunk rule: the streams in at most 32 contiguous chunks, one segment; a workgroup adds the streams of its
//                      chunk in order and stores ONE partial tile, no atomics.
#include "convstack_common.h"

namespace ntm {

constexpr int kCritMaxChunks = 32;

void crit_plan(StackPlan &p, int64_t B, int64_t C0, int64_t F0, int n, const ntm_conv1d_layer *L)
{
    stack_plan_layers(p, B, F0, n, L, true, [&](int l, int64_t F) { return F - L[l].k + 1; });
    for (int l = 0; l < n; ++l) {
        stack_stream_chunks(B, kCritMaxChunks, p.nchunk[l], p.per[l]);
        p.seg[l] = p.F[l + 1], p.nseg[l] = 1;
    }
    stack_plan_partials(p);
}

namespace {

constexpr float kSlope = 0.2f;
constexpr float kLn10 = 2.302585092994046f;

enum { EPI_BIAS_LRELU = 0, EPI_BIAS = 1, EPI_MASK = 2, EPI_HEAD = 3, EPI_NONE = 4 };

struct ConvArgs {
    const float *in;    // [B][Cin][Fin]
    const float *w;     // [K][cin_g][Cout]
    const float *bias;  // EPI_BIAS*: [Cout]
    const float *aux;   // EPI_MASK: the saved output this gradient belongs to; EPI_HEAD: x; in out's layout
    float *out;         // [B][Cout][Fout]
    int Cin, Cout, cin_g, cout_g, K, Fin, Fout, off, in_log, epi, mtiles, ntiles, PX;
    float floor_;
};

constexpr int kCI = 16;   // input channels per LDS slab
constexpr int kKT = 4;    // taps per weight slab

// LDS pitches are 16 mod 64 floats: the four K-lanes groups of an MFMA operand read (16 consecutive floats of four
// consecutive rows) then fall on 64 different banks
__host__ __device__ constexpr int conv_pa(int TM) { return TM == 16 ? 16 : TM + 16; }
inline int pitch16(int w) { return ((w - 16 + 63) / 64) * 64 + 16; }

template <int WM, int RM, int WN, int RN>
__global__ __launch_bounds__(256) void crit_conv_kernel(ConvArgs a)
{
    constexpr int TM = WM * RM * 16, TN = WN * RN * 16, PA = conv_pa(TM);
    extern __shared__ float lds[];
    float *As = lds, *Xs = lds + kKT * kCI * PA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM, li = lane & 15, kq = lane >> 4;
    const int64_t b = blockIdx.x / a.ntiles;
    const int n0 = (int)(blockIdx.x % a.ntiles) * TN;
    const int grp = blockIdx.y / a.mtiles, m0 = (blockIdx.y % a.mtiles) * TM;
    const int K = a.K, PX = a.PX, TNX = TN + K - 1;
    const float *inb = a.in + (b * a.Cin + (int64_t)grp * a.cin_g) * a.Fin;

    // acc: the sum over the current slab of 16 input channels (all taps), tot: the slabs added up -- a two-level sum, so that a
    // reduction 10 250 deep (1025 bins x 10 taps) is sums of 160 products and 65 additions instead of one chain of 10 250
    f32x4 acc[RM][RN], tot[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) acc[i][j] = tot[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // one step = (slab of 16 input channels, 4 taps).  The global loads of step it + 1 are issued into registers before the MFMAs
    // of step it and stored to LDS after them, so their latency hides behind the matrix pipe (the order of addition is the loop's)
    constexpr int AR = kKT * kCI * TM / 256, XR = (kCI * (TN + 63) + 255) / 256;
    const int nk = (K + kKT - 1) / kKT, nit = ((a.cin_g + kCI - 1) / kCI) * nk;
    float ra[AR], rx[XR];
    auto fetch = [&](int it) {
        const int c0 = (it / nk) * kCI, k0 = (it % nk) * kKT;
#pragma unroll
        for (int q = 0; q < AR; ++q) {
            const int e = tid + q * 256, r = e / TM, m = e - r * TM, kt = r / kCI, cl = r - kt * kCI;
            float val = 0.0f;
            if (k0 + kt < K && c0 + cl < a.cin_g && m0 + m < a.cout_g)
                val = a.w[((int64_t)(k0 + kt) * a.cin_g + c0 + cl) * a.Cout + grp * a.cout_g + m0 + m];
            ra[q] = val;
        }
        if (k0 == 0) {
#pragma unroll
            for (int q = 0; q < XR; ++q) {
                const int e = tid + q * 256, cl = e / TNX, t = e - cl * TNX, fr = n0 + t + a.off;
                float val = a.in_log ? 1.0f : 0.0f;                 // log10(1) = 0
                if (e < kCI * TNX && c0 + cl < a.cin_g && fr >= 0 && fr < a.Fin) val = inb[(int64_t)(c0 + cl) * a.Fin + fr];
                rx[q] = val;
            }
        }
    };
    auto stash = [&](int it) {
#pragma unroll
        for (int q = 0; q < AR; ++q) {
            const int e = tid + q * 256, r = e / TM, m = e - r * TM;
            As[r * PA + m] = ra[q];
        }
        if (it % nk == 0) {
#pragma unroll
            for (int q = 0; q < XR; ++q) {
                const int e = tid + q * 256, cl = e / TNX, t = e - cl * TNX;
                if (e < kCI * TNX) Xs[cl * PX + t] = a.in_log ? log10f(fmaxf(rx[q], a.floor_)) : rx[q];
            }
        }
    };
    fetch(0);
    for (int it = 0; it < nit; ++it) {
        __syncthreads();
        stash(it);
        __syncthreads();
        if (it + 1 < nit) fetch(it + 1);
        const int c0 = (it / nk) * kCI, k0 = (it % nk) * kKT;
        const int cn = min(4, (a.cin_g - c0 + 3) >> 2);     // groups of 4 channels this slab holds
        const int kn = min(kKT, K - k0);
        for (int kt = 0; kt < kn; ++kt)
            for (int c4 = 0; c4 < cn; ++c4) {
                const int row = c4 * 4 + kq;
                float av[RM], bv[RN];
#pragma unroll
                for (int i = 0; i < RM; ++i) av[i] = As[(kt * kCI + row) * PA + (wm * RM + i) * 16 + li];
#pragma unroll
                for (int j = 0; j < RN; ++j) bv[j] = Xs[row * PX + (wn * RN + j) * 16 + li + k0 + kt];
#pragma unroll
                for (int i = 0; i < RM; ++i)
#pragma unroll
                    for (int j = 0; j < RN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            }
        if ((it + 1) % nk == 0) {                           // the slab is complete
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j) {
                    tot[i][j] += acc[i][j];
                    acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
        }
    }

#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            const int f = n0 + (wn * RN + j) * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wm * RM + i) * 16 + kq * 4 + r;
                if (m < a.cout_g && f < a.Fout) {
                    const int co = grp * a.cout_g + m;
                    const int64_t idx = (b * a.Cout + co) * a.Fout + f;
                    float v = tot[i][j][r];
                    if (a.epi == EPI_BIAS_LRELU) {
                        v += a.bias[co];
                        v = v > 0.0f ? v : v * kSlope;
                    } else if (a.epi == EPI_BIAS) {
                        v += a.bias[co];
                    } else if (a.epi == EPI_MASK) {
                        v = a.aux[idx] > 0.0f ? v : v * kSlope;
                    } else if (a.epi == EPI_HEAD) {
                        const float x = a.aux[idx];
                        v = x >= a.floor_ ? v / (x * kLn10) : 0.0f;
                    }
                    a.out[idx] = v;
                }
            }
        }
}

struct WgradArgs {
    const float *gz;   // [B][Cout][Fout]
    const float *in;   // [B][Cin][Fin], Fin = Fout + K - 1
    float *part;       // [chunk][Cout][cin_g * K]
    float *bpart;      // [chunk][Cout]
    int Cin, Cout, cin_g, cout_g, K, Fin, Fout, in_log, mtiles, nch, PX, per;
    int64_t B;
    float floor_;
};

constexpr int kTF = 64;   // frames per reduction step
constexpr int kPG = 68;   // pitch of the gz tile: 4 mod 64, so (16 rows) x (4 consecutive frames) fall on 64 different banks

template <int WM, int RM, int WN, int RN>
__global__ __launch_bounds__(256) void crit_wgrad_kernel(WgradArgs a)
{
    constexpr int TM = WM * RM * 16, TN = WN * RN * 16;
    extern __shared__ float lds[];
    float *Gs = lds, *Xs = lds + TM * kPG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM, li = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.x * TN, grp = blockIdx.y / a.mtiles, m0 = (blockIdx.y % a.mtiles) * TM;
    const int K = a.K, PX = a.PX, n = a.cin_g * K, W = kTF + K - 1, cbase = j0 / K;
    const int chunk = blockIdx.z;

    int offB[RN];
#pragma unroll
    for (int jj = 0; jj < RN; ++jj) {
        const int j = j0 + (wn * RN + jj) * 16 + li;
        const int ci = j / K;
        offB[jj] = j < n ? (ci - cbase) * PX + (j - ci * K) : 0;
    }
    f32x4 acc[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float bsum = 0.0f;

    // one step = 64 frames of one stream of the chunk; the loads of the next step are in flight during the MFMAs of this one
    constexpr int GR = TM * kTF / 256, XR = 17;             // nch * W <= 65 * 64 floats (K = 1)
    const int64_t b_begin = (int64_t)chunk * a.per, b_end = min((int64_t)(chunk + 1) * a.per, a.B);
    const int nf = (a.Fout + kTF - 1) / kTF, nit = (int)(b_end - b_begin) * nf;
    float rg[GR], rx[XR];
    auto fetch = [&](int it) {
        const int64_t b = b_begin + it / nf;
        const int f0 = (it % nf) * kTF;
        const float *gb = a.gz + (b * a.Cout + (int64_t)grp * a.cout_g + m0) * a.Fout;
        const float *xb = a.in + (b * a.Cin + (int64_t)grp * a.cin_g + cbase) * a.Fin;
#pragma unroll
        for (int q = 0; q < GR; ++q) {
            const int e = tid + q * 256, m = e / kTF, t = e - m * kTF;
            rg[q] = (m0 + m < a.cout_g && f0 + t < a.Fout) ? gb[(int64_t)m * a.Fout + f0 + t] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < XR; ++q) {
            const int e = tid + q * 256, cl = e / W, t = e - cl * W;
            float val = a.in_log ? 1.0f : 0.0f;                     // log10(1) = 0
            if (e < a.nch * W && cbase + cl < a.cin_g && f0 + t < a.Fin) val = xb[(int64_t)cl * a.Fin + f0 + t];
            rx[q] = val;
        }
    };
    fetch(0);
    for (int it = 0; it < nit; ++it) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < GR; ++q) {
            const int e = tid + q * 256, m = e / kTF, t = e - m * kTF;
            Gs[m * kPG + t] = rg[q];
        }
#pragma unroll
        for (int q = 0; q < XR; ++q) {
            const int e = tid + q * 256, cl = e / W, t = e - cl * W;
            if (e < a.nch * W) Xs[cl * PX + t] = a.in_log ? log10f(fmaxf(rx[q], a.floor_)) : rx[q];
        }
        __syncthreads();
        if (it + 1 < nit) fetch(it + 1);
        if (blockIdx.x == 0 && tid < TM)
            for (int t = 0; t < kTF; ++t) bsum += Gs[tid * kPG + t];
        for (int f4 = 0; f4 < kTF; f4 += 4) {
            float av[RM], bv[RN];
#pragma unroll
            for (int i = 0; i < RM; ++i) av[i] = Gs[((wm * RM + i) * 16 + li) * kPG + f4 + kq];
#pragma unroll
            for (int j = 0; j < RN; ++j) bv[j] = Xs[offB[j] + f4 + kq];
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }

#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int jj = 0; jj < RN; ++jj) {
            const int j = j0 + (wn * RN + jj) * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wm * RM + i) * 16 + kq * 4 + r;
                if (m < a.cout_g && j < n)
                    a.part[((int64_t)chunk * a.Cout + grp * a.cout_g + m) * n + j] = acc[i][jj][r];
            }
        }
    if (blockIdx.x == 0 && tid < TM && m0 + tid < a.cout_g)
        a.bpart[(int64_t)chunk * a.Cout + grp * a.cout_g + m0 + tid] = bsum;
}

hipError_t launch_conv(ConvArgs a, int64_t B, int groups, hipStream_t stream)
{
    const bool narrow = a.cout_g <= 16;
    const int TM = narrow ? 16 : 64, TN = narrow ? 128 : 64;
    a.mtiles = (a.cout_g + TM - 1) / TM;
    a.ntiles = (a.Fout + TN - 1) / TN;
    a.PX = pitch16(TN + a.K - 1);
    const size_t lds = (size_t)(kKT * kCI * conv_pa(TM) + kCI * a.PX) * sizeof(float);
    const dim3 grid((unsigned)(B * a.ntiles), (unsigned)(groups * a.mtiles));
    if (narrow)
        hipLaunchKernelGGL((crit_conv_kernel<1, 1, 4, 2>), grid, dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL((crit_conv_kernel<2, 2, 2, 2>), grid, dim3(256), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_wgrad(WgradArgs a, int groups, int nchunk, hipStream_t stream)
{
    const bool narrow = a.cout_g <= 16;
    const int TM = narrow ? 16 : 64, W = kTF + a.K - 1;
    a.mtiles = (a.cout_g + TM - 1) / TM;
    a.nch = 63 / a.K + 2;
    a.PX = ((W - 8 + 31) / 32) * 32 + 8;
    const size_t lds = (size_t)(TM * kPG + a.nch * a.PX) * sizeof(float);
    const dim3 grid((unsigned)((a.cin_g * a.K + 63) / 64), (unsigned)(groups * a.mtiles), (unsigned)nchunk);
    if (narrow)
        hipLaunchKernelGGL((crit_wgrad_kernel<1, 1, 4, 1>), grid, dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL((crit_wgrad_kernel<2, 2, 2, 2>), grid, dim3(256), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_speccrit_forward(const StackPlan &p, const float *x, int64_t B, float log_floor, const float *const *g,
                                   const float *const *v, const float *const *bias, float *saved, float *out, hipStream_t stream)
{
    if (hipError_t e = launch_stack_prep<TapMajorLayout>(p, g, v, saved, stream)) return e;
    for (int l = 0; l < p.n; ++l) {
        const bool last = l == p.n - 1;
        ConvArgs a{};
        a.in = l ? saved + p.act_off[l - 1] : x;
        a.w = saved + p.w_off[l];
        a.bias = bias[l];
        a.out = last ? out : saved + p.act_off[l];
        a.Cin = p.c_in[l], a.Cout = p.c_out[l], a.cin_g = p.c_in[l] / p.groups[l], a.cout_g = p.c_out[l] / p.groups[l];
        a.K = p.k[l], a.Fin = (int)p.F[l], a.Fout = (int)p.F[l + 1], a.off = 0;
        a.in_log = l == 0 && log_floor > 0.0f, a.floor_ = log_floor;
        a.epi = last ? EPI_BIAS : EPI_BIAS_LRELU;
        if (hipError_t e = launch_conv(a, B, p.groups[l], stream)) return e;
    }
    return hipSuccess;
}

hipError_t launch_speccrit_backward(const StackPlan &p, const float *x, int64_t B, float log_floor, const float *const *g,
                                    const float *const *v, const float *saved, const float *gout, float *gx, float *const *dg,
                                    float *const *dv, float *const *dbias, float *ws, hipStream_t stream)
{
    const float *gz = gout;
    for (int l = p.n - 1; l >= 0; --l) {
        const int cin_g = p.c_in[l] / p.groups[l], cout_g = p.c_out[l] / p.groups[l];
        const float *in = l ? saved + p.act_off[l - 1] : x;
        const int in_log = l == 0 && log_floor > 0.0f;
        if (dg) {
            WgradArgs a{};
            a.gz = gz, a.in = in, a.part = ws + p.part_off[l], a.bpart = ws + p.bpart_off[l];
            a.Cin = p.c_in[l], a.Cout = p.c_out[l], a.cin_g = cin_g, a.cout_g = cout_g, a.K = p.k[l];
            a.Fin = (int)p.F[l], a.Fout = (int)p.F[l + 1], a.in_log = in_log, a.floor_ = log_floor, a.per = p.per[l], a.B = B;
            if (hipError_t e = launch_wgrad(a, p.groups[l], p.nchunk[l], stream)) return e;
        }
        if (l == 0 && !gx) break;
        float *dst = l ? ws + ((p.n - 1 - l) & 1) * p.gz_size : gx;
        ConvArgs a{};
        a.in = gz, a.w = saved + p.w_total + p.w_off[l], a.out = dst;
        a.aux = l ? saved + p.act_off[l - 1] : x;
        a.Cin = p.c_out[l], a.Cout = p.c_in[l], a.cin_g = cout_g, a.cout_g = cin_g;
        a.K = p.k[l], a.Fin = (int)p.F[l + 1], a.Fout = (int)p.F[l], a.off = -(p.k[l] - 1);
        a.in_log = 0, a.floor_ = log_floor;
        a.epi = l ? EPI_MASK : (in_log ? EPI_HEAD : EPI_NONE);
        if (hipError_t e = launch_conv(a, B, p.groups[l], stream)) return e;
        gz = dst;
    }
    return dg ? launch_stack_wnorm(p, p.n, g, v, dg, dv, dbias, saved, ws, stream) : hipSuccess;
}

}  // namespace ntm
