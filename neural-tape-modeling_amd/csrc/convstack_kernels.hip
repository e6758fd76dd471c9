// The conv stack of the reference's time-domain critic (DilatedConvDisc, code/critics.py:262-331) and of any stack like it: n
// weight-normed Conv1d(c_in, c_out, k, groups, dilation) layers, stride 1, no padding, LeakyReLU(slope) after every layer but the
// last.  What it shares with the spectral and the MelGAN family (the plan, weight preparation, weight-norm adjoint) is
// convstack_common.h; this file holds its GEMM kernels: a dilation per layer (up to 2^20, so no slab of tile + (K - 1) d frames
// can sit in LDS) and with it the PER-TAP fetch form of the conv kernel, the two-level weight gradient, and the chunk rule.
//
// cs_conv_kernel      the implicit GEMM along the frames: out[b][m][f] = sum_{c,j} W[j][c][m] in[b][c][f + j d + off], one workgroup
//                     per (stream, group, tile of output channels, tile of frames).  One step = (slab of 16 input channels, 4
//                     taps): the LDS operand is PER-TAP WINDOWS, 4 taps x 16 channels x tile frames, tap j's window starting at
//                     frame n0 + off + j d -- one form for every dilation (at d >= tile the windows do not overlap and nothing is
//                     read twice; at small d the overlap is read again from L2, up to K times the slab form's traffic, against
//                     64 MFMAs per wave and step).  A wave's MFMA takes 4 consecutive input channels of one tap as its K = 4.
//                       forward        off = 0,  W = wF (TapMajorLayout)
//                       data gradient  the same sum with the roles of the channels swapped: in = gz (the gradient at the layer's
//                                      pre-activation), off = -(K-1) d with zeros outside, W = wB
//                     Epilogues: forward, bias -> LeakyReLU(slope) (the last layer: bias).  Data gradient: times the LeakyReLU
//                     slope of the layer below, recovered from the sign of its saved output (y > 0 <=> pre > 0 as slope > 0;
//                     y == 0 takes the slope, torch's choice), so every stored gz is already a pre-activation gradient.
//                     Order of addition of one output: per slab of 16 input channels a sum from 0, taps ascending and per tap
//                     the channels in fours (one MFMA each, its K = 4 an fmaf chain); the slab sums are then added in ascending
//                     order -- a function of the layer alone, so a stream's result does not depend on its batch.  The loads of
//                     the next step are in flight during the MFMAs of the current one; every tile load is unconditional (from
//                     element 0 where the tile runs over an edge, the value chosen afterwards), because a branch per load
//                     cost more issue cycles than the step's MFMAs.
//                     The first layer (c_in = 1: one real row of the MFMA's four) and the last (c_out = 1: the 16 x 128 tile, one
//                     real row of 16) run on this same code with predicated edges: together they are under 3 % of the stack's
//                     flop even at 1/16 use of the pipe, and a second kernel would be a second order of addition to pin.
// cs_wgrad_kernel     dW[co][ci][k] = sum_{b,f} gz[b][co][f] in[b][ci][f + k d]: GEMM with M = co, N = (ci, k) flattened as dW is
//                     stored, reduction over the frames (64 per step, the MFMA's K = 4 consecutive frames).  The LDS operand is
//                     per-column windows: column (ci, k) holds in[b][ci][f0 + k d .. + 63].  Chunk rule: the streams into at most
//                     32 contiguous chunks (as the spectral family), the output frames of a layer into segments of kCsSegFrames =
//                     1024.  A workgroup walks the streams of its chunk in order and the frames of its segment in order, adding
//                     4 steps (256 frames) from 0 and then that sum to its total, and stores ONE partial tile, no atomics.  The
//                     workgroups of the first N tile also add up the rows of gz (the bias gradient), 64 frames from 0 at a time.
//
// Two tile shapes per GEMM kernel: 64 output channels x 64 columns (2 x 2 waves of 32 x 32) where a group has more than 16
// output channels, else 16 x 128 (16 x 64 for the weight gradient), four waves side by side.  Every valid layer runs on them:
// edges are predicated, there is no second code path.
#include "convstack_common.h"

namespace ntm {

constexpr int kCsMaxChunks = 32;      // stream chunks of the weight gradient
constexpr int kCsSegFrames = 1024;    // output frames per segment of the weight gradient (include/ntm.h documents both)

void convstack_plan(StackPlan &p, int64_t B, int64_t C0, int64_t F0, int n, const ntm_conv1d_layer_d *L)
{
    stack_plan_layers(p, B, F0, n, L, true, [&](int l, int64_t F) { return F - (int64_t)(L[l].k - 1) * L[l].dilation; });
    for (int l = 0; l < n; ++l) {
        p.dil[l] = L[l].dilation;
        stack_stream_chunks(B, kCsMaxChunks, p.nchunk[l], p.per[l]);
        p.seg[l] = kCsSegFrames, p.nseg[l] = stack_cdiv(p.F[l + 1], kCsSegFrames);
    }
    stack_plan_partials(p);
}

namespace {

enum { EPI_BIAS_LRELU = 0, EPI_BIAS = 1, EPI_MASK = 2, EPI_NONE = 3 };

struct ConvArgs {
    const float *in;    // [B][Cin][Fin]
    const float *w;     // [K][cin_g][Cout]
    const float *bias;  // EPI_BIAS*: [Cout]
    const float *aux;   // EPI_MASK: the saved output this gradient belongs to, in out's layout
    float *out;         // [B][Cout][Fout]
    int Cin, Cout, cin_g, cout_g, K, dil, Fin, Fout, epi, mtiles, ntiles;
    int64_t off;        // frame of `in` under output frame 0 at tap 0: 0 forward, -(K - 1) d for the data gradient
    float slope;
};

constexpr int kCI = 16;   // input channels per LDS slab
constexpr int kKT = 4;    // taps per step

// LDS pitches are 16 mod 64 floats: the four K-lanes groups of an MFMA operand read (16 consecutive floats of four
// consecutive rows) then fall on 64 different banks
__host__ __device__ constexpr int pitch_of(int T) { return T == 16 ? 16 : T + 16; }

template <int WM, int RM, int WN, int RN>
__global__ __launch_bounds__(256) void cs_conv_kernel(ConvArgs a)
{
    constexpr int TM = WM * RM * 16, TN = WN * RN * 16, PA = pitch_of(TM), PX = pitch_of(TN);
    extern __shared__ float lds[];
    float *As = lds, *Xs = lds + kKT * kCI * PA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM, li = lane & 15, kq = lane >> 4;
    const int64_t b = blockIdx.x / a.ntiles;
    const int n0 = (int)(blockIdx.x % a.ntiles) * TN;
    const int grp = blockIdx.y / a.mtiles, m0 = (blockIdx.y % a.mtiles) * TM;
    const int K = a.K;
    const float *inb = a.in + (b * a.Cin + (int64_t)grp * a.cin_g) * a.Fin;

    // acc: the sum over the current slab of 16 input channels (all taps), tot: the slabs added up -- a two-level sum
    f32x4 acc[RM][RN], tot[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) acc[i][j] = tot[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // one step = (slab of 16 input channels, 4 taps).  The global loads of step it + 1 are issued into registers before the MFMAs
    // of step it and stored to LDS after them, so their latency hides behind the matrix pipe (the order of addition is the loop's).
    // A thread keeps its column (m or t) and walks the rows: 256 / T rows per pass, 16 / that passes per tap.  Every load is
    // unconditional, from element 0 where the tile runs over an edge, and the value is chosen afterwards: no branch per load
    constexpr int RPA = 256 / TM, NPA = kCI / RPA, RPX = 256 / TN, NPX = kCI / RPX;
    const int am = tid % TM, ar = tid / TM, xt = tid % TN, xr = tid / TN;
    const int nk = (K + kKT - 1) / kKT, nit = ((a.cin_g + kCI - 1) / kCI) * nk;
    const bool am_ok = m0 + am < a.cout_g;
    const int a_col = grp * a.cout_g + m0 + am;
    const int64_t fr0 = (int64_t)n0 + xt + a.off;
    float ra[kKT * NPA], rx[kKT * NPX];
    auto fetch = [&](int it) {
        const int c0 = (it / nk) * kCI, k0 = (it % nk) * kKT;
#pragma unroll
        for (int kt = 0; kt < kKT; ++kt) {
            const bool k_ok = k0 + kt < K;
            const int64_t fr = fr0 + (int64_t)(k0 + kt) * a.dil;
            const bool f_ok = k_ok && fr >= 0 && fr < a.Fin;
            const int fri = f_ok ? (int)fr : 0;
#pragma unroll
            for (int ps = 0; ps < NPA; ++ps) {
                const int cl = ar + ps * RPA;
                const bool ok = k_ok && am_ok && c0 + cl < a.cin_g;
                const float val = a.w[ok ? ((k0 + kt) * a.cin_g + c0 + cl) * a.Cout + a_col : 0];
                ra[kt * NPA + ps] = ok ? val : 0.0f;
            }
#pragma unroll
            for (int ps = 0; ps < NPX; ++ps) {
                const int cl = xr + ps * RPX;
                const bool ok = f_ok && c0 + cl < a.cin_g;
                const float val = inb[ok ? (c0 + cl) * a.Fin + fri : 0];     // within one stream: below 2^31
                rx[kt * NPX + ps] = ok ? val : 0.0f;
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int kt = 0; kt < kKT; ++kt) {
#pragma unroll
            for (int ps = 0; ps < NPA; ++ps) As[(kt * kCI + ar + ps * RPA) * PA + am] = ra[kt * NPA + ps];
#pragma unroll
            for (int ps = 0; ps < NPX; ++ps) Xs[(kt * kCI + xr + ps * RPX) * PX + xt] = rx[kt * NPX + ps];
        }
    };
    fetch(0);
    for (int it = 0; it < nit; ++it) {
        __syncthreads();
        stash();
        __syncthreads();
        if (it + 1 < nit) fetch(it + 1);
        const int c0 = (it / nk) * kCI, k0 = (it % nk) * kKT;
        const int cn = min(4, (a.cin_g - c0 + 3) >> 2);     // groups of 4 channels this slab holds
        const int kn = min(kKT, K - k0);
        auto mma = [&](int kt, int c4) {
            const int row = kt * kCI + c4 * 4 + kq;
            float av[RM], bv[RN];
#pragma unroll
            for (int i = 0; i < RM; ++i) av[i] = As[row * PA + (wm * RM + i) * 16 + li];
#pragma unroll
            for (int j = 0; j < RN; ++j) bv[j] = Xs[row * PX + (wn * RN + j) * 16 + li];
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        };
        if (kn == kKT && cn == 4) {                         // a full step, unrolled: the LDS reads run ahead of the MFMAs
#pragma unroll
            for (int kt = 0; kt < kKT; ++kt)
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) mma(kt, c4);
        } else {                                            // an edge step: the same products in the same order
            for (int kt = 0; kt < kn; ++kt)
                for (int c4 = 0; c4 < cn; ++c4) mma(kt, c4);
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
                        v = v > 0.0f ? v : v * a.slope;
                    } else if (a.epi == EPI_BIAS) {
                        v += a.bias[co];
                    } else if (a.epi == EPI_MASK) {
                        v = a.aux[idx] > 0.0f ? v : v * a.slope;
                    }
                    a.out[idx] = v;
                }
            }
        }
}

struct WgradArgs {
    const float *gz;   // [B][Cout][Fout]
    const float *in;   // [B][Cin][Fin], Fin = Fout + (K - 1) d
    float *part;       // [stream chunk][segment][Cout][cin_g * K]
    float *bpart;      // [stream chunk][segment][Cout]
    int Cin, Cout, cin_g, cout_g, K, dil, Fin, Fout, mtiles, per;
    int64_t B, nseg;
};

constexpr int kTF = 64;   // frames per reduction step
constexpr int kPG = 68;   // pitch of both tiles: 4 mod 64, so (16 rows) x (4 consecutive frames) fall on 64 different banks
constexpr int kSub = 4;   // steps added from 0 before they join the total (256 frames)

template <int WM, int RM, int WN, int RN>
__global__ __launch_bounds__(256) void cs_wgrad_kernel(WgradArgs a)
{
    constexpr int TM = WM * RM * 16, TN = WN * RN * 16;
    static_assert(TN == 64, "the X tile is 64 columns x 64 frames");
    extern __shared__ float lds[];
    float *Gs = lds, *Xs = lds + TM * kPG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM, li = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.z * TN, grp = blockIdx.y / a.mtiles, m0 = (blockIdx.y % a.mtiles) * TM;
    const int K = a.K, n = a.cin_g * K;
    const int64_t part_i = blockIdx.x, chunk = part_i / a.nseg, seg = part_i - chunk * a.nseg;
    const int fs0 = (int)(seg * kCsSegFrames), fs1 = (int)min((int64_t)a.Fout, (seg + 1) * kCsSegFrames);

    f32x4 acc[RM][RN], tot[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) acc[i][j] = tot[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float bsum = 0.0f;

    // a thread keeps its frame t = tid % 64 and walks the rows of both tiles, 4 per pass: row tid / 64 + 4 q.  Every load is
    // unconditional, from element 0 where the tile runs over an edge, and the value is chosen afterwards: no branch per load
    constexpr int GR = TM * kTF / 256, XR = TN * kTF / 256;
    const int lt = tid % kTF, lr = tid / kTF;
    int xoff[XR];           // ci * Fin + k d of the column (within one stream: below 2^31), -1: no such column
#pragma unroll
    for (int q = 0; q < XR; ++q) {
        const int j = j0 + lr + q * 4, ci = j / K;
        xoff[q] = j < n ? ci * a.Fin + (j - ci * K) * a.dil : -1;
    }

    // one step = 64 frames of one stream of the chunk; the loads of the next step are in flight during the MFMAs of this one
    const int64_t b_begin = chunk * a.per, b_end = min((chunk + 1) * a.per, a.B);
    const int nf = (fs1 - fs0 + kTF - 1) / kTF, nit = (int)(b_end - b_begin) * nf;
    float rg[GR], rx[XR];
    auto fetch = [&](int it) {
        const int64_t b = b_begin + it / nf;
        const int f = fs0 + (it % nf) * kTF + lt;
        const bool f_ok = f < fs1;
        const float *gb = a.gz + (b * a.Cout + (int64_t)grp * a.cout_g + m0) * a.Fout;
        const float *xb = a.in + (b * a.Cin + (int64_t)grp * a.cin_g) * a.Fin;
#pragma unroll
        for (int q = 0; q < GR; ++q) {
            const int m = lr + q * 4;
            const bool ok = f_ok && m0 + m < a.cout_g;
            const float val = gb[ok ? m * a.Fout + f : 0];
            rg[q] = ok ? val : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < XR; ++q) {
            const bool ok = f_ok && xoff[q] >= 0;
            const float val = xb[ok ? xoff[q] + f : 0];
            rx[q] = ok ? val : 0.0f;
        }
    };
    fetch(0);
    for (int it = 0; it < nit; ++it) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < GR; ++q) Gs[(lr + q * 4) * kPG + lt] = rg[q];
#pragma unroll
        for (int q = 0; q < XR; ++q) Xs[(lr + q * 4) * kPG + lt] = rx[q];
        __syncthreads();
        if (it + 1 < nit) fetch(it + 1);
        if (blockIdx.z == 0 && tid < TM) {
            float s = 0.0f;
            for (int t = 0; t < kTF; ++t) s += Gs[tid * kPG + t];
            bsum += s;
        }
        for (int f4 = 0; f4 < kTF; f4 += 4) {
            float av[RM], bv[RN];
#pragma unroll
            for (int i = 0; i < RM; ++i) av[i] = Gs[((wm * RM + i) * 16 + li) * kPG + f4 + kq];
#pragma unroll
            for (int j = 0; j < RN; ++j) bv[j] = Xs[((wn * RN + j) * 16 + li) * kPG + f4 + kq];
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if ((it + 1) % kSub == 0 || it + 1 == nit) {
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
        for (int jj = 0; jj < RN; ++jj) {
            const int j = j0 + (wn * RN + jj) * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wm * RM + i) * 16 + kq * 4 + r;
                if (m < a.cout_g && j < n)
                    a.part[(part_i * a.Cout + grp * a.cout_g + m) * n + j] = tot[i][jj][r];
            }
        }
    if (blockIdx.z == 0 && tid < TM && m0 + tid < a.cout_g)
        a.bpart[part_i * a.Cout + grp * a.cout_g + m0 + tid] = bsum;
}

hipError_t launch_conv(ConvArgs a, int64_t B, int groups, hipStream_t stream)
{
    const bool narrow = a.cout_g <= 16;
    const int TM = narrow ? 16 : 64, TN = narrow ? 128 : 64;
    a.mtiles = (a.cout_g + TM - 1) / TM;
    a.ntiles = (a.Fout + TN - 1) / TN;
    const size_t lds = (size_t)(kKT * kCI * (pitch_of(TM) + pitch_of(TN))) * sizeof(float);
    const dim3 grid((unsigned)(B * a.ntiles), (unsigned)(groups * a.mtiles));
    if (narrow)
        hipLaunchKernelGGL((cs_conv_kernel<1, 1, 4, 2>), grid, dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL((cs_conv_kernel<2, 2, 2, 2>), grid, dim3(256), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_wgrad(WgradArgs a, int groups, int nchunk, hipStream_t stream)
{
    const bool narrow = a.cout_g <= 16;
    const int TM = narrow ? 16 : 64;
    a.mtiles = (a.cout_g + TM - 1) / TM;
    const size_t lds = (size_t)((TM + 64) * kPG) * sizeof(float);
    const dim3 grid((unsigned)(nchunk * a.nseg), (unsigned)(groups * a.mtiles), (unsigned)((a.cin_g * a.K + 63) / 64));
    if (narrow)
        hipLaunchKernelGGL((cs_wgrad_kernel<1, 1, 4, 1>), grid, dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL((cs_wgrad_kernel<2, 2, 2, 2>), grid, dim3(256), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_convstack_forward(const StackPlan &p, const float *x, int64_t B, float slope, const float *const *g,
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
        a.K = p.k[l], a.dil = p.dil[l], a.Fin = (int)p.F[l], a.Fout = (int)p.F[l + 1], a.off = 0;
        a.slope = slope;
        a.epi = last ? EPI_BIAS : EPI_BIAS_LRELU;
        if (hipError_t e = launch_conv(a, B, p.groups[l], stream)) return e;
    }
    return hipSuccess;
}

hipError_t launch_convstack_backward(const StackPlan &p, const float *x, int64_t B, float slope, const float *const *g,
                                     const float *const *v, const float *saved, const float *gout, float *gx, float *const *dg,
                                     float *const *dv, float *const *dbias, float *ws, hipStream_t stream)
{
    const float *gz = gout;
    for (int l = p.n - 1; l >= 0; --l) {
        const int cin_g = p.c_in[l] / p.groups[l], cout_g = p.c_out[l] / p.groups[l];
        const float *in = l ? saved + p.act_off[l - 1] : x;
        if (dg) {
            WgradArgs a{};
            a.gz = gz, a.in = in, a.part = ws + p.part_off[l], a.bpart = ws + p.bpart_off[l];
            a.Cin = p.c_in[l], a.Cout = p.c_out[l], a.cin_g = cin_g, a.cout_g = cout_g, a.K = p.k[l], a.dil = p.dil[l];
            a.Fin = (int)p.F[l], a.Fout = (int)p.F[l + 1], a.per = p.per[l], a.B = B, a.nseg = p.nseg[l];
            if (hipError_t e = launch_wgrad(a, p.groups[l], p.nchunk[l], stream)) return e;
        }
        if (l == 0 && !gx) break;
        float *dst = l ? ws + ((p.n - 1 - l) & 1) * p.gz_size : gx;
        ConvArgs a{};
        a.in = gz, a.w = saved + p.w_total + p.w_off[l], a.out = dst;
        a.aux = l ? saved + p.act_off[l - 1] : nullptr;
        a.Cin = p.c_out[l], a.Cout = p.c_in[l], a.cin_g = cout_g, a.cout_g = cin_g;
        a.K = p.k[l], a.dil = p.dil[l], a.Fin = (int)p.F[l + 1], a.Fout = (int)p.F[l];
        a.off = -(int64_t)(p.k[l] - 1) * p.dil[l];
        a.slope = slope;
        a.epi = l ? EPI_MASK : EPI_NONE;
        if (hipError_t e = launch_conv(a, B, p.groups[l], stream)) return e;
        gz = dst;
    }
    return dg ? launch_stack_wnorm(p, p.n, g, v, dg, dv, dbias, saved, ws, stream) : hipSuccess;
}

}  // namespace ntm
