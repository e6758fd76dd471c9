// The conv stack of the reference's MelGAN critic (MelGCrit / NLayerDiscriminator, code/critics.py:18-122) and of any stack like
// it: n weight-normed Conv1d(c_in, c_out, k, groups, stride, pad) layers, dilation 1, LeakyReLU(slope) after every layer but the
// last, zero padding, or a reflection pad on the first layer.  What it shares with the spectral and the dilated family (the plan,
// weight preparation, weight-norm adjoint) is convstack_common.h; this file holds its GEMM kernels and what differs:
// a stride and a pad per layer instead of a dilation, the reflected first layer, the output of EVERY layer a tensor of the caller's
// (they are the saved activations: there is no second copy), a gradient that may arrive at every one of them -- and with them the
// PER-INDEX fetch form of the conv kernel, the weight layouts it reads, the dot, mask and fold kernels and the chunk rule.
//
// PhaseLayout         both weight layouts are [reduction index][every channel of the other side], so a step's weights are 64
//                     consecutive rows:
//                       wF[ci K + k][CO]            (ci within the group, CO every output channel)   -- forward
//                       wB[phase][co Kph + i][CI]   (co within the group, CI every input channel; tap k = phase + stride i, the
//                                                   phases one after the other, Kph taps each)         -- data gradient
// sc_conv_kernel      the implicit GEMM along the frames, one workgroup per (stream, phase, group, tile of output channels, tile of
//                     columns).  The reduction index is r = c K + i (input channel of the group major, tap minor) and one step
//                     takes 64 of them, whatever c_in/groups and k are: the LDS operand is 64 per-index windows of tile columns
//                     (row q: input channel c at tap i).  The grouped layers' 4 channels x 41 taps are 3 steps (a slab of 16
//                     channels x 4 taps per step, as cs_conv_kernel cuts it, would be 11 steps a quarter full), the dense layer's
//                     k = 5 wastes no tap.
//                       forward        column n = output frame, tap i = weight tap, window frame n s + i - pad: a read strided
//                                      by s (the lanes of a load s floats apart; the s - 1 floats between them are the next taps'
//                                      and come from the same lines).  Frames outside read 0, or on a reflected layer the
//                                      mirrored sample.  The epilogue stores into the layer's output tensor.
//                       data gradient  PER PHASE, the exact work: the input frames t with (t + pad) mod s = r take the taps
//                                      j = r + s i only, gin[c][s u + r - pad] = sum_{m,i} w[m][c][r + s i] gz[m][u - i] -- a
//                                      stride-1 correlation over u per phase, the windows contiguous; the s phases are s
//                                      workgroups, the store is strided by s.  A phase with no tap (k < s) stores the epilogue
//                                      of 0.  The epilogue adds the caller's gradient at that tensor where there is one.  Under a
//                                      reflected first layer the kernel writes the gradient of the PADDED input (F0 + 2 pad
//                                      frames) and sc_fold_kernel adds the border terms back: gx[t] = P[t] + P[-t] (1 <= t <=
//                                      pad) + P[2 (F0 - 1) - t] (F0 - 1 - pad <= t <= F0 - 2), in that order.
//                     Epilogues: forward, bias -> LeakyReLU(slope) (the last layer: bias).  Data gradient: + the caller's
//                     gradient at that tensor where there is one, then times the LeakyReLU slope of the layer below, recovered
//                     from the sign of its saved output (y > 0 <=> pre > 0 as slope > 0; y == 0 takes the slope, torch's choice).
//                     Order of addition of one output: the reduction indices ascending in fours (one MFMA each, its K = 4 an
//                     fmaf chain, for the data gradient over the taps of its phase), 4 steps (256 indices) from 0, and those sums
//                     added in ascending order -- a function of the layer alone.
// sc_wgrad_kernel     cs_wgrad_kernel with the X window at frame f s + k - pad, zero or mirrored outside, cut by the chunk rule of
//                     include/ntm.h (sconv_plan): per layer, stream chunks x frame segments of `seg` frames.
// sc_dot_kernel       the same sum and epilogue for a layer with one output channel per group and >= 128 reduction indices per
//                     phase (the last layer, 1024 x 3 -> 1; the first layer's data gradient): 64 columns of one channel per
//                     workgroup, the reduction in four contiguous quarters (one per wave, an fmaf chain from 0 each) added
//                     in order.  Which kernel a layer runs on is a function of the layer alone.
// sc_mask_kernel      gz = gout * LeakyReLU'(y) for the highest layer a gradient arrives at when it is not the last.
// weight-norm adjoint stack_wnorm_kernel over the layers a gradient reaches; layers above them get zeros from a memset.
//
// Two tile shapes per GEMM kernel, as in convstack_kernels.hip: 64 x 64 where a group has more than 16 rows, else 16 x 128
// (16 x 64 for the weight gradient) with predicated edges -- the grouped layers' 4-channel groups (four real rows of sixteen) run
// on the narrow tile.
#include "convstack_common.h"

namespace ntm {

constexpr int kScMaxChunks = 32;                 // at most this many stream chunks ...
constexpr int64_t kScSegFrames = 1024;           // ... times segments of this many output frames (doubled while ...)
constexpr int64_t kScMinFrames = 2048;           // a partial sums at least this many frames (where the layer has them)
constexpr int64_t kScCapFloats = (int64_t)1 << 24;   // ... and the partials of one layer stay within 2^24 floats (64 MiB)

void sconv_plan(StackPlan &p, int64_t B, int64_t C0, int64_t F0, int n, const ntm_conv1d_layer_s *L)
{
    stack_plan_layers(p, B, F0, n, L, false, [&](int l, int64_t F) { return (F + 2 * (int64_t)L[l].pad - L[l].k) / L[l].stride + 1; });
    for (int l = 0; l < n; ++l) {
        p.stride[l] = L[l].stride, p.pad[l] = L[l].pad, p.reflect[l] = L[l].pad_mode == 1 && L[l].pad > 0;
        const int64_t W = p.w_size(l), Fo = p.F[l + 1];
        int64_t seg = kScSegFrames;
        while (stack_cdiv(Fo, seg) > 1 && stack_cdiv(Fo, seg) * W > kScCapFloats) seg *= 2;
        const int64_t nseg = stack_cdiv(Fo, seg);
        int64_t per = 1, nchunk = 0;
        if (B > 0) {
            per = stack_cdiv(B, kScMaxChunks);
            const int64_t need = stack_cdiv(kScMinFrames, Fo < seg ? Fo : seg);
            if (need > per) per = need;
            int64_t maxparts = kScCapFloats / (nseg * W);
            if (maxparts < 1) maxparts = 1;
            if (stack_cdiv(B, maxparts) > per) per = stack_cdiv(B, maxparts);
            if (per > B) per = B;
            nchunk = stack_cdiv(B, per);
        }
        p.seg[l] = seg, p.nseg[l] = nseg, p.per[l] = (int)per, p.nchunk[l] = (int)nchunk;
    }
    p.fold_size = p.reflect[0] ? B * C0 * (F0 + 2 * (int64_t)p.pad[0]) : 0;
    stack_plan_partials(p);
}

namespace {

struct PhaseLayout {
    static __device__ __forceinline__ void put(const PrepRow &r, float *wF, float *wB, int j, int ci, int k, float w)
    {
        wF[(int64_t)j * r.c_out + r.co] = w;
        // tap k is tap i = k / stride of phase ph = k mod stride, which has Kph taps; the phases before it hold `before`
        const int kq = r.K / r.stride, krem = r.K % r.stride;
        const int ph = k % r.stride, i = k / r.stride, Kph = kq + (ph < krem), before = ph * kq + min(ph, krem);
        wB[((int64_t)before * r.cout_g + r.co_l * Kph + i) * r.c_in + r.grp * r.cin_g + ci] = w;
    }
};

enum { EPI_BIAS_LRELU = 0, EPI_BIAS = 1, EPI_MASK = 2, EPI_NONE = 3 };

struct ConvArgs {
    const float *in;    // [B][Cin][Fin]
    const float *w;     // forward [cin_g Ktot][Cout]; data gradient [phase][cin_g Kph][Cout]
    const float *bias;  // EPI_BIAS*: [Cout]
    const float *aux;   // EPI_MASK: the saved output this gradient belongs to, in out's layout
    const float *add;   // EPI_MASK: the caller's gradient at that output, or null
    float *out;         // [B][Cout][Fout]
    int Cin, Cout, cin_g, cout_g, Ktot, Fin, Fout, epi, mtiles, ntiles;
    int nphase;         // forward 1; data gradient: the stride
    int sx, dt;         // window frame of (column n, tap i of the phase) = n sx + i dt + off
    int off, reflect;   // forward: sx = stride, dt = 1, off = -pad; data gradient: sx = 1, dt = -1, off = 0
    int os, oo;         // output frame of column n in phase r = n os + r + oo  (forward 1, 0; data gradient stride, -pad)
    int ncols;          // columns per phase
    float slope;
};

constexpr int kRows = 64;   // reduction indices per step
constexpr int kJoin = 4;    // steps added from 0 before they join the total (256 reduction indices)
constexpr int kDotMin = 128; // a layer with one output channel per group and this many reduction indices runs on sc_dot_kernel

// LDS pitches are 16 mod 64 floats: the four K-lanes groups of an MFMA operand read (16 consecutive floats of four
// consecutive rows) then fall on 64 different banks
__host__ __device__ constexpr int pitch_of(int T) { return T == 16 ? 16 : T + 16; }

template <int WM, int RM, int WN, int RN>
__global__ __launch_bounds__(256) void sc_conv_kernel(ConvArgs a)
{
    constexpr int TM = WM * RM * 16, TN = WN * RN * 16, PA = pitch_of(TM), PX = pitch_of(TN);
    extern __shared__ float lds[];
    float *As = lds, *Xs = lds + kRows * PA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM, li = lane & 15, kq = lane >> 4;
    const int per_b = a.nphase * a.ntiles;
    const int64_t b = blockIdx.x / per_b;
    const int rem = (int)(blockIdx.x % per_b), ph = rem / a.ntiles;
    const int n0 = (rem % a.ntiles) * TN;
    const int grp = blockIdx.y / a.mtiles, m0 = (blockIdx.y % a.mtiles) * TM;
    // the taps of this phase: weight tap ph + i nphase, i in [0, K); the phases before it hold `before` taps
    const int tq = a.Ktot / a.nphase, trem = a.Ktot % a.nphase;
    const int K = tq + (ph < trem), before = ph * tq + min(ph, trem);
    // the reduction runs over r = c K + i (input channel of the group major, tap minor), r in [0, R).  c = r / K in float:
    // (r + 1/2) / K is at least 1 / (2 K) >= 2^-7 from an integer and the product's rounding error below 2^10 2^-23
    const int R = a.cin_g * K;
    const float invK = K > 0 ? 1.0f / (float)K : 0.0f;
    const float *wph = a.w + (int64_t)before * a.cin_g * a.Cout;
    const float *inb = a.in + (b * a.Cin + (int64_t)grp * a.cin_g) * a.Fin;

    // acc: the sum over up to kJoin steps, tot: those sums added up -- a two-level sum
    f32x4 acc[RM][RN], tot[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) acc[i][j] = tot[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // one step = 64 reduction indices: row q of the two LDS tiles holds the weights w[.][c][tap] of index r0 + q and the window
    // of input channel c at that tap.  The global loads of step it + 1 are issued into registers before the MFMAs of step it and
    // stored to LDS after them.  A thread keeps its column (m or n) and walks the rows.  Every load is unconditional, from element
    // 0 where the tile runs over an edge, and the value is chosen afterwards: no branch per load
    constexpr int RPA = 256 / TM, NPA = kRows / RPA, RPX = 256 / TN, NPX = kRows / RPX;
    const int am = tid % TM, ar = tid / TM, xt = tid % TN, xr = tid / TN;
    const int nit = (R + kRows - 1) / kRows;
    const bool am_ok = m0 + am < a.cout_g;
    const int a_col = grp * a.cout_g + m0 + am;
    const bool col_ok = n0 + xt < a.ncols;
    const int64_t fr0 = (int64_t)(n0 + xt) * a.sx + a.off;
    const int fr0i = col_ok ? (int)fr0 : 0;                     // a real column's window starts within the stream: an int
    float ra[NPA], rx[NPX];
    auto fetch = [&](int it) {
        const int r0 = it * kRows;
        const int abase = (r0 + ar) * a.Cout + a_col;           // below 2^26
#pragma unroll
        for (int q = 0; q < NPA; ++q) {
            const bool ok = r0 + ar + q * RPA < R && am_ok;
            const float val = wph[ok ? abase + q * RPA * a.Cout : 0];
            ra[q] = ok ? val : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < NPX; ++q) {
            const int r = r0 + xr + q * RPX;                    // r < 2^16 + 64, c < 2^10, K <= 64: 24-bit products
            const int c = (int)(((float)r + 0.5f) * invK), i = r - __mul24(c, K);
            int fr = fr0i + __mul24(i, a.dt);
            if (a.reflect) fr = fr < 0 ? -fr : (fr >= a.Fin ? 2 * (a.Fin - 1) - fr : fr);
            const bool ok = r < R && col_ok && fr >= 0 && fr < a.Fin;
            const float val = inb[ok ? c * a.Fin + fr : 0];     // within one stream: below 2^31
            rx[q] = ok ? val : 0.0f;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < NPA; ++q) As[(ar + q * RPA) * PA + am] = ra[q];
#pragma unroll
        for (int q = 0; q < NPX; ++q) Xs[(xr + q * RPX) * PX + xt] = rx[q];
    };
    if (nit > 0) fetch(0);
    for (int it = 0; it < nit; ++it) {
        __syncthreads();
        stash();
        __syncthreads();
        if (it + 1 < nit) fetch(it + 1);
        const int n4 = min(kRows / 4, (R - it * kRows + 3) >> 2);   // groups of 4 reduction indices this step holds
        auto mma = [&](int r4) {
            const int row = r4 * 4 + kq;
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
        if (n4 == kRows / 4) {                              // a full step, unrolled: the LDS reads run ahead of the MFMAs
#pragma unroll
            for (int r4 = 0; r4 < kRows / 4; ++r4) mma(r4);
        } else {                                            // an edge step: the same products in the same order
            for (int r4 = 0; r4 < n4; ++r4) mma(r4);
        }
        if ((it + 1) % kJoin == 0 || it + 1 == nit) {
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
            const int col = n0 + (wn * RN + j) * 16 + li;
            const int64_t f = (int64_t)col * a.os + ph + a.oo;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wm * RM + i) * 16 + kq * 4 + r;
                if (m < a.cout_g && col < a.ncols && f >= 0 && f < a.Fout) {
                    const int co = grp * a.cout_g + m;
                    const int64_t idx = (b * a.Cout + co) * a.Fout + f;
                    float v = tot[i][j][r];
                    if (a.epi == EPI_BIAS_LRELU) {
                        v += a.bias[co];
                        v = v > 0.0f ? v : v * a.slope;
                    } else if (a.epi == EPI_BIAS) {
                        v += a.bias[co];
                    } else if (a.epi == EPI_MASK) {
                        if (a.add) v += a.add[idx];
                        v = a.aux[idx] > 0.0f ? v : v * a.slope;
                    }
                    a.out[idx] = v;
                }
            }
        }
}

// The same sum for a layer with ONE output channel per group and a long reduction (the critic's last layer, 1024 x 3 -> 1): a
// 16-row MFMA tile would hold one real row and a workgroup would walk the whole reduction alone, a step at a time.  Here a
// workgroup takes 64 columns of one output channel, its four waves a quarter of the reduction indices each (contiguous, ascending,
// one fmaf chain per column from 0), and the quarters are added in order: ((q0 + q1) + q2) + q3.  ConvArgs and the epilogue are
// sc_conv_kernel's; which of the two a layer runs on is a function of the layer alone (launch_conv).
__global__ __launch_bounds__(256) void sc_dot_kernel(ConvArgs a)
{
    __shared__ float red[4][64];
    const int tid = threadIdx.x, lane = tid & 63, slice = tid >> 6;
    const int per_b = a.nphase * a.ntiles;
    const int64_t b = blockIdx.x / per_b;
    const int rem = (int)(blockIdx.x % per_b), ph = rem / a.ntiles;
    const int col = (rem % a.ntiles) * 64 + lane;
    const int co = blockIdx.y;                                   // cout_g == 1: the group is the output channel
    const int kq = a.Ktot / a.nphase, krem = a.Ktot % a.nphase;
    const int K = kq + (ph < krem), before = ph * kq + min(ph, krem);
    const float *wph = a.w + (int64_t)before * a.cin_g * a.Cout;
    const int R = a.cin_g * K, rq = (R + 3) >> 2;
    const int r_begin = min(R, slice * rq), r_end = min(R, r_begin + rq);
    const float *inb = a.in + (b * a.Cin + (int64_t)co * a.cin_g) * a.Fin;
    const bool col_ok = col < a.ncols;
    const int64_t fr0 = (int64_t)col * a.sx + a.off;
    int c = K > 0 ? r_begin / K : 0, i = r_begin - c * K;
    float acc = 0.0f;
#pragma unroll 4
    for (int r = r_begin; r < r_end; ++r) {
        int64_t fr = fr0 + (int64_t)i * a.dt;
        if (a.reflect) fr = fr < 0 ? -fr : (fr >= a.Fin ? 2 * ((int64_t)a.Fin - 1) - fr : fr);
        const bool ok = col_ok && fr >= 0 && fr < a.Fin;
        const float x = inb[ok ? c * a.Fin + (int)fr : 0];
        const float w = wph[r * a.Cout + co];
        acc = fmaf(w, ok ? x : 0.0f, acc);
        if (++i == K) i = 0, ++c;
    }
    red[slice][lane] = acc;
    __syncthreads();
    if (slice != 0) return;
    float v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    const int64_t f = (int64_t)col * a.os + ph + a.oo;
    if (col_ok && f >= 0 && f < a.Fout) {
        const int64_t idx = (b * a.Cout + co) * a.Fout + f;
        if (a.epi == EPI_BIAS_LRELU) {
            v += a.bias[co];
            v = v > 0.0f ? v : v * a.slope;
        } else if (a.epi == EPI_BIAS) {
            v += a.bias[co];
        } else if (a.epi == EPI_MASK) {
            if (a.add) v += a.add[idx];
            v = a.aux[idx] > 0.0f ? v : v * a.slope;
        }
        a.out[idx] = v;
    }
}

// gz = gout * LeakyReLU'(y), elementwise
__global__ __launch_bounds__(256) void sc_mask_kernel(const float *gout, const float *y, float *gz, int64_t n, float slope)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) gz[i] = y[i] > 0.0f ? gout[i] : gout[i] * slope;
}

// the adjoint of ReflectionPad1d(pad): P [rows][F + 2 pad] -> gx [rows][F], the interior, then the left mirror, then the right
__global__ __launch_bounds__(256) void sc_fold_kernel(const float *P, float *gx, int64_t rows, int F, int pad)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * F) return;
    const int64_t row = i / F;
    const int t = (int)(i - row * F);
    const float *p = P + row * ((int64_t)F + 2 * pad) + pad;      // p[t'] for t' in [-pad, F + pad)
    float v = p[t];
    if (t >= 1 && t <= pad) v += p[-t];
    if (t >= F - 1 - pad && t <= F - 2) v += p[2 * (F - 1) - t];
    gx[i] = v;
}

struct WgradArgs {
    const float *gz;   // [B][Cout][Fout]
    const float *in;   // [B][Cin][Fin]
    float *part;       // [stream chunk][segment][Cout][cin_g * K]
    float *bpart;      // [stream chunk][segment][Cout]
    int Cin, Cout, cin_g, cout_g, K, stride, pad, reflect, Fin, Fout, mtiles, per;
    int64_t B, nseg, seg;
};

constexpr int kTF = 64;   // frames per reduction step
constexpr int kPG = 68;   // pitch of both tiles: 4 mod 64, so (16 rows) x (4 consecutive frames) fall on 64 different banks
constexpr int kSub = 4;   // steps added from 0 before they join the total (256 frames)

template <int WM, int RM, int WN, int RN>
__global__ __launch_bounds__(256) void sc_wgrad_kernel(WgradArgs a)
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
    const int fs0 = (int)(seg * a.seg), fs1 = (int)min((int64_t)a.Fout, (seg + 1) * a.seg);

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
    int xrow[XR], xk[XR];   // ci * Fin of the column (within one stream: below 2^31; -1: no such column) and its k - pad
#pragma unroll
    for (int q = 0; q < XR; ++q) {
        const int j = j0 + lr + q * 4, ci = j / K;
        xrow[q] = j < n ? ci * a.Fin : -1;
        xk[q] = j - ci * K - a.pad;
    }

    // one step = 64 frames of one stream of the chunk; the loads of the next step are in flight during the MFMAs of this one
    const int64_t b_begin = chunk * a.per, b_end = min((chunk + 1) * a.per, a.B);
    const int nf = (fs1 - fs0 + kTF - 1) / kTF, nit = (int)(b_end - b_begin) * nf;
    float rg[GR], rx[XR];
    auto fetch = [&](int it) {
        const int64_t b = b_begin + it / nf;
        const int f = fs0 + (it % nf) * kTF + lt;
        const bool f_ok = f < fs1;
        const int64_t fx = (int64_t)f * a.stride;
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
            int64_t fr = fx + xk[q];
            if (a.reflect) fr = fr < 0 ? -fr : (fr >= a.Fin ? 2 * ((int64_t)a.Fin - 1) - fr : fr);
            const bool ok = f_ok && xrow[q] >= 0 && fr >= 0 && fr < a.Fin;
            const float val = xb[ok ? xrow[q] + (int)fr : 0];
            rx[q] = ok ? val : 0.0f;
        }
    };
    if (nit > 0) fetch(0);
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
    // one output channel per group and at least kDotMin reduction indices per phase: the dot kernel
    if (a.cout_g == 1 && a.cin_g * ((a.Ktot + a.nphase - 1) / a.nphase) >= kDotMin) {
        a.mtiles = 1;
        a.ntiles = (a.ncols + 63) / 64;
        hipLaunchKernelGGL(sc_dot_kernel, dim3((unsigned)(B * a.nphase * a.ntiles), (unsigned)groups), dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    const bool narrow = a.cout_g <= 16;
    const int TM = narrow ? 16 : 64, TN = narrow ? 128 : 64;
    a.mtiles = (a.cout_g + TM - 1) / TM;
    a.ntiles = (a.ncols + TN - 1) / TN;
    const size_t lds = (size_t)(kRows * (pitch_of(TM) + pitch_of(TN))) * sizeof(float);
    const dim3 grid((unsigned)(B * a.nphase * a.ntiles), (unsigned)(groups * a.mtiles));
    if (narrow)
        hipLaunchKernelGGL((sc_conv_kernel<1, 1, 4, 2>), grid, dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL((sc_conv_kernel<2, 2, 2, 2>), grid, dim3(256), lds, stream, a);
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
        hipLaunchKernelGGL((sc_wgrad_kernel<1, 1, 4, 1>), grid, dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL((sc_wgrad_kernel<2, 2, 2, 2>), grid, dim3(256), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sconvstack_forward(const StackPlan &p, const float *x, int64_t B, float slope, const float *const *g,
                                     const float *const *v, const float *const *bias, float *saved, float *const *outs,
                                     hipStream_t stream)
{
    if (hipError_t e = launch_stack_prep<PhaseLayout>(p, g, v, saved, stream)) return e;
    for (int l = 0; l < p.n; ++l) {
        const bool last = l == p.n - 1;
        ConvArgs a{};
        a.in = l ? outs[l - 1] : x;
        a.w = saved + p.w_off[l];
        a.bias = bias[l];
        a.out = outs[l];
        a.Cin = p.c_in[l], a.Cout = p.c_out[l], a.cin_g = p.c_in[l] / p.groups[l], a.cout_g = p.c_out[l] / p.groups[l];
        a.Ktot = p.k[l], a.Fin = (int)p.F[l], a.Fout = (int)p.F[l + 1];
        a.nphase = 1, a.sx = p.stride[l], a.dt = 1, a.off = -p.pad[l], a.reflect = p.reflect[l];
        a.os = 1, a.oo = 0, a.ncols = a.Fout;
        a.slope = slope;
        a.epi = last ? EPI_BIAS : EPI_BIAS_LRELU;
        if (hipError_t e = launch_conv(a, B, p.groups[l], stream)) return e;
    }
    return hipSuccess;
}

hipError_t launch_sconvstack_backward(const StackPlan &p, const float *x, int64_t B, float slope, const float *const *g,
                                      const float *const *v, const float *saved, const float *const *outs,
                                      const float *const *gouts, float *gx, float *const *dg, float *const *dv,
                                      float *const *dbias, float *ws, hipStream_t stream)
{
    int top = p.n - 1;
    while (top > 0 && !gouts[top]) --top;       // the caller has checked that one entry is not null
    if (dg)
        for (int l = top + 1; l < p.n; ++l) {   // no gradient reaches these layers
            const int64_t W = (int64_t)p.c_out[l] * (p.c_in[l] / p.groups[l]) * p.k[l];
            if (hipError_t e = hipMemsetAsync(dg[l], 0, sizeof(float) * p.c_out[l], stream)) return e;
            if (hipError_t e = hipMemsetAsync(dv[l], 0, sizeof(float) * W, stream)) return e;
            if (hipError_t e = hipMemsetAsync(dbias[l], 0, sizeof(float) * p.c_out[l], stream)) return e;
        }
    int flip = 0;
    const float *gz = gouts[top];
    if (top != p.n - 1) {                       // the gradient arrives behind a LeakyReLU
        const int64_t sz = B * p.c_out[top] * p.F[top + 1];
        float *dst = ws + flip * p.gz_size;
        hipLaunchKernelGGL(sc_mask_kernel, dim3((unsigned)((sz + 255) / 256)), dim3(256), 0, stream, gz, outs[top], dst, sz, slope);
        if (hipError_t e = hipGetLastError()) return e;
        gz = dst, flip ^= 1;
    }
    for (int l = top; l >= 0; --l) {
        const int cin_g = p.c_in[l] / p.groups[l], cout_g = p.c_out[l] / p.groups[l];
        const float *in = l ? outs[l - 1] : x;
        if (dg) {
            WgradArgs a{};
            a.gz = gz, a.in = in, a.part = ws + p.part_off[l], a.bpart = ws + p.bpart_off[l];
            a.Cin = p.c_in[l], a.Cout = p.c_out[l], a.cin_g = cin_g, a.cout_g = cout_g, a.K = p.k[l];
            a.stride = p.stride[l], a.pad = p.pad[l], a.reflect = p.reflect[l];
            a.Fin = (int)p.F[l], a.Fout = (int)p.F[l + 1], a.per = p.per[l], a.B = B, a.nseg = p.nseg[l], a.seg = p.seg[l];
            if (hipError_t e = launch_wgrad(a, p.groups[l], p.nchunk[l], stream)) return e;
        }
        if (l == 0 && !gx) break;
        const bool fold = l == 0 && p.reflect[0];
        float *dst = l ? ws + flip * p.gz_size : (fold ? ws + 2 * p.gz_size : gx);
        flip ^= 1;
        ConvArgs a{};
        a.in = gz, a.w = saved + p.w_total + p.w_off[l], a.out = dst;
        a.aux = l ? outs[l - 1] : nullptr;
        a.add = l ? gouts[l - 1] : nullptr;
        a.Cin = p.c_out[l], a.Cout = p.c_in[l], a.cin_g = cout_g, a.cout_g = cin_g;
        a.Ktot = p.k[l], a.Fin = (int)p.F[l + 1];
        const int pad_eff = fold ? 0 : p.pad[l];            // the reflected layer: the gradient of the padded input
        a.Fout = (int)(fold ? p.F[0] + 2 * (int64_t)p.pad[0] : p.F[l]);
        a.nphase = p.stride[l], a.sx = 1, a.dt = -1, a.off = 0, a.reflect = 0;
        a.os = p.stride[l], a.oo = -pad_eff;
        a.ncols = (a.Fout - 1 + pad_eff) / p.stride[l] + 1;
        a.slope = slope;
        a.epi = l ? EPI_MASK : EPI_NONE;
        if (hipError_t e = launch_conv(a, B, p.groups[l], stream)) return e;
        if (fold) {
            const int64_t rows = B * p.c_in[0], tot = rows * p.F[0];
            hipLaunchKernelGGL(sc_fold_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, dst, gx, rows,
                               (int)p.F[0], p.pad[0]);
            if (hipError_t e = hipGetLastError()) return e;
        }
        gz = dst;
    }
    return dg ? launch_stack_wnorm(p, top + 1, g, v, dg, dv, dbias, saved, ws, stream) : hipSuccess;
}

}  // namespace ntm
