// Training of the diffusion generators' network: the fused ResnetBlock of unet_kernels.hip with what its adjoint needs saved, the
// adjoint itself, and the reduction of its weight-gradient partials -- in the WHOLE form (T <= 1024, one workgroup per stream)
// and in the TILED form (any length, one workgroup per window of a tile of 512 frames and 256 of halo a side), one body each.
// fp32 in, fp32 accumulate, no atomics: equal calls give equal bits, and a stream's g_src / gfilm never depend on its batch.
// Notation (unet_block.h): X = film * [src0 from off0 | src1] (cin x T), a = gelu(X), y_0 = W_first a,
//   g_l = gelu(y_l) (0 outside [0, T)), y_{l+1} = (y_l + conv_{k5, d = 2^l}(g_l)) / sqrt 2, out = (y_n + W_res X) / sqrt 2.
//
// unet_block_save_kernel      unet_block_body<true>: the inference forward, which also writes y_0 .. y_{n-1} to [B][n][cout][T].
// unet_block_backward_{layers,tail}_kernel   two launches with gy_0 [B][cout][T] between them in the caller's workspace.
//                     layers: one workgroup per stream walks the layers from n - 1 down to 0 with gy in registers, in the forward's
//                     layout (eight waves: a wave owns up to eight column blocks of 16 frames).  Per layer, gc = gy_{l+1} / sqrt 2 and
//                     g_l = gelu(y_l) (y_l from the save) go to two LDS planes; then
//                       data:    gg_l[ci][q] = sum_{co,t} W_l[co][ci][t] gc[co][q - (t - 2) d]   the forward's MFMA shape with the
//                                weights transposed and the taps mirrored;  gy_l = gc + gg_l * gelu'(y_l)
//                       weights: dW_l[co][ci][t] = sum_f gc[co][f] g_l[ci][f + (t - 2) d]       M = co, N = ci, K = 4 frames per
//                                MFMA, both operands from LDS, summed over the wave's own column blocks.
//                     Where the dW tiles live: in the wave's registers (5 taps x 4 floats a lane), written as per-(stream, wave)
//                     partials for unet_wgrad_reduce_kernel.  The two planes are cout x 1040 floats each (133 KB of the CU's
//                     160 KB), so a cross-wave buffer of 16 x 1280 floats does not fit beside them, and summing through a
//                     plane would cost two more barriers per layer; the partials are 5 KB a wave and layer.
//                     Tail: gy_0 and gout / sqrt 2 in the planes; dW_first = gy_0 a^T and dW_res = (gout / sqrt 2) X^T (K = frames,
//                     X read in place); gX = (W_first^T gy_0) * gelu'(X) + W_res^T gout / sqrt 2 (identity: + gout / sqrt 2);
//                     gfilm = sum_f gX xin through LDS in wave order; gxin = gX film to g_src0 (at off0, 0 outside the crop) and
//                     g_src1; with init_w, dinit_w[ci][k] = sum_f gxin[ci][f] raw[f + off0 + k - 2] and no waveform gradient.
// unet_wgrad_reduce_kernel    out[e] = sum over the partials, in index order, in fp64, rounded once.
// The tiled form: a gated layer's adjoint is local (gy_l[f] needs gc within 2 d of f, dW_l needs g_l within 2 d of an owned
// frame, both from the save, which is right everywhere), so the forward's windows and runs of layers serve backwards:
//   unet_block_save_kernel                 the forward's runs (layers 0-6, layer 7); y_l saved by the tile that owns the frame
//   unet_block_backward_layers_kernel<true>  per run, last to first: layer 7 from gout / sqrt 2, layers 6 .. 0 from its gy_7
//   unet_block_backward_tail_kernel<true>    per tile, no halo; gfilm as a per-(stream, tile) partial
//   unet_wgrad_reduce_groups_kernel        gfilm over a stream's tiles; the weight gradients over a tile's waves, then over a
//                                          stream's tiles; unet_wgrad_reduce_kernel then adds the streams
#include "unet_block.h"

namespace ntm {

__global__ __launch_bounds__(kUWaves * 64) void unet_block_save_kernel(UBlockArgs a, float *ysave) { unet_block_body<true>(a, ysave); }

// the adjoint's workgroup: 512 threads, a wave owns up to eight column blocks.  1024 threads leave 128 registers a lane, which
// the layers kernel (gy, five dW tiles, twenty weights, the operand addresses of five taps) and the tail (two source reads per
// frame, six sums per channel row) both overran into scratch; two waves a SIMD have 256.  Only gy lives in registers across
// the layers, and every loop over column blocks that does not index it stays rolled
constexpr int kBWaves = 8, kBNB = kUW / 16 / kBWaves;

struct UBackArgs {
    UBlockArgs f;                    // the forward's description (y_out, out unused; y_in: the tiled form's gy_{l1} [B][cout][T]
                                     // from the run before, NULL for the first run, which starts from gout / sqrt 2)
    const float *ysave, *gout;
    float *g_src0, *g_src1, *gfilm, *part, *gy0;   // gy0 [B][cout][T]: gy_0 between the two launches
    int NW;                          // waves that own frames: the partials of a stream
    int64_t PS;                      // floats of one partial
};

// d gelu(v) / dv = Phi(v) + v phi(v)
__device__ __forceinline__ float dgelu_f32(float v)
{
    return 0.5f * (1.0f + erff(v * kRsqrt2)) + v * (0.39894228040143267794f * expf(-0.5f * v * v));
}

// The layers of the adjoint, one body for both forms.  TILED: the workgroup is window blockIdx.x of stream blockIdx.y, f0 the
// frame of its position 0 (negative in the first window); it walks the run's layers l1 - 1 .. l0 over the whole window -- gy
// enters from gout / sqrt 2 or from the run before, 0 outside [0, T), and stays correct on a range that shrinks by 2 d a layer
// (a tap that leaves the window reads 0), so the run ends correct on the tile's own frames, which alone are stored and alone
// enter the weight gradients.  Not TILED: the window is the signal, f0 = 0, every frame is owned, all layers.
template <bool TILED>
__global__ __launch_bounds__(kBWaves * 64) void unet_block_backward_layers_kernel(UBackArgs k)
{
    extern __shared__ float lds[];
    const UBlockArgs &a = k.f;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int64_t b = TILED ? blockIdx.y : blockIdx.x;
    // the tiled window is a constant: kUW frames = kUTile + 2 kUHalo
    const int cout = a.cout, cq = a.CP >> 2, P = TILED ? kUW + 16 : a.P, T = a.T, W = TILED ? kUW : a.W, n = a.nl;
    const int plane = a.CP * P, wn = cout * cout * 5;
    const int f0 = TILED ? (int)blockIdx.x * kUTile - kUHalo : 0, lhi = TILED ? a.l1 : n, llo = TILED ? a.l0 : 0;
    float *GC = lds, *GL = lds + plane;                               // gc; g_l
    const bool active = TILED || wave < k.NW;
    // written by active waves only; tiled: a partial per (stream, tile, wave)
    float *part = k.part + (TILED ? (b * gridDim.x + blockIdx.x) * kBWaves + wave : b * k.NW + (active ? wave : 0)) * k.PS;
    // element (row kq * 4 + r, frame of column block j) of a [cout][T] plane: o0 + r T + 128 j, one lane offset for all
    const int o0 = kq * 4 * T + wave * 16 + li + f0;
    float *gy0 = k.gy0 + b * cout * T;

    // ---- gy_n = gout / sqrt 2 (tiled, a later run: gy_{l1} as the run before left it) ----
    f32x4 GY[kBNB];
    {
        const bool first = !TILED || !a.y_in;
        const float *go = (first ? k.gout : a.y_in) + b * cout * T;
        const float sc = first ? kRsqrt2 : 1.0f;
#pragma unroll
        for (int j = 0; j < kBNB; ++j) {
            const int f = (j * kBWaves + wave) * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                GY[j][r] = (kq * 4 + r < cout && (TILED ? (unsigned)(f0 + f) < (unsigned)T : f < T)) ? go[o0 + r * T + j * (kBWaves * 16)] * sc : 0.0f;
        }
    }

    // ---- the gated layers, last to first ----
    for (int l = lhi - 1; l >= llo; --l) {
        const int d = 1 << l;
        const float *yl = k.ysave + (b * n + l) * cout * T;
#pragma unroll
        for (int j = 0; j < kBNB; ++j) {
            const int p0 = (j * kBWaves + wave) * 16, f = p0 + li;
            if (p0 >= W) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kq * 4 + r;
                const bool ok = row < cout && (TILED ? (unsigned)(f0 + f) < (unsigned)T : f < T);
                const float y = ok ? yl[o0 + r * T + j * (kBWaves * 16)] : 0.0f;
                GY[j][r] *= kRsqrt2;                       // gc: 0 outside [0, T) and below c_out, as gy is
                if (row < a.CP) {
                    GC[row * P + f] = GY[j][r];
                    GL[row * P + f] = ok ? gelu_f32(y) : 0.0f;
                }
            }
        }
        __syncthreads();

        // weights: the wave's column blocks, K = 4 frames per MFMA
        {
            f32x4 dw[5];
#pragma unroll
            for (int t = 0; t < 5; ++t) dw[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const bool rok = li < cout;
#pragma unroll 1
            for (int j = 0; j < kBNB; ++j) {
                const int p0 = (j * kBWaves + wave) * 16;
                if (p0 >= W) continue;
                if (TILED && (p0 < kUHalo || p0 >= kUHalo + kUTile)) continue;     // own frames only: whole column blocks
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int fa = p0 + 4 * s + kq;
                    const float gcv = GC[(rok ? li : 0) * P + fa];
                    const float av = rok ? gcv : 0.0f;
#pragma unroll
                    for (int t = 0; t < 5; ++t) {
                        const int q = fa + (t - 2) * d;
                        const bool ok = rok && q >= 0 && q < W;
                        const float g = GL[ok ? li * P + q : 0];
                        dw[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ok ? g : 0.0f, dw[t], 0, 0, 0);
                    }
                }
            }
            if (active) {
#pragma unroll
                for (int t = 0; t < 5; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int co = kq * 4 + r;
                        if (co < cout && li < cout) (part + l * wn)[(kq * 4 * cout + li) * 5 + r * cout * 5 + t] = dw[t][r];
                    }
            }
        }

        // data: the forward's shape, weights transposed (M = ci, K = co), taps mirrored
        __builtin_amdgcn_sched_barrier(0);     // the two contractions one after the other: their operands do not fit side by side
        {
            const float *wl = a.w_gated + (int64_t)l * wn;
            float wv[5][4];
#pragma unroll
            for (int t = 0; t < 5; ++t)
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const int co = c4 * 4 + kq;
                    const bool ok = li < cout && co < cout;
                    const float w = wl[ok ? (co * cout + li) * 5 + t : 0];
                    wv[t][c4] = ok ? w : 0.0f;
                }
#pragma unroll
            for (int j = 0; j < kBNB; ++j) {
                const int p0 = (j * kBWaves + wave) * 16, f = p0 + li;
                if (p0 >= W) continue;
                float y[4];                                // y_l again (from the cache): its gelu' scales gg below
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = kq * 4 + r;
                    y[r] = (row < cout && (TILED ? (unsigned)(f0 + f) < (unsigned)T : f < T)) ? yl[o0 + r * T + j * (kBWaves * 16)] : 0.0f;
                }
                f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const int q = f - (t - 2) * d;
                    const bool ok = q >= 0 && q < W;
                    const int qi = ok ? q : 0;
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        if (c4 < cq) {
                            const float g = GC[(c4 * 4 + kq) * P + qi];
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t][c4], ok ? g : 0.0f, acc, 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = kq * 4 + r;
                    if (row < cout && (TILED ? (unsigned)(f0 + f) < (unsigned)T : f < T)) GY[j][r] = fmaf(acc[r], dgelu_f32(y[r]), GY[j][r]);
                }
                __builtin_amdgcn_sched_barrier(0);         // one column block's operands at a time
            }
        }
        __syncthreads();
    }

    // ---- gy_0 leaves for the tail (tiled: gy_{l0} at the tile's own frames, for the next run or the tail) ----
#pragma unroll
    for (int j = 0; j < kBNB; ++j) {
        const int f = (j * kBWaves + wave) * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (f0 + f < T && (!TILED || (f >= kUHalo && f < kUHalo + kUTile)) && kq * 4 + r < cout) gy0[o0 + r * T + j * (kBWaves * 16)] = GY[j][r];
    }
}


// The tail of the adjoint, a launch of its own (the two halves together do not fit the registers of 1024 threads): gy_0 from
// the layers kernel and go = gout / sqrt 2 in the planes, then the 1x1s, FiLM, the sources and init_w.
// TILED: the 1x1s need no halo, so the workgroup is tile blockIdx.x of stream blockIdx.y with no halo: window position p is
// frame f0 + p, the window the tile's frames.  Its weight-gradient partials go beside the layers kernel's, per (stream, tile,
// wave), and gfilm leaves as a per-(stream, tile) partial [B][tiles][cin] for the fixed-order sum.
template <bool TILED>
__global__ __launch_bounds__(kBWaves * 64) void unet_block_backward_tail_kernel(UBackArgs k)
{
    extern __shared__ float lds[];
    const UBlockArgs &a = k.f;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int64_t b = TILED ? blockIdx.y : blockIdx.x;
    const int cin = a.c0 + a.c1, cout = a.cout, cq = a.CP >> 2, P = TILED ? kUW + 16 : a.P, T = a.T, W = TILED ? kUTile : a.W, n = a.nl;
    const int plane = a.CP * P, wn = cout * cout * 5;
    const int f0 = TILED ? (int)blockIdx.x * kUTile : 0;
    float *GC = lds, *GL = lds + plane, *red = lds + 2 * plane;      // gy_0; go; [waves][32] sums of gfilm
    const float *film = a.film + b * a.film_stride;
    const bool active = TILED || wave < k.NW;
    // written by active waves only; tiled: a partial per (stream, tile, wave)
    float *part = k.part + (TILED ? (b * gridDim.x + blockIdx.x) * kBWaves + wave : b * k.NW + (active ? wave : 0)) * k.PS;
    {
        const float *gy0 = k.gy0 + b * cout * T + f0, *go = k.gout + b * cout * T + f0;
        for (int i = tid; i < a.CP * W; i += kBWaves * 64) {
            const int row = i / W, f = i - row * W;
            const bool ok = row < cout && f0 + f < T;
            const float v0 = gy0[ok ? row * T + f : 0], v1 = go[ok ? row * T + f : 0];
            GC[row * P + f] = ok ? v0 : 0.0f;
            GL[row * P + f] = ok ? v1 * kRsqrt2 : 0.0f;
        }
    }
    __syncthreads();

    const int64_t off_first = (int64_t)n * wn, off_res = off_first + cout * cin, off_init = off_res + cout * cin;
    const int mt = (cin + 15) >> 4;
    for (int m = 0; m < mt; ++m) {
        // dW_first = gy_0 a^T, dW_res = go X^T: M = co, N = ci of this tile, K = 4 frames per MFMA
        {
            f32x4 df = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, dr = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const bool rok = li < cout;
            const int ci = m * 16 + li;
            const float fl = ci < cin ? film[ci] : 0.0f;
#pragma unroll 1
            for (int j = 0; j < kBNB; ++j) {
                const int p0 = (j * kBWaves + wave) * 16;
                if (p0 >= W) continue;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int fa = p0 + 4 * s + kq;
                    const float v1 = GC[(rok ? li : 0) * P + fa], v2 = GL[(rok ? li : 0) * P + fa];
                    const float xv = (ci < cin && f0 + fa < T) ? ublock_src(a, b, ci, f0 + fa) * fl : 0.0f;
                    df = __builtin_amdgcn_mfma_f32_16x16x4f32(rok ? v1 : 0.0f, gelu_f32(xv), df, 0, 0, 0);
                    if (a.w_res) dr = __builtin_amdgcn_mfma_f32_16x16x4f32(rok ? v2 : 0.0f, xv, dr, 0, 0, 0);
                }
            }
            if (active) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = kq * 4 + r;
                    if (co < cout && ci < cin) {
                        part[off_first + co * cin + ci] = df[r];
                        part[off_res + co * cin + ci] = dr[r];
                    }
                }
            }
        }

        // gX of the tile's channels: M = ci, N = 16 frames, K = co
        float wf[4], wr[4];
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
            const int co = c4 * 4 + kq, ci = m * 16 + li;
            const bool ok = co < cout && ci < cin;
            const float w1 = a.w_first[ok ? co * cin + ci : 0];
            wf[c4] = ok ? w1 : 0.0f;
            wr[c4] = 0.0f;
            if (a.w_res) {
                const float w2 = a.w_res[ok ? co * cin + ci : 0];
                wr[c4] = ok ? w2 : 0.0f;
            }
        }
        float s[4][6];                       // per channel row: gfilm, then the five taps of dinit_w
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) s[r][c] = 0.0f;
#pragma unroll 1
        for (int j = 0; j < kBNB; ++j) {
            const int p0 = (j * kBWaves + wave) * 16, f = p0 + li;
            if (p0 >= W) continue;
            f32x4 p1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, p2 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                if (c4 < cq) {
                    p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[c4], GC[(c4 * 4 + kq) * P + f], p1, 0, 0, 0);
                    if (a.w_res) p2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[c4], GL[(c4 * 4 + kq) * P + f], p2, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = m * 16 + kq * 4 + r;
                if (ci >= cin || f0 + f >= T) continue;
                const float xin = ublock_src(a, b, ci, f0 + f), fl = film[ci];
                const float res = a.w_res ? p2[r] : GL[ci * P + f];        // the identity residual: cin == cout
                const float gX = fmaf(p1[r], dgelu_f32(xin * fl), res);
                s[r][0] = fmaf(gX, xin, s[r][0]);
                const float gxin = gX * fl;
                if (ci < a.c0) {
                    if (a.init_w) {
                        const float *raw = a.src0 + b * a.T0;
#pragma unroll
                        for (int t = 0; t < 5; ++t) {
                            const int q = f0 + f + a.off0 + t - 2;
                            const bool ok = q >= 0 && q < a.T0;
                            const float v = raw[ok ? q : 0];
                            s[r][1 + t] = fmaf(gxin, ok ? v : 0.0f, s[r][1 + t]);
                        }
                    } else if (k.g_src0) {
                        k.g_src0[(b * a.c0 + ci) * a.T0 + a.off0 + f0 + f] = gxin;
                    }
                } else if (k.g_src1) {
                    k.g_src1[(b * a.c1 + (ci - a.c0)) * a.T1 + a.off1 + f0 + f] = gxin;
                }
            }
        }
        // the 16 frames of a column block, in a fixed order
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                float v = s[r][c];
#pragma unroll
                for (int x = 1; x < 16; x <<= 1) v += __shfl_xor(v, x, 64);
                s[r][c] = v;
            }
        if (li == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = m * 16 + kq * 4 + r;
                red[wave * 32 + ci] = s[r][0];
                if (active && a.init_w && ci < a.c0) {
#pragma unroll
                    for (int t = 0; t < 5; ++t) part[off_init + ci * 5 + t] = s[r][1 + t];
                }
            }
        }
    }
    __syncthreads();
    if (tid < cin) {
        float v = 0.0f;
        for (int w = 0; w < kBWaves; ++w) v += red[w * 32 + tid];
        k.gfilm[(TILED ? b * gridDim.x + blockIdx.x : b) * cin + tid] = v;
    }
    // frames of the sources that the block never read (tiled: those before the crop with the first tile, those behind it with
    // the last)
    if (TILED) {
        for (int s = 0; s < 2; ++s) {
            float *g = s ? k.g_src1 : k.g_src0;
            const int c = s ? a.c1 : a.c0, Ts = s ? a.T1 : a.T0, off = s ? a.off1 : a.off0, hi = Ts - off - T;
            if (!g || (s == 0 && a.init_w)) continue;
            g += b * c * Ts;
            if (blockIdx.x == 0)
                for (int i = tid; i < c * off; i += kBWaves * 64) g[(i / off) * Ts + i % off] = 0.0f;
            if (blockIdx.x == gridDim.x - 1)
                for (int i = tid; i < c * hi; i += kBWaves * 64) g[(i / hi) * Ts + off + T + i % hi] = 0.0f;
        }
        return;
    }
    if (k.g_src0 && !a.init_w)
        for (int i = tid; i < a.c0 * a.T0; i += kBWaves * 64) {
            const int f = i % a.T0;
            if (f < a.off0 || f >= a.off0 + T) k.g_src0[b * a.c0 * a.T0 + i] = 0.0f;
        }
    if (k.g_src1)
        for (int i = tid; i < a.c1 * a.T1; i += kBWaves * 64) {
            const int f = i % a.T1;
            if (f < a.off1 || f >= a.off1 + T) k.g_src1[b * a.c1 * a.T1 + i] = 0.0f;
        }
}

__global__ __launch_bounds__(256) void unet_wgrad_reduce_kernel(const float *__restrict__ part, int64_t count, int64_t n,
                                                                float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double acc = 0.0;
    for (int64_t p = 0; p < count; ++p) acc += (double)part[p * n + e];
    out[e] = (float)acc;
}

// the same sum for `groups` sets of `count` partials each, one behind the other: out[g][e] = sum_p part[(g count + p) n + e]
__global__ __launch_bounds__(256) void unet_wgrad_reduce_groups_kernel(const float *__restrict__ part, int64_t count, int64_t n,
                                                                       float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x, g = blockIdx.x;
    if (e >= n) return;
    const float *p = part + g * count * n + e;
    double acc = 0.0;
#pragma unroll 8
    for (int64_t i = 0; i < count; ++i) acc += (double)p[i * n];
    out[g * n + e] = (float)acc;
}

// floats of one weight-gradient partial: [n][cout][cout][5] | [cout][cin] first | [cout][cin] res | [c0][5] init (with init)
int64_t unet_block_wgrad_floats(const ntm_unet_block &k)
{
    const int64_t cin = k.c0 + k.c1;
    return (int64_t)k.n_layers * k.c_out * k.c_out * 5 + 2 * k.c_out * cin + (k.init ? k.c0 * 5 : 0);
}

// partials of one stream: the waves that own frames
int unet_block_partials(const ntm_unet_block &k)
{
    const int64_t blocks = (k.T + 15) / 16;
    return (int)(blocks < kBWaves ? blocks : kBWaves);
}

hipError_t launch_unet_block_save(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                                  const float *w_first, const float *w_gated, const float *w_res, int64_t B, const ntm_unet_block &k,
                                  float *ysave, float *out, hipStream_t stream)
{
    UBlockArgs a = unet_block_args(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, k, out);
    a.l0 = 0, a.l1 = k.n_layers;
    const size_t lds = unet_block_lds_bytes(a);
    if (lds > 64 * 1024)
        if (hipError_t e = hipFuncSetAttribute((const void *)unet_block_save_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
            return e;
    hipLaunchKernelGGL(unet_block_save_kernel, dim3(1, (unsigned)B), dim3(kUWaves * 64), lds, stream, a, ysave);
    return hipGetLastError();
}

hipError_t launch_unet_block_backward(const float *src0, const float *src1, const float *init_w, const float *film,
                                      int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res, int64_t B,
                                      const ntm_unet_block &k, const float *ysave, const float *gout, float *ws, float *g_src0,
                                      float *g_src1, float *gfilm, float *part, hipStream_t stream)
{
    UBackArgs q{};
    q.f = unet_block_args(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, k, nullptr);
    q.f.l0 = 0, q.f.l1 = k.n_layers;
    q.ysave = ysave, q.gout = gout, q.g_src0 = g_src0, q.g_src1 = g_src1, q.gfilm = gfilm, q.part = part, q.gy0 = ws;
    q.NW = unet_block_partials(k), q.PS = unet_block_wgrad_floats(k);
    const size_t lds = ((size_t)2 * q.f.CP * q.f.P + kBWaves * 32) * sizeof(float);
    if (lds > 64 * 1024)
        for (const void *fn : {(const void *)unet_block_backward_layers_kernel<false>, (const void *)unet_block_backward_tail_kernel<false>})
            if (hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
    hipLaunchKernelGGL(unet_block_backward_layers_kernel<false>, dim3((unsigned)B), dim3(kBWaves * 64), lds, stream, q);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(unet_block_backward_tail_kernel<false>, dim3((unsigned)B), dim3(kBWaves * 64), lds, stream, q);
    return hipGetLastError();
}

// ---- the tiled form ----
// tiles of a stream; the runs of layers are the forward's (ublock_run_end), walked backwards by the adjoint
int64_t unet_block_tiles(const ntm_unet_block &k) { return (k.T + kUTile - 1) / kUTile; }

static int unet_block_tiled_runs(const ntm_unet_block &k, int *l0s)
{
    int n = 0;
    for (int l = 0; l < k.n_layers; l = ublock_run_end(l, k.n_layers)) l0s[n++] = l;
    return n;
}

// floats of the adjoint's workspace: gy [B][cout][T] between its launches (two planes in turn from three launches on), then
// the gfilm partials [B][tiles][cin]
int64_t unet_block_tiled_workspace(int64_t B, const ntm_unet_block &k)
{
    int l0s[8];
    const int runs = unet_block_tiled_runs(k, l0s);
    return (runs > 1 ? 2 : 1) * B * k.c_out * k.T + B * unet_block_tiles(k) * (k.c0 + k.c1);
}

// partials of the tiled adjoint, in units of one partial: [B] per stream | [B tiles] per tile | [B tiles waves] as written
int64_t unet_block_tiled_partials(int64_t B, const ntm_unet_block &k) { return B * (1 + unet_block_tiles(k) * (1 + kBWaves)); }

static ntm_unet_block tiled(ntm_unet_block k)
{
    k.form = NTM_UNET_TILED;
    return k;
}

hipError_t launch_unet_block_tiled_save(const float *src0, const float *src1, const float *init_w, const float *film,
                                        int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res, int64_t B,
                                        const ntm_unet_block &k, float *ysave, float *out, hipStream_t stream)
{
    UBlockArgs a = unet_block_args(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, tiled(k), out);
    const size_t lds = unet_block_lds_bytes(a);
    if (lds > 64 * 1024)
        if (hipError_t e = hipFuncSetAttribute((const void *)unet_block_save_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
            return e;
    const dim3 grid((unsigned)unet_block_tiles(k), (unsigned)B);
    for (int l = 0; l < k.n_layers; l = a.l1) {
        a.l0 = l, a.l1 = ublock_run_end(l, k.n_layers);
        hipLaunchKernelGGL(unet_block_save_kernel, grid, dim3(kUWaves * 64), lds, stream, a, ysave);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// part: unet_block_tiled_partials(B, k) partials; its first B are the per-stream sums the caller reduces
hipError_t launch_unet_block_tiled_backward(const float *src0, const float *src1, const float *init_w, const float *film,
                                            int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res,
                                            int64_t B, const ntm_unet_block &k, const float *ysave, const float *gout, float *ws,
                                            float *g_src0, float *g_src1, float *gfilm, float *part, hipStream_t stream)
{
    UBackArgs q{};
    q.f = unet_block_args(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, tiled(k), nullptr);
    const int64_t tiles = unet_block_tiles(k), plane = B * k.c_out * k.T, PS = unet_block_wgrad_floats(k);
    const int cin = k.c0 + k.c1;
    int l0s[8];
    const int runs = unet_block_tiled_runs(k, l0s);
    float *gfp = ws + (runs > 1 ? 2 : 1) * plane, *mid = part + B * PS, *raw = mid + B * tiles * PS;
    q.ysave = ysave, q.gout = gout, q.g_src0 = g_src0, q.g_src1 = g_src1, q.gfilm = gfp, q.part = raw;
    q.NW = kBWaves, q.PS = PS;
    const size_t lds = ((size_t)2 * q.f.CP * q.f.P + kBWaves * 32) * sizeof(float);
    if (lds > 64 * 1024)
        for (const void *fn : {(const void *)unet_block_backward_layers_kernel<true>, (const void *)unet_block_backward_tail_kernel<true>})
            if (hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
    const dim3 grid((unsigned)tiles, (unsigned)B);
    for (int r = 0; r < runs; ++r) {                 // the forward's runs, last to first
        q.f.l0 = l0s[runs - 1 - r], q.f.l1 = r ? l0s[runs - r] : k.n_layers;
        q.f.y_in = r ? ws + ((r - 1) & 1) * plane : nullptr, q.gy0 = ws + (r & 1) * plane;
        hipLaunchKernelGGL(unet_block_backward_layers_kernel<true>, grid, dim3(kBWaves * 64), lds, stream, q);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(unet_block_backward_tail_kernel<true>, grid, dim3(kBWaves * 64), lds, stream, q);
    if (hipError_t e = hipGetLastError()) return e;
    // gfilm over a stream's tiles; the weight gradients over a tile's waves, then over a stream's tiles
    const auto reduce = [&](const float *in, int64_t groups, int64_t count, int64_t n, float *o) {
        hipLaunchKernelGGL(unet_wgrad_reduce_groups_kernel, dim3((unsigned)groups, (unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           in, count, n, o);
        return hipGetLastError();
    };
    if (hipError_t e = reduce(gfp, B, tiles, cin, gfilm)) return e;
    if (hipError_t e = reduce(raw, B * tiles, kBWaves, PS, mid)) return e;
    return reduce(mid, B, tiles, PS, part);
}

hipError_t launch_unet_wgrad_reduce(const float *part, int64_t count, int64_t n, float *out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;      // count = 0 is launched: out <- 0
    hipLaunchKernelGGL(unet_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part, count, n, out);
    return hipGetLastError();
}

}  // namespace ntm
