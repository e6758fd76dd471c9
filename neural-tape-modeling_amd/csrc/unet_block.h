// The fused ResnetBlock of the diffusion generators, shared by its inference kernel (unet_kernels.hip: unet_block_kernel) and
// its training kernels (unet_train.hip: the same forward that also saves y_0 .. y_{n-1}, and the adjoint): the arguments, the
// block's input read in place and the forward's body, written once.  The notation is unet_kernels.hip's.
#pragma once
#include "ntm_common.h"

namespace ntm {

constexpr int kUW = NTM_UNET_WHOLE_MAX_T;   // frames of a window at most
constexpr int kUTile = NTM_UNET_TILE, kUHalo = (kUW - kUTile) / 2;
constexpr int kUWaves = 16, kUNB = kUW / 16 / kUWaves;   // 1024 threads; column blocks of 16 frames per wave
constexpr int kUWn = 16 * 16 * 5;                         // floats of one gated layer's weights at most
constexpr float kRsqrt2 = 0.70710678118654752440f;

struct UBlockArgs {
    const float *src0, *src1, *init_w, *film, *w_first, *w_gated, *w_res, *y_in;
    float *y_out, *out;
    int64_t film_stride;
    int c0, c1, cout, l0, l1, nl;
    int T, T0, off0, T1, off1;
    int tile, halo, W, P, CP;   // window: W frames (a multiple of 16) = tile + 2 halo; LDS pitch; rows of a plane (c_out up to 4)
};

__device__ __forceinline__ float gelu_f32(float v) { return 0.5f * v * (1.0f + erff(v * kRsqrt2)); }

// channel ci of the block's input at frame f of the block (0 <= f < T), before FiLM
__device__ __forceinline__ float ublock_src(const UBlockArgs &a, int64_t b, int ci, int f)
{
    if (ci < a.c0) {
        const int g = f + a.off0;
        if (a.init_w) {
            const float *raw = a.src0 + b * a.T0;
            float v = 0.0f;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int q = g + k - 2;
                const bool ok = q >= 0 && q < a.T0;
                const float r = raw[ok ? q : 0];
                v = fmaf(a.init_w[ci * 5 + k], ok ? r : 0.0f, v);
            }
            return v;
        }
        return a.src0[(b * a.c0 + ci) * a.T0 + g];
    }
    return a.src1[(b * a.c1 + (ci - a.c0)) * a.T1 + f + a.off1];
}

// window position p of a frame in [0, T): one of the tile's own frames, not the halo's
__device__ __forceinline__ bool ublock_mine_in(const UBlockArgs &a, int p) { return (unsigned)(p - a.halo) < (unsigned)a.tile; }

// The forward of one window of one stream.  SAVE: y_l of every gated layer l < nl also goes to ysave [B][nl][cout][T], for the
// adjoint, at the frames the window OWNS (deep in a fused run the halo's values are not the signal's; in the whole form every
// frame is owned).  Between the runs of the tiled form y travels in the save itself: a run reads y_{l0} from its plane and
// leaves y_{l1} in the next one, y_in / y_out are not read.  Without SAVE the pointer is not read and the code is the inference
// kernel's.
template <bool SAVE>
__device__ __forceinline__ void unet_block_body(UBlockArgs a, float *ysave)
{
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int64_t b = blockIdx.y;
    const int f0 = (int)blockIdx.x * a.tile - a.halo;    // frame of window position 0
    const int cin = a.c0 + a.c1, cout = a.cout, cq = a.CP >> 2, P = a.P;
    const int plane = a.CP * P;
    const float *film = a.film + b * a.film_stride;

    // the gated weights of one layer, twice: layer l is read from LDS while layer l + 1 is on its way from memory
    float *wb = lds + 2 * plane;
    const int wn = cout * cout * 5;                      // <= kUWn
    {
        const float *w0 = a.w_gated + (int64_t)a.l0 * wn;
        for (int i = tid; i < wn; i += kUWaves * 64) wb[i] = w0[i];
    }

    f32x4 Y[kUNB];
    // ---- the value the run of layers starts from ----
#pragma unroll
    for (int j = 0; j < kUNB; ++j) {
        const int p0 = (j * kUWaves + wave) * 16;
        Y[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (p0 >= a.W) continue;
        const int f = f0 + p0 + li;
        const bool in = f >= 0 && f < a.T;
        if (a.l0 == 0) {
            // the operands of every K step first (independent loads: one memory latency), then the chain of MFMAs
            float av[8], bv[8];
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4) {
                const int ci = c4 * 4 + kq;
                const bool cok = ci < cin;
                av[c4] = (cok && li < cout) ? a.w_first[li * cin + ci] : 0.0f;
                bv[c4] = (cok && in) ? ublock_src(a, b, ci, f) * film[ci] : 0.0f;
            }
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4)
                if (c4 * 4 < cin) Y[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c4], gelu_f32(bv[c4]), Y[j], 0, 0, 0);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kq * 4 + r;
                if (row < cout && in) {
                    if constexpr (SAVE)
                        Y[j][r] = (ysave + (b * a.nl + a.l0) * cout * a.T)[row * a.T + f];
                    else
                        Y[j][r] = a.y_in[(b * cout + row) * a.T + f];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = kq * 4 + r;
            if (row < a.CP) lds[row * P + p0 + li] = in ? gelu_f32(Y[j][r]) : 0.0f;
            if (SAVE && a.l0 == 0 && row < cout && in && ublock_mine_in(a, p0 + li)) (ysave + b * a.nl * cout * a.T)[row * a.T + f] = Y[j][r];
        }
    }
    __syncthreads();

    // ---- the gated layers l0 .. l1 - 1 ----
    int cur = 0;
    for (int l = a.l0; l < a.l1; ++l) {
        const int d = 1 << l;
        const bool more = l + 1 < a.l1;
        const float *wnext = a.w_gated + (int64_t)(l + 1) * wn;
        float pre[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + i * kUWaves * 64;
            pre[i] = (more && e < wn) ? wnext[e] : 0.0f;
        }
        const float *wl = wb + cur * kUWn;
        float wv[5][4];
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const int ci = c4 * 4 + kq;
                const bool ok = li < cout && ci < cout;
                const float w = wl[ok ? (li * cout + ci) * 5 + t : 0];
                wv[t][c4] = ok ? w : 0.0f;
            }
        const float *G = lds + cur * plane;
        float *Gn = lds + (cur ^ 1) * plane;
#pragma unroll
        for (int j = 0; j < kUNB; ++j) {
            const int p0 = (j * kUWaves + wave) * 16;
            if (p0 >= a.W) continue;
            f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int q = p0 + li + (t - 2) * d;
                const bool ok = q >= 0 && q < a.W;
                const int qi = ok ? q : 0;
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    if (c4 < cq) {
                        const float g = G[(c4 * 4 + kq) * P + qi];
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t][c4], ok ? g : 0.0f, acc, 0, 0, 0);
                    }
                }
            }
            const int f = f0 + p0 + li;
            const bool in = f >= 0 && f < a.T;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Y[j][r] = (Y[j][r] + acc[r]) * kRsqrt2;
                const int row = kq * 4 + r;
                if (more && row < a.CP) Gn[row * P + p0 + li] = in ? gelu_f32(Y[j][r]) : 0.0f;
                if (SAVE && more && row < cout && in && ublock_mine_in(a, p0 + li)) (ysave + (b * a.nl + l + 1) * cout * a.T)[row * a.T + f] = Y[j][r];
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + i * kUWaves * 64;
            if (more && e < wn) wb[(cur ^ 1) * kUWn + e] = pre[i];
        }
        __syncthreads();
        cur ^= 1;
    }

    // ---- the tile's frames leave: y for the next run of layers, or the block's output with the residual ----
    const bool last = a.l1 == a.nl;
#pragma unroll
    for (int j = 0; j < kUNB; ++j) {
        const int p0 = (j * kUWaves + wave) * 16;
        if (p0 >= a.W) continue;
        const int p = p0 + li, f = f0 + p;
        const bool mine = p >= a.halo && p < a.halo + a.tile && f < a.T;     // f >= 0 there
        if (!last) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kq * 4 + r;
                if (mine && row < cout) {
                    if constexpr (SAVE)
                        (ysave + (b * a.nl + a.l1) * cout * a.T)[row * a.T + f] = Y[j][r];
                    else
                        a.y_out[(b * cout + row) * a.T + f] = Y[j][r];
                }
            }
            continue;
        }
        f32x4 res = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (a.w_res) {
            float av[8], bv[8];
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4) {
                const int ci = c4 * 4 + kq;
                const bool cok = ci < cin;
                av[c4] = (cok && li < cout) ? a.w_res[li * cin + ci] : 0.0f;
                bv[c4] = (cok && mine) ? ublock_src(a, b, ci, f) * film[ci] : 0.0f;
            }
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4)
                if (c4 * 4 < cin) res = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c4], bv[c4], res, 0, 0, 0);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kq * 4 + r;
                if (mine && row < cout) res[r] = ublock_src(a, b, row, f) * film[row];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = kq * 4 + r;
            if (mine && row < cout) a.out[(b * cout + row) * a.T + f] = (Y[j][r] + res[r]) * kRsqrt2;
        }
    }
}

__host__ __device__ inline bool ublock_whole(const ntm_unet_block &k) { return k.form == 1 || (k.form == 0 && k.T <= kUW); }

// the description of a launch, filled from a block description the API has checked (on the device too: the one-launch sampler,
// unet_sampler.hip, fills it per stage from its table)
__host__ __device__ inline UBlockArgs unet_block_args(const float *src0, const float *src1, const float *init_w, const float *film,
                                                      int64_t film_stride, const float *w_first, const float *w_gated,
                                                      const float *w_res, const ntm_unet_block &k, float *out)
{
    UBlockArgs a{};
    a.src0 = src0, a.src1 = src1, a.init_w = k.init ? init_w : nullptr, a.film = film, a.film_stride = film_stride;
    a.w_first = w_first, a.w_gated = w_gated, a.w_res = w_res, a.out = out;
    a.c0 = k.c0, a.c1 = k.c1, a.cout = k.c_out, a.nl = k.n_layers;
    a.T = (int)k.T, a.T0 = (int)k.T0, a.off0 = (int)k.off0, a.T1 = (int)k.T1, a.off1 = (int)k.off1;
    a.CP = (k.c_out + 3) & ~3;
    if (ublock_whole(k)) {
        a.W = ((int)k.T + 15) & ~15, a.tile = a.W, a.halo = 0;
    } else {
        a.W = kUW, a.tile = kUTile, a.halo = kUHalo;
    }
    a.P = a.W + 16;     // 16 mod 64 floats: the four channel rows of an MFMA operand read fall on 64 different banks
    return a;
}
size_t unet_block_lds_bytes(const UBlockArgs &a);       // unet_kernels.hip
int ublock_run_end(int l0, int nl);     // layers [l0, l1) of a tiled run

}  // namespace ntm
