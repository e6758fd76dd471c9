// The diffusion generators' network and sampler step (UNet1D, code/networks/unet_1d.py; DiffusionGenerator, code/model.py:656-891):
// inference only, fp32 in, fp32 accumulate, no atomics -- equal calls give equal bits and a stream never sees its batch.
//
// unet_block_kernel   a whole ResnetBlock, or a run of its gated layers, for one window of one stream per workgroup:
//                       x = film * [src0 (from frame off0: CropConcatBlock's centre crop) | src1]    -- never materialised; with
//                           init_w, src0 is the waveform and its channels are Conv1d(1, c0, 5, "same") of it, computed on the fly
//                       y = W_first gelu(x);   n times  y <- (y + conv_{k5, d = 2^l}(gelu(y))) / sqrt 2;   out = (y + W_res x) / sqrt 2
//                     Every contraction runs on v_mfma_f32_16x16x4_f32: M = c_out padded to 16, N = 16 frames, K = 4 channels of
//                     one tap per instruction (K = c_in for the 1x1s, 5 c_out for a gated layer).  A wave owns up to four column
//                     blocks of 16 frames and keeps their y in registers for the whole run of layers; only gelu(y) goes through
//                     LDS, in two planes that the layers read and write in turn -- one barrier per layer.  A layer's weights
//                     are read from LDS too, where the layer before put them while it ran its MFMAs: no layer waits on memory.
//                     Zero padding: gelu(y) is stored as 0 for every frame outside [0, T) at EVERY layer (the reference pads each
//                     layer's input with zeros; a halo value computed from out-of-range frames would not be zero), and a tap that
//                     leaves the window reads 0.
//                     Two forms.  WHOLE (T <= 1024): the window is the signal, no halo, all layers, one launch.  TILED: windows
//                     of 1024 frames = a tile of 512 and a halo of 256 a side; a run of layers is fused while 2 sum(d) <= 256, so
//                     the eight dilations 1 .. 128 take TWO launches (layers 0-6: 254 frames of halo; layer 7: 256), with y
//                     between them in the caller's workspace.  Halo frames are recomputed by both neighbours (2x the
//                     arithmetic, which is small next to a launch).
// unet_down_kernel    Downsample(S) of x and pyr by the polyphase FIR from the module's buffer + CombinerDown.
// unet_up_kernel      CombinerUp + Upsample(S) of x and pyr (S phases of 2 width + 1 taps); S = 1: the combiner alone; without
//                     weights: a plain upsampler (the sampler's 100 Hz -> 44.1 kHz resampler, 441 phases).
// edm_pre / edm_post  the sampler's step around the network, in the reference's order of operations.
// The block's arguments and the forward's body are in unet_block.h, which the training kernels (unet_train.hip) share; what
// the other kernels compute per output is in unet_steps.h, which the one-launch sampler (unet_sampler.hip) shares.
#include "unet_steps.h"

namespace ntm {

__global__ __launch_bounds__(kUWaves * 64) void unet_block_kernel(UBlockArgs a) { unet_block_body<false>(a, nullptr); }

// layers [l0, l1) of a tiled run: as many as keep 2 sum(d) within the halo
int ublock_run_end(int l0, int nl)
{
    int l1 = l0, reach = 0;
    while (l1 < nl && reach + (2 << l1) <= kUHalo) reach += 2 << l1, ++l1;    // a layer of dilation d reaches 2 d a side
    return l1 > l0 ? l1 : l0 + 1;
}

int unet_block_launches(const ntm_unet_block &k)
{
    if (ublock_whole(k)) return 1;
    int n = 0;
    for (int l = 0; l < k.n_layers; l = ublock_run_end(l, k.n_layers)) ++n;
    return n;
}

// floats of workspace: y between the runs of the tiled form, two buffers when there are more than two runs
int64_t unet_block_workspace(int64_t B, const ntm_unet_block &k)
{
    const int n = unet_block_launches(k);
    return n <= 1 ? 0 : (n == 2 ? 1 : 2) * B * k.c_out * k.T;
}

size_t unet_block_lds_bytes(const UBlockArgs &a) { return ((size_t)2 * a.CP * a.P + 2 * kUWn) * sizeof(float); }

hipError_t launch_unet_block(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                             const float *w_first, const float *w_gated, const float *w_res, int64_t B, const ntm_unet_block &k,
                             float *ws, float *out, hipStream_t stream)
{
    UBlockArgs a = unet_block_args(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, k, out);
    const bool whole = ublock_whole(k);
    const size_t lds = unet_block_lds_bytes(a);
    if (lds > 64 * 1024)      // above the default limit of a launch: the CU has 160 KB
        if (hipError_t e = hipFuncSetAttribute((const void *)unet_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
            return e;
    const dim3 grid((unsigned)((k.T + a.tile - 1) / a.tile), (unsigned)B);
    const int64_t plane = B * k.c_out * k.T;
    int run = 0;
    for (int l = 0; l < k.n_layers; ++run) {
        a.l0 = l, a.l1 = whole ? k.n_layers : ublock_run_end(l, k.n_layers);
        a.y_in = run ? ws + ((run - 1) & 1) * plane : nullptr;
        a.y_out = ws ? ws + (run & 1) * plane : nullptr;
        hipLaunchKernelGGL(unet_block_kernel, grid, dim3(kUWaves * 64), lds, stream, a);
        if (hipError_t e = hipGetLastError()) return e;
        l = a.l1;
    }
    return hipSuccess;
}

// ---- resample + combine: a thread per output, the output itself in unet_steps.h ---------------------------------------------------
__global__ __launch_bounds__(256) void unet_down_kernel(UDownArgs a)
{
    const int j = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (j >= a.Fo) return;
    udown_one(a, blockIdx.z, c, j);
}

constexpr int kUpStage = 256 + 64;   // input frames under 256 outputs: 256 / S + 1 + taps - 1, taps <= 64

__global__ __launch_bounds__(256) void unet_up_kernel(UUpArgs a)
{
    __shared__ float pn[kUpStage];
    const int64_t n0 = (int64_t)blockIdx.x * 256, n = n0 + threadIdx.x, b = blockIdx.z;
    const int c = blockIdx.y;
    const bool pyramid = c == (int)gridDim.y - 1;
    const int j = (int)(n / a.S), ph = (int)(n - (int64_t)j * a.S);
    if (!pyramid) {                              // a channel of x (block-uniform)
        if (n >= a.Fo) return;
        uup_x_one(a, b, c, n, j, ph);
        return;
    }
    // the pyramid: the combined frames under this workgroup's outputs once, then the filter
    const int64_t nl = (n0 + 255 < a.Fo ? n0 + 255 : a.Fo - 1);
    const int jlo = (int)(n0 / a.S) - a.width, cnt = (int)(nl / a.S) - (int)(n0 / a.S) + 1 + (a.taps > 0 ? a.taps - 1 : 0);
    for (int t = threadIdx.x; t < cnt; t += 256) pn[t] = uup_combined(a, b, jlo + t);
    __syncthreads();
    if (n >= a.Fo) return;
    uup_pyr_one(a, b, n, ph, pn + (j - a.width - jlo));
}

hipError_t launch_unet_down(const float *x, const float *pyr, const float *ker, const float *wc, int64_t B, int C, int64_t F, int S,
                            int width, int taps, float *x_out, float *pyr_out, hipStream_t stream)
{
    UDownArgs a{x, pyr, ker, wc, x_out, pyr_out, C, (int)F, (int)((F + S - 1) / S), S, width, taps};
    hipLaunchKernelGGL(unet_down_kernel, dim3((unsigned)((a.Fo + 255) / 256), (unsigned)C, (unsigned)B), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_unet_up(const float *x, const float *pyr, int64_t pyr_T, const float *ker, const float *wc, int64_t B, int C,
                          int64_t F, int S, int width, int taps, float *x_out, float *pyr_out, hipStream_t stream)
{
    UUpArgs a{x, pyr, ker, wc, x_out, pyr_out, C, (int)F, S, width, taps, (int)pyr_T, (int64_t)S * F};
    const unsigned chans = (x_out ? (unsigned)C : 0u) + 1u;
    hipLaunchKernelGGL(unet_up_kernel, dim3((unsigned)((a.Fo + 255) / 256), chans, (unsigned)B), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---- the EDM step around the network ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edm_pre_kernel(EdmPreArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    edm_pre_one(a, i);
}

__global__ __launch_bounds__(256) void edm_post_kernel(const float *z, const float *F, float cskip, float cout, float b2, float k,
                                                       int64_t N, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    edm_post_one(z, F, cskip, cout, b2, k, i, out);
}

hipError_t launch_edm_pre(const float *z, const float *eps, float eps_scale, float snoise, const float *mask, int64_t mask_stride,
                          const float *x_out, const float *n, float sigma0, float cin, int64_t B, int64_t T, float *z_out,
                          float *net_in, hipStream_t stream)
{
    EdmPreArgs a{z, eps, mask, x_out, n, z_out, net_in, eps_scale, snoise, sigma0, cin, mask_stride, T, B * T};
    hipLaunchKernelGGL(edm_pre_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_edm_post(const float *z, const float *F, float cskip, float cout, float b2, float k, int64_t N, float *out,
                           hipStream_t stream)
{
    hipLaunchKernelGGL(edm_post_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, z, F, cskip, cout, b2, k, N, out);
    return hipGetLastError();
}

}  // namespace ntm
