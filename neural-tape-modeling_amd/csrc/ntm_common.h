// Shared device helpers for the libntm.so kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntm.h"

namespace ntm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kH = 64;  // hidden size of the matrix-pipe / low-latency kernels (NTM_HIDDEN); gru_small.hip: 8, 16, 32

// sigma(v) = 1/(1+e^-v) on v_exp_f32 / v_rcp_f32 (both ~1 ulp).  Saturates cleanly:
// e^-v -> inf gives 0, -> 0 gives 1.
__device__ __forceinline__ float sigmoid_f32(float v)
{
    const float e = __builtin_amdgcn_exp2f(v * -1.44269504088896340736f);
    return __builtin_amdgcn_rcpf(1.0f + e);
}

// tanh(v) = 1 - 2/(1+e^{2v}); abs error ~1e-7, exact limits +-1.
__device__ __forceinline__ float tanh_f32(float v)
{
    const float e = __builtin_amdgcn_exp2f(v * 2.88539008177792681472f);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + e);
}

// Kernel arguments of every GRU variant (pointers are device pointers, strides in elements).
struct GruArgs {
    const float *w_ih, *w_hh, *b_ih, *b_hh, *w_o, *b_o;  // b_o may be null
    const float *x;
    float *y;
    float *h_state;  // [B,64] in/out, may be null
    int64_t B, T, xs, ys;
    unsigned long long *dbg;  // diagnostic stamp sums (ntm_debug_gru_stamps), else null
    int abl;                  // diagnostic ablation mask (ntm_debug_gru_ablate), else 0
    int engine;               // MFMA2 GEMV engine: 0 exact fp32, 1 split-fp16 x3 (NTM_GRU_F16X3), 2 split-bf16 x3 x3 (NTM_GRU_BF16X3)
    // fused DiffDelRNN step (gru_mfma2_kernel<FUSE>): `y` above is then pre_d, and the delay line writes yd
    const float *dd = nullptr;      // delay trajectory [B,T] in samples, contiguous
    float *yd = nullptr;            // delayed output [B,T], contiguous
    const float *dl_buf = nullptr;  // carried delay buffer [B,D] (read only here; delay_update_kernel moves it on)
    int32_t *dl_flag = nullptr;     // sticky range-violation flag (may be null)
    int D = 0;
    int warmup = 0;
    // predict + loss leg in one launch (gru_mfma2_kernel<ESR>): per-stream sums of (tgt - y)^2 and tgt^2 over [esr_skip, T)
    const float *tgt = nullptr;     // target [B,T], contiguous
    double *esr_out = nullptr;      // [B,2] fp64
    int64_t esr_skip = 0;           // multiple of 4
    double *dcp_out = nullptr;      // gru_mfma2_kernel<ESR, DCP>: [B,2] fp64 DC-pre-emphasised sums (non-null selects DCP)
    float dcp_R = 0.995f;           // pole of the DC blocker
    int H = 64;                     // hidden size as the caller's tensors have it (gru_small.hip: any size but 64; the
                                    // matrix-pipe / low-latency kernels are compiled for kH)
    // R stacked replicas in one low-latency launch (gru_lat_kernel<HEADW, REP>, launch_gru_lat_replicas): streams per replica;
    // B = R * bper, stream s reads the parameters of replica s / bper from the [R, ...] stacks.  0: one model (nobody reads it)
    unsigned bper = 0;
};

}  // namespace ntm

namespace ntm {
// compute units of the current device (256 on MI355X); the launch heuristics count stream groups against it
inline int device_cus()
{
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
        return n;
    return 256;
}

hipError_t launch_gru_mfma(const GruArgs &a, hipStream_t stream);
hipError_t launch_gru_valu(const GruArgs &a, hipStream_t stream);
hipError_t launch_gru_mfma2(const GruArgs &a, hipStream_t stream);   // a.dd set: GRU + head + delay line in one launch
hipError_t launch_gru_lat(const GruArgs &a, hipStream_t stream);
hipError_t launch_gru_lat_replicas(const GruArgs &a, hipStream_t stream);   // a.bper > 0, a.B = R * a.bper, the parameters are stacks
hipError_t launch_gru_small(const GruArgs &a, int H, hipStream_t stream);   // any H in [1, 1024] but 64
hipError_t launch_gru_io(const GruArgs &a, int H, int I, int O, hipStream_t stream);   // any input_size / output_size (gru_small.hip)
// one block of the DiffDelRNN streamer (diffdel_stream.hip): the recurrence's arguments and the stream's ring
struct StreamArgs {
    GruArgs g;          // x / xs, y = the rows pre_d is written to (the caller's pre_d, else yd), ys (of y AND yd), h_state, B,
                        // T = block; dd = d, yd = the delayed output, D, warmup, dl_flag
    int64_t ds;         // row stride of d
    float *ring;        // [B, mask + 1]
    int64_t *pos;       // [B] samples written so far, counted from the ring's origin
    int64_t mask;       // C - 1, C a power of two >= D + block
};
hipError_t launch_diffdel_stream(const StreamArgs &sa, hipStream_t stream);
hipError_t launch_diffdel_stream_seed(const float *dl_state, float *ring, int64_t *pos, int64_t B, int D, int64_t C, hipStream_t stream);
hipError_t launch_diffdel_stream_export(const float *ring, const int64_t *pos, float *dl_state, int64_t B, int D, int64_t C,
                                        hipStream_t stream);
hipError_t launch_debug_transpose(const float *in, float *out, hipStream_t stream);
// training (gru_train.hip)
int64_t train_grad_floats();
// bper = 0: one model; bper > 0: R stacked replicas of bper streams each, stream s reads the parameters of replica s / bper
hipError_t launch_gru_train_fwd(const GruArgs &a, float *ws, int64_t bper, hipStream_t stream);
hipError_t launch_gru_train_bwd(const float *w_hh, const float *w_o, const float *x, int64_t xs, const float *ws, const float *dy,
                                int64_t dys, const float *dh_T, int64_t B, int64_t T, float *dh0, float *part, int64_t bper,
                                hipStream_t stream);
// the reduction and the loss adjoints: R models of bper streams each (one model: R = 1, bper = B)
hipError_t launch_gru_train_reduce_replicas(const float *part, int64_t R, int64_t bper, float *grad, hipStream_t stream);
hipError_t launch_esr_grad_replicas(const float *y, const float *t, int64_t R, int64_t N, const double *sums2, const float *gout,
                                    double eps, float *dy, hipStream_t stream);
hipError_t launch_esr_dcpre_grad_replicas(const float *y, const float *t, int64_t R, int64_t bper, int64_t T, float pole,
                                          const double *sums2, const float *gout, double eps, float *dy, hipStream_t stream);
hipError_t launch_loss_sums_replicas(const double *rows, int64_t R, int64_t bper, int splits, double *out, hipStream_t stream);
// the three critic conv stacks: the spectral critics (critic_kernels.hip), the dilated stack of the time-domain critic
// (convstack_kernels.hip) and the strided stack of the MelGAN critic (sconv_kernels.hip).  One record says where everything lies in
// `saved` and `ws`; each family's planner fills it from sizes ntm_api.hip has checked (the shared part and the kernels the families
// have in common: convstack_common.h)
constexpr int kStackMaxLayers = 16;   // include/ntm.h: n_layers in [1, 16] (the spectral family: [1, 8], checked by ntm_api.hip)
struct StackPlan {
    int n;
    int c_in[kStackMaxLayers], c_out[kStackMaxLayers], k[kStackMaxLayers], groups[kStackMaxLayers];
    int dil[kStackMaxLayers];                                                       // the dilated family, else 1
    int stride[kStackMaxLayers], pad[kStackMaxLayers], reflect[kStackMaxLayers];    // the strided family, else 1, 0, 0
    int64_t F[kStackMaxLayers + 1];           // frames entering layer l; F[n]: frames of the (last) output
    int64_t w_off[kStackMaxLayers], w_total;  // floats of layer l's weights within wF / wB
    int row0[kStackMaxLayers], rows;          // output channels counted through the layers
    int64_t act_off[kStackMaxLayers];         // saved: wF | wB | 1/|v| | outputs of layers 0 .. n-2 (the strided family: the
    int64_t saved_total;                      //        outputs are tensors of the caller's, `saved` ends after 1/|v|)
    int nchunk[kStackMaxLayers], per[kStackMaxLayers];    // weight gradient of layer l: chunks of `per` streams ...
    int64_t seg[kStackMaxLayers], nseg[kStackMaxLayers];  // ... times segments of `seg` output frames (the family's chunk rule)
    int64_t gz_size, fold_size;               // ws: gz ping | gz pong | padded gx of a reflected first layer | per layer the
    int64_t part_off[kStackMaxLayers], bpart_off[kStackMaxLayers], ws_total;   // partials of dW, then of dbias
    int cin_g(int l) const { return c_in[l] / groups[l]; }
    int cout_g(int l) const { return c_out[l] / groups[l]; }
    int64_t w_size(int l) const { return (int64_t)c_out[l] * cin_g(l) * k[l]; }
};
void crit_plan(StackPlan &p, int64_t B, int64_t C0, int64_t F0, int n, const ntm_conv1d_layer *L);
void convstack_plan(StackPlan &p, int64_t B, int64_t C0, int64_t F0, int n, const ntm_conv1d_layer_d *L);
void sconv_plan(StackPlan &p, int64_t B, int64_t C0, int64_t F0, int n, const ntm_conv1d_layer_s *L);
hipError_t launch_speccrit_forward(const StackPlan &p, const float *x, int64_t B, float log_floor, const float *const *g,
                                   const float *const *v, const float *const *bias, float *saved, float *out, hipStream_t stream);
hipError_t launch_speccrit_backward(const StackPlan &p, const float *x, int64_t B, float log_floor, const float *const *g,
                                    const float *const *v, const float *saved, const float *gout, float *gx, float *const *dg,
                                    float *const *dv, float *const *dbias, float *ws, hipStream_t stream);
hipError_t launch_convstack_forward(const StackPlan &p, const float *x, int64_t B, float slope, const float *const *g,
                                    const float *const *v, const float *const *bias, float *saved, float *out, hipStream_t stream);
hipError_t launch_convstack_backward(const StackPlan &p, const float *x, int64_t B, float slope, const float *const *g,
                                     const float *const *v, const float *saved, const float *gout, float *gx, float *const *dg,
                                     float *const *dv, float *const *dbias, float *ws, hipStream_t stream);
hipError_t launch_sconvstack_forward(const StackPlan &p, const float *x, int64_t B, float slope, const float *const *g,
                                     const float *const *v, const float *const *bias, float *saved, float *const *outs,
                                     hipStream_t stream);
hipError_t launch_sconvstack_backward(const StackPlan &p, const float *x, int64_t B, float slope, const float *const *g,
                                      const float *const *v, const float *saved, const float *const *outs,
                                      const float *const *gouts, float *gx, float *const *dg, float *const *dv,
                                      float *const *dbias, float *ws, hipStream_t stream);
// the hinge / mean heads of the adversarial losses (advhead_kernels.hip): the K outputs, their gradients (backward only) and sizes
struct AdvHeadArgs {
    const float *o[NTM_ADV_HEAD_MAX_K];
    float *g[NTM_ADV_HEAD_MAX_K];
    int64_t elems[NTM_ADV_HEAD_MAX_K];       // floats per row of output k
    int64_t rows, n_fake;
    int K, mode;
};
int64_t adv_head_chunks(const AdvHeadArgs &a);   // chunks of the longest half: the first grid dimension, the row length of ws
hipError_t launch_adv_head_forward(const AdvHeadArgs &a, double *ws, float *loss, hipStream_t stream);
hipError_t launch_adv_head_backward(const AdvHeadArgs &a, const float *gout, hipStream_t stream);
// the optimiser step over a list of tensors (multi_tensor.hip): one launch's table, passed by value.  ptr[j][k]: pointer j of
// tensor k (sqnorm: g; ema: dst, src; adam: p, g, m, v), n[k] > 0 its floats, first[k] its first workgroup, first[count] the grid
template <int NP>
struct MultiTable {
    void *ptr[NP][NTM_MULTI_MAX_TENSORS];
    int64_t n[NTM_MULTI_MAX_TENSORS];
    int32_t first[NTM_MULTI_MAX_TENSORS + 1];
    int32_t count;
};
struct MultiAdamScalars {
    float neg_step_size, bc2_sqrt, one_minus_beta1, beta2, one_minus_beta2, eps;
};
hipError_t launch_multi_sqnorm(const MultiTable<1> &t, double *partials, int64_t base, hipStream_t stream);
hipError_t launch_multi_norm_finalize(const double *partials, int64_t n, float max_norm, float *norm_coef, hipStream_t stream);
hipError_t launch_multi_adam(const MultiTable<4> &t, const float *norm_coef, const MultiAdamScalars &s, hipStream_t stream);
hipError_t launch_multi_ema(const MultiTable<2> &t, float s, float one_minus_s, hipStream_t stream);
// the batch feeder of the diffusion trainers (segment_feed.hip): the first bank sample of each row of one launch, passed by value
struct SegStarts {
    int64_t s[NTM_SEGMENT_MAX_ROWS];
};
hipError_t launch_segment_mean(const float *bank, const SegStarts &st, int rows, int64_t L, float *mean, hipStream_t stream);
hipError_t launch_segment_crop(const float *bank, const SegStarts &st, const float *mean, int rows, int64_t L, float *out,
                               hipStream_t stream);
hipError_t launch_segment_decimate(const float *bank, const SegStarts &st, const float *mean, int rows, int64_t L, const float *ker,
                                   int orig, int width, int taps, int64_t n_out, float *out, hipStream_t stream);
// the diffusion generators' network and sampler step (unet_kernels.hip); the sizes are checked by ntm_api.hip
int unet_block_launches(const ntm_unet_block &k);
int64_t unet_block_workspace(int64_t B, const ntm_unet_block &k);
hipError_t launch_unet_block(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                             const float *w_first, const float *w_gated, const float *w_res, int64_t B, const ntm_unet_block &k,
                             float *ws, float *out, hipStream_t stream);
hipError_t launch_unet_down(const float *x, const float *pyr, const float *ker, const float *wc, int64_t B, int C, int64_t F, int S,
                            int width, int taps, float *x_out, float *pyr_out, hipStream_t stream);
hipError_t launch_unet_up(const float *x, const float *pyr, int64_t pyr_T, const float *ker, const float *wc, int64_t B, int C,
                          int64_t F, int S, int width, int taps, float *x_out, float *pyr_out, hipStream_t stream);
hipError_t launch_edm_pre(const float *z, const float *eps, float eps_scale, float snoise, const float *mask, int64_t mask_stride,
                          const float *x_out, const float *n, float sigma0, float cin, int64_t B, int64_t T, float *z_out,
                          float *net_in, hipStream_t stream);
hipError_t launch_edm_post(const float *z, const float *F, float cskip, float cout, float b2, float k, int64_t N, float *out,
                           hipStream_t stream);
// that sampler in one launch (unet_sampler.hip): stages is the host copy ntm_api.hip has checked, stages_dev what the kernel walks
hipError_t launch_unet_sampler(const ntm_unet_stage *stages, const ntm_unet_stage *stages_dev, int n_stages, const float *scal,
                               const float *films, int64_t film_len, int n_steps, uint64_t eps_steps, const float *z0,
                               const float *draws, const float *x_outpaint, const float *mask, int64_t mask_stride, int64_t B,
                               int64_t T, float *ws, float *z, hipStream_t stream);
// the training of that network (unet_train.hip): the whole-form block with y_0 .. y_{n-1} saved, its adjoint, the reduction
int64_t unet_block_wgrad_floats(const ntm_unet_block &k);
int unet_block_partials(const ntm_unet_block &k);
hipError_t launch_unet_block_save(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                                  const float *w_first, const float *w_gated, const float *w_res, int64_t B, const ntm_unet_block &k,
                                  float *ysave, float *out, hipStream_t stream);
hipError_t launch_unet_block_backward(const float *src0, const float *src1, const float *init_w, const float *film,
                                      int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res, int64_t B,
                                      const ntm_unet_block &k, const float *ysave, const float *gout, float *ws, float *g_src0,
                                      float *g_src1, float *gfilm, float *part, hipStream_t stream);
hipError_t launch_unet_wgrad_reduce(const float *part, int64_t count, int64_t n, float *out, hipStream_t stream);
// the same in the tiled form, at any length: sizes in tiles, floats of workspace and partials (of wgrad_floats each)
int64_t unet_block_tiles(const ntm_unet_block &k);
int64_t unet_block_tiled_workspace(int64_t B, const ntm_unet_block &k);
int64_t unet_block_tiled_partials(int64_t B, const ntm_unet_block &k);
hipError_t launch_unet_block_tiled_save(const float *src0, const float *src1, const float *init_w, const float *film,
                                        int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res, int64_t B,
                                        const ntm_unet_block &k, float *ysave, float *out, hipStream_t stream);
hipError_t launch_unet_block_tiled_backward(const float *src0, const float *src1, const float *init_w, const float *film,
                                            int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res,
                                            int64_t B, const ntm_unet_block &k, const float *ysave, const float *gout, float *ws,
                                            float *g_src0, float *g_src1, float *gfilm, float *part, hipStream_t stream);
// the adjoints of the resample + combine steps (unet_resample_train.hip)
int64_t unet_up_backward_tiles(int64_t F);     // combiner-weight partials of one stream of ntm_unet_up_combine_backward
hipError_t launch_unet_down_backward(const float *pd, const float *ker, const float *wc, const float *g_xo, const float *g_po,
                                     int64_t B, int C, int64_t F, int S, int width, int taps, float *g_x, float *g_pyr, float *part,
                                     hipStream_t stream);
hipError_t launch_unet_up_backward(const float *x, const float *ker, const float *wc, const float *g_xo, const float *g_po, int64_t B,
                                   int C, int64_t F, int S, int width, int taps, int64_t pyr_T, float *g_x, float *g_pyr, float *part,
                                   hipStream_t stream);
hipError_t launch_delay_f64(const float *x, const double *d, float *y, int64_t B, int64_t T, float *dl_state, int D, int warmup,
                            int32_t *err_flag, hipStream_t stream);
hipError_t launch_delay_bwd(const float *gy, const float *d, const float *g_newbuf, float *gpre, float *gbuf, int64_t B, int64_t L,
                            int D, int warmup, int force_scan, hipStream_t stream);
}  // namespace ntm
