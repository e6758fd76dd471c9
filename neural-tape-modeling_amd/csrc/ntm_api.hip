// extern "C" surface of libntm.so (declared in include/ntm.h): argument checking, variant choice,
// error reporting.  No allocation, no synchronisation, no global mutable state besides the
// thread-local error string and the per-device pool of two side streams ntm_tcn_forward keeps for chunked batches.
#include "ntm.h"
#include "ntm_common.h"

#include <mutex>
#include <string>

namespace ntm {
hipError_t launch_delay(const float *x, const float *d, float *y, int64_t B, int64_t T, float *dl_state, int D,
                        int warmup, int32_t *err_flag, hipStream_t stream);
hipError_t launch_delay_apply(const float *x, const float *d, float *y, int64_t B, int64_t T, const float *dl_state, int D,
                              int warmup, int32_t *err_flag, hipStream_t stream);
hipError_t launch_delay_update(const float *x, int64_t B, int64_t T, float *dl_state, int D, const int32_t *err_flag,
                               hipStream_t stream);
hipError_t launch_esr(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int splits, double *out,
                      hipStream_t stream);
int esr_default_splits(int64_t B, int64_t T, int64_t skip);
hipError_t launch_loss_scalars(const double *rows, int64_t B, double n, double eps, double *out4, hipStream_t stream);
hipError_t launch_esr_dcpre(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, float R, double *out,
                            hipStream_t stream);
hipError_t launch_stft_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop,
                            int win, float eps, int chunks, int mode, double *out, hipStream_t stream, int n_mels = 0,
                            const int *mel_first = nullptr, const int *mel_start = nullptr, const float *mel_w = nullptr);
hipError_t launch_stft_grad(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop, int win,
                            float eps, const float *coef, float *ws, float *dy, int accumulate, hipStream_t stream);
hipError_t launch_spectrogram(const float *y, int64_t B, int64_t T, int n_fft, int hop, int win, float *P, hipStream_t stream);
hipError_t launch_spectrogram_grad(const float *y, const float *gP, int64_t B, int64_t T, int n_fft, int hop, int win, float *ws,
                                   float *dy, int accumulate, hipStream_t stream);
hipError_t launch_demodulate(const float *x, float *out, int C, int64_t N, const int64_t *y_idx, int P, int64_t period,
                             int64_t shift, double *scratch, hipStream_t stream);
hipError_t launch_tape_record_field(const double *I, const double *bias, double *H, int64_t B, int64_t N, double gain,
                                    double gap, hipStream_t stream);
hipError_t launch_tape_hmag(const double *H, double *M, int64_t B, int64_t N, double *state, double Ts, const double *par,
                            hipStream_t stream);
hipError_t launch_resample_fir(const double *x, double *y, int64_t B, int64_t N, int64_t M, int up, int down, int width,
                               const double *ker, hipStream_t stream);
hipError_t launch_fir_f64(const double *x, double *y, int64_t B, int64_t N, const double *h, int taps, int clamp, hipStream_t stream);
hipError_t launch_tcn(const float *params, int L, int C, int K, const int *dil, const float *x, float *y, int64_t B,
                      int64_t T, float *scratch, hipStream_t stream);
}  // namespace ntm

namespace {
thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char *where)
{
    return fail(NTM_EHIP, std::string(where) + ": " + hipGetErrorString(e));
}

// The size checks every entry point of a critic conv stack makes (ntm_speccrit, ntm_convstack, ntm_sconvstack).  Shared: sizes, n_layers, channel range, k, groups, chaining and, after
// the last layer, B * C * F < 2^31.  A family adds `params` (what it checks between k and groups: dilation; stride and pad) and
// `frames` (what it checks of the frames that reach the layer, and how the layer changes them).  spectral: the first layer
// reads the bins of the largest transform, so C0 and its c_in may be 1025; every other channel count is at most 1024.
template <class Layer, class Params, class Frames>
int stack_sizes(const std::string &w, int64_t B, int64_t C0, int64_t F0, int n_layers, const Layer *layers, int max_layers,
                bool spectral, Params params, Frames frames)
{
    if (B < 0 || C0 < 1 || F0 < 1) return fail(NTM_EINVAL, w + ": bad size");
    if (n_layers < 1 || n_layers > max_layers)
        return fail(NTM_EINVAL, w + ": n_layers must lie in [1, " + std::to_string(max_layers) + "]");
    if (!layers) return fail(NTM_EINVAL, w + ": null pointer");
    const int max_c0 = spectral ? 1025 : 1024;
    if (spectral && C0 > 1025) return fail(NTM_EINVAL, w + ": C0 must lie in [1, 1025] (the bins of the largest transform)");
    int64_t c = C0, F = F0;
    for (int l = 0; l < n_layers; ++l) {
        const Layer &y = layers[l];
        if (c > max_c0 || y.c_in < 1 || y.c_in > (l ? 1024 : max_c0) || y.c_out < 1 || y.c_out > 1024)
            return fail(NTM_EINVAL, w + ": channel counts must lie in [1, 1024]");
        if (y.k < 1 || y.k > 64) return fail(NTM_EINVAL, w + ": k must lie in [1, 64]");
        if (int rc = params(l, y, F)) return rc;
        if (y.groups < 1 || y.c_in % y.groups || y.c_out % y.groups) return fail(NTM_EINVAL, w + ": groups must divide both channel counts");
        if (y.c_in != c) return fail(NTM_EINVAL, w + ": c_in of a layer must be c_out of the layer before it (C0 for the first)");
        if (int rc = frames(l, y, c, F)) return rc;
        c = y.c_out;
    }
    if (B * c * F > 0x7fffffff) return fail(NTM_EINVAL, w + ": B * C * F must be below 2^31");
    return NTM_OK;
}
}  // namespace

extern "C" {

int ntm_abi_version(void) { return NTM_ABI_VERSION; }

const char *ntm_last_error(void) { return g_err.c_str(); }

int ntm_gru_forward_io(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                       const float *b_o, int H, int I, int O, const float *x, float *y, int64_t B, int64_t T,
                       int64_t x_stride_b, int64_t y_stride_b, float *h_state, void *stream)
{
    if (H < 1 || H > NTM_MAX_HIDDEN) return fail(NTM_EINVAL, "ntm_gru_forward_io: hidden size must lie in [1, 1024]");
    if (I < 1 || I > 1024 || O < 1 || O > 1024) return fail(NTM_EINVAL, "ntm_gru_forward_io: input_size and output_size must lie in [1, 1024]");
    if (B < 0 || T < 0) return fail(NTM_EINVAL, "ntm_gru_forward_io: negative B or T");
    if (B == 0 || T == 0) return NTM_OK;
    if (!w_ih || !w_hh || !b_ih || !b_hh || !w_o || !x || !y) return fail(NTM_EINVAL, "ntm_gru_forward_io: null pointer");
    if (x_stride_b < T * I || y_stride_b < T * O) return fail(NTM_EINVAL, "ntm_gru_forward_io: row stride below T * size");
    if (B > 0x7fffffff) return fail(NTM_EINVAL, "ntm_gru_forward_io: at most 2^31 - 1 streams per call");
    if (x == y) return fail(NTM_EINVAL, "ntm_gru_forward_io: y must not alias x");
    ntm::GruArgs a{w_ih, w_hh, b_ih, b_hh, w_o, b_o, x, y, h_state, B, T, x_stride_b, y_stride_b, nullptr, 0, 0};
    hipError_t e = ntm::launch_gru_io(a, H, I, O, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_gru_forward_io");
}

// How many of B streams the matrix-pipe kernel takes under NTM_GRU_AUTO (the low-latency kernel takes the rest): none up to
// NTM_GRU_LAT_MAX_B, otherwise all of them -- except when B is a whole number of full device rounds (16 streams x CUs) plus
// a remainder the low-latency kernel can take: the remainder goes there instead of opening another round of workgroups
// (B = 4112: 5.4 ms instead of 7.2 per 4096 steps)
static int64_t mfma2_streams(int64_t B)
{
    if (B <= NTM_GRU_LAT_MAX_B) return 0;
    const int64_t round = 16 * (int64_t)ntm::device_cus();
    const int64_t full = (B / round) * round, rem = B - full;
    return (full > 0 && rem > 0 && rem <= NTM_GRU_LAT_MAX_B) ? full : B;
}

// the per-stream loss sums a call forms beside its output: ESR sums of y against target over [skip, T); with dcp_out also the
// DC-pre-emphasised ones (pole R)
struct LossSums {
    const float *target;
    int64_t skip;
    double *esr_out;
    float R;
    double *dcp_out;
};

static int zero_sums(const LossSums &ls, int64_t B, const char *who, void *stream)      // no samples: the sums are zero
{
    hipError_t e = hipMemsetAsync(ls.esr_out, 0, (size_t)B * 2 * sizeof(double), (hipStream_t)stream);
    if (e == hipSuccess && ls.dcp_out) e = hipMemsetAsync(ls.dcp_out, 0, (size_t)B * 2 * sizeof(double), (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, who);
}

// the streaming passes (one row per stream) over rows [from, B) of contiguous y and target
static int loss_passes(const LossSums &ls, const float *y, int64_t from, int64_t B, int64_t T, const char *who, void *stream)
{
    const float *yr = y + from * T, *tr = ls.target + from * T;
    hipError_t e = ntm::launch_esr(yr, tr, B - from, T, ls.skip, 1, ls.esr_out + 2 * from, (hipStream_t)stream);
    if (e == hipSuccess && ls.dcp_out)
        e = ntm::launch_esr_dcpre(yr, tr, B - from, T, ls.skip, ls.R, ls.dcp_out + 2 * from, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, who);
}

// ntm_gru_forward[_ex] (ls == NULL) and ntm_gru_forward_esr / _losses share this body.  Every argument is checked BEFORE
// anything is enqueued: an NTM_EINVAL leaves y, h_state and the sums untouched.
static int gru_impl(const char *who, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                    const float *b_o, int H, const float *x, float *y, int64_t B, int64_t T, int64_t x_stride_b,
                    int64_t y_stride_b, float *h_state, int variant, const LossSums *ls, void *stream)
{
    const std::string w(who);
    if (H < 1 || H > NTM_MAX_HIDDEN) return fail(NTM_EINVAL, w + ": hidden size must lie in [1, 1024]");
    if (B < 0 || T < 0) return fail(NTM_EINVAL, w + ": negative B or T");
    if (ls && (ls->skip < 0 || ls->skip > T)) return fail(NTM_EINVAL, w + ": bad size");
    if (ls && ls->dcp_out && !(ls->R >= 0.0f && ls->R < 1.0f)) return fail(NTM_EINVAL, w + ": R must be in [0,1)");
    if (B == 0) return NTM_OK;
    if (ls && (!ls->target || !ls->esr_out)) return fail(NTM_EINVAL, w + ": null pointer");
    if (T == 0) return ls ? zero_sums(*ls, B, who, stream) : NTM_OK;
    if (!w_ih || !w_hh || !b_ih || !b_hh || !w_o || !x || !y) return fail(NTM_EINVAL, w + ": null pointer");
    if (x_stride_b < T || y_stride_b < T) return fail(NTM_EINVAL, w + ": stride < T");
    if (ls && ls->target == y) return fail(NTM_EINVAL, w + ": target must not alias y");
    if (H != NTM_HIDDEN) {
        // every other hidden size (the reference's constructor / training defaults 8 and 16, code/model.py:22,
        // code/train.py:50, and whatever --HIDDEN_SIZE a user trained with): gru_small.hip -- 64/HP streams per wavefront at
        // the next power of two HP for H < 64, a workgroup per stream above; the matrix-pipe variants exist for H = 64 only
        if (variant != NTM_GRU_AUTO && variant != NTM_GRU_LAT && variant != NTM_GRU_VALU)
            return fail(NTM_EINVAL, w + ": the matrix-pipe kernel variants are compiled for hidden size 64 only");
        if (H > NTM_HIDDEN && B > 0x7fffffff) return fail(NTM_EINVAL, w + ": at most 2^31 - 1 streams per call for H > 64");
    } else if (variant == NTM_GRU_VALU && (reinterpret_cast<uintptr_t>(w_hh) & 15))
        return fail(NTM_EINVAL, w + ": NTM_GRU_VALU reads W_hh with 16-byte loads; w_hh must be 16-byte aligned");
    // streams [0, m) take the matrix-pipe kernel under AUTO; the sums of streams [0, from) ride in that launch
    const int64_t m = (variant == NTM_GRU_AUTO && H == NTM_HIDDEN) ? mfma2_streams(B) : 0;
    const int64_t from = (ls && (ls->skip & 3) == 0) ? m : 0;
    if (ls && from < B && y_stride_b != T)
        return fail(NTM_EINVAL, w + ": the streaming loss passes (streams outside the matrix-pipe launch) need contiguous y rows (stride T)");
    ntm::GruArgs a{w_ih, w_hh, b_ih, b_hh, w_o, b_o, x, y, h_state, m, T, x_stride_b, y_stride_b, nullptr, 0, 0};
    hipError_t e = hipSuccess;
    if (m > 0) {
        if (from > 0) {
            a.tgt = ls->target;
            a.esr_out = ls->esr_out;
            a.esr_skip = ls->skip;
            a.dcp_out = ls->dcp_out;
            a.dcp_R = ls->R;
        }
        e = ntm::launch_gru_mfma2(a, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, who);
    }
    if (m < B) {        // the rest: the kernel `variant` names (under AUTO, the low-latency kernel)
        ntm::GruArgs r{w_ih, w_hh, b_ih, b_hh, w_o, b_o, x + m * x_stride_b, y + m * y_stride_b, h_state ? h_state + m * H : nullptr,
                       B - m, T, x_stride_b, y_stride_b, nullptr, 0, 0};
        if (H != NTM_HIDDEN) e = ntm::launch_gru_small(r, H, (hipStream_t)stream);
        else switch (variant) {
            case NTM_GRU_AUTO: case NTM_GRU_LAT: e = ntm::launch_gru_lat(r, (hipStream_t)stream); break;
            case NTM_GRU_MFMA2: e = ntm::launch_gru_mfma2(r, (hipStream_t)stream); break;
            case NTM_GRU_F16X3: r.engine = 1; e = ntm::launch_gru_mfma2(r, (hipStream_t)stream); break;
            case NTM_GRU_BF16X3: r.engine = 2; e = ntm::launch_gru_mfma2(r, (hipStream_t)stream); break;
            case NTM_GRU_MFMA: case NTM_GRU_VALU:
                return fail(NTM_EINVAL, w + ": laboratory kernel variant -- those live in libntm_lab.so "
                                            "(ntm_lab_gru_forward, include/ntm_lab.h), not in the product library");
            case NTM_GRU_MFMA3: case NTM_GRU_MFMA4:
                return fail(NTM_EINVAL, w + ": kernel variant retired in round 6 (a measured negative result)");
            default: return fail(NTM_EINVAL, w + ": unknown kernel variant");
        }
        if (e != hipSuccess) return hip_fail(e, who);
    }
    return ls && from < B ? loss_passes(*ls, y, from, B, T, who, stream) : NTM_OK;
}

int ntm_gru_forward_ex(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                       const float *b_o, int H, const float *x, float *y, int64_t B, int64_t T, int64_t x_stride_b,
                       int64_t y_stride_b, float *h_state, int variant, void *stream)
{
    return gru_impl("ntm_gru_forward", w_ih, w_hh, b_ih, b_hh, w_o, b_o, H, x, y, B, T, x_stride_b, y_stride_b, h_state, variant,
                    nullptr, stream);
}

int ntm_gru_forward(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                    const float *b_o, int H, const float *x, float *y, int64_t B, int64_t T, int64_t x_stride_b,
                    int64_t y_stride_b, float *h_state, void *stream)
{
    return gru_impl("ntm_gru_forward", w_ih, w_hh, b_ih, b_hh, w_o, b_o, H, x, y, B, T, x_stride_b, y_stride_b, h_state,
                    NTM_GRU_AUTO, nullptr, stream);
}

int ntm_gru_forward_esr(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                        const float *b_o, int H, const float *x, float *y, int64_t B, int64_t T, int64_t x_stride_b,
                        int64_t y_stride_b, float *h_state, const float *target, int64_t skip, double *esr_out, void *stream)
{
    const LossSums ls{target, skip, esr_out, 0.0f, nullptr};
    return gru_impl("ntm_gru_forward_esr", w_ih, w_hh, b_ih, b_hh, w_o, b_o, H, x, y, B, T, x_stride_b, y_stride_b, h_state,
                    NTM_GRU_AUTO, &ls, stream);
}

int ntm_gru_forward_losses(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                           const float *b_o, int H, const float *x, float *y, int64_t B, int64_t T, int64_t x_stride_b,
                           int64_t y_stride_b, float *h_state, const float *target, int64_t skip, double *esr_out, float dcpre_R,
                           double *dcpre_out, void *stream)
{
    if (!dcpre_out) return fail(NTM_EINVAL, "ntm_gru_forward_losses: null pointer");
    if (dcpre_out == esr_out) return fail(NTM_EINVAL, "ntm_gru_forward_losses: esr_out and dcpre_out must be distinct");
    const LossSums ls{target, skip, esr_out, dcpre_R, dcpre_out};
    return gru_impl("ntm_gru_forward_losses", w_ih, w_hh, b_ih, b_hh, w_o, b_o, H, x, y, B, T, x_stride_b, y_stride_b, h_state,
                    NTM_GRU_AUTO, &ls, stream);
}

int ntm_delay_forward(const float *x, const float *d, float *y, int64_t B, int64_t T, float *dl_state, int D,
                      int warmup, int32_t *err_flag, void *stream)
{
    if (B < 0 || T < 0 || D < 0) return fail(NTM_EINVAL, "ntm_delay_forward: negative size");
    if (B == 0 || T == 0) return NTM_OK;
    if (!x || !d || !y || (D > 0 && !dl_state)) return fail(NTM_EINVAL, "ntm_delay_forward: null pointer");
    if (x == y) return fail(NTM_EINVAL, "ntm_delay_forward: y must not alias x");
    hipError_t e = ntm::launch_delay(x, d, y, B, T, dl_state, D, warmup, err_flag, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_delay_forward");
}

int ntm_delay_forward_f64(const float *x, const double *d, float *y, int64_t B, int64_t T, float *dl_state, int D, int warmup,
                          int32_t *err_flag, void *stream)
{
    if (B < 0 || T < 0 || D < 0) return fail(NTM_EINVAL, "ntm_delay_forward_f64: negative size");
    if (B == 0 || T == 0) return NTM_OK;
    if (B > 65535) return fail(NTM_EINVAL, "ntm_delay_forward_f64: at most 65535 streams per call");
    if (!x || !d || !y || (D > 0 && !dl_state)) return fail(NTM_EINVAL, "ntm_delay_forward_f64: null pointer");
    if (x == y) return fail(NTM_EINVAL, "ntm_delay_forward_f64: y must not alias x");
    hipError_t e = ntm::launch_delay_f64(x, d, y, B, T, dl_state, D, warmup, err_flag, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_delay_forward_f64");
}

// the argument checks ntm_unet_resblock_workspace_floats and _forward share
static int unet_block_check(const std::string &w, int64_t B, const ntm_unet_block *k)
{
    if (!k) return fail(NTM_EINVAL, w + ": null pointer");
    if (B < 0 || B > 65535) return fail(NTM_EINVAL, w + ": B must lie in [0, 65535]");
    if (k->c0 < 1 || k->c1 < 0 || k->c0 + k->c1 > 32) return fail(NTM_EINVAL, w + ": input channels c0 + c1 must lie in [1, 32]");
    if (k->c_out < 1 || k->c_out > 16) return fail(NTM_EINVAL, w + ": c_out must lie in [1, 16]");
    if (k->n_layers < 1 || k->n_layers > 8) return fail(NTM_EINVAL, w + ": n_layers must lie in [1, 8]");
    if (k->T < 1) return fail(NTM_EINVAL, w + ": T must be positive");
    if (k->off0 < 0 || k->off0 + k->T > k->T0) return fail(NTM_EINVAL, w + ": src0 is shorter than off0 + T (or off0 < 0)");
    if (k->c1 > 0 && (k->off1 < 0 || k->off1 + k->T > k->T1)) return fail(NTM_EINVAL, w + ": src1 is shorter than off1 + T (or off1 < 0)");
    if (k->T0 > 0x7fffffff / 32 || (k->c1 > 0 && k->T1 > 0x7fffffff / 32)) return fail(NTM_EINVAL, w + ": 32 * frames must be below 2^31");
    if (k->form != NTM_UNET_AUTO && k->form != NTM_UNET_WHOLE && k->form != NTM_UNET_TILED) return fail(NTM_EINVAL, w + ": unknown form");
    if (k->form == NTM_UNET_WHOLE && k->T > NTM_UNET_WHOLE_MAX_T) return fail(NTM_EINVAL, w + ": the whole form takes T <= 1024");
    return NTM_OK;
}

int64_t ntm_unet_resblock_workspace_floats(int64_t B, const ntm_unet_block *blk)
{
    if (unet_block_check("ntm_unet_resblock_workspace_floats", B, blk) != NTM_OK) return -1;
    return ntm::unet_block_workspace(B, *blk);
}

int ntm_unet_resblock_forward(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                              const float *w_first, const float *w_gated, const float *w_res, int64_t B, const ntm_unet_block *blk,
                              float *ws, float *out, void *stream)
{
    const std::string w("ntm_unet_resblock_forward");
    if (int rc = unet_block_check(w, B, blk)) return rc;
    const int cin = blk->c0 + blk->c1;
    if (film_stride != 0 && film_stride < cin) return fail(NTM_EINVAL, w + ": film_stride must be 0 or at least c0 + c1");
    if (!w_res && cin != blk->c_out) return fail(NTM_EINVAL, w + ": an identity residual (w_res == NULL) needs c0 + c1 == c_out");
    if (B == 0) return NTM_OK;
    if (!src0 || !film || !w_first || !w_gated || !out || (blk->c1 > 0 && !src1) || (blk->init && !init_w))
        return fail(NTM_EINVAL, w + ": null pointer");
    if (ntm::unet_block_workspace(B, *blk) > 0 && !ws) return fail(NTM_EINVAL, w + ": null pointer (ws)");
    if (out == src0 || out == src1) return fail(NTM_EINVAL, w + ": out must not alias a source");
    hipError_t e = ntm::launch_unet_block(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, B, *blk, ws, out,
                                          (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_resblock_forward");
}

// the argument checks the training entry points of the block share: the forward's, and the whole form only -- or, for the
// ntm_unet_resblock_tiled_* family, the tiled form only: forced at any length, or what NTM_UNET_AUTO picks above 1024 frames
static int unet_train_check(const std::string &w, int64_t B, const ntm_unet_block *k, bool tiled = false)
{
    if (int rc = unet_block_check(w, B, k)) return rc;
    if (!tiled && (k->T > NTM_UNET_WHOLE_MAX_T || k->form == NTM_UNET_TILED))
        return fail(NTM_EINVAL, w + ": the whole form only, T <= 1024 (the tiled form: ntm_unet_resblock_tiled_*)");
    if (tiled && (k->form == NTM_UNET_WHOLE || (k->form == NTM_UNET_AUTO && k->T <= NTM_UNET_WHOLE_MAX_T)))
        return fail(NTM_EINVAL, w + ": the tiled form only, NTM_UNET_TILED or NTM_UNET_AUTO with T > 1024");
    if (tiled && B * ntm::unet_block_tiles(*k) > 0x7fffffff / 8) return fail(NTM_EINVAL, w + ": 8 B tiles must be below 2^31");
    return NTM_OK;
}

int64_t ntm_unet_resblock_save_floats(int64_t B, const ntm_unet_block *blk)
{
    if (unet_train_check("ntm_unet_resblock_save_floats", B, blk) != NTM_OK) return -1;
    return B * blk->n_layers * blk->c_out * blk->T;
}

int64_t ntm_unet_resblock_wgrad_floats(const ntm_unet_block *blk)
{
    if (unet_train_check("ntm_unet_resblock_wgrad_floats", 0, blk) != NTM_OK) return -1;
    return ntm::unet_block_wgrad_floats(*blk);
}

int64_t ntm_unet_resblock_partial_floats(int64_t B, const ntm_unet_block *blk)
{
    if (unet_train_check("ntm_unet_resblock_partial_floats", B, blk) != NTM_OK) return -1;
    return B * ntm::unet_block_partials(*blk) * ntm::unet_block_wgrad_floats(*blk);
}

// what _forward_save and _backward check of the forward's operands
static int unet_train_operands(const std::string &w, const float *src0, const float *src1, const float *init_w, const float *film,
                               int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res, int64_t B,
                               const ntm_unet_block *blk, bool tiled = false)
{
    if (int rc = unet_train_check(w, B, blk, tiled)) return rc;
    const int cin = blk->c0 + blk->c1;
    if (film_stride != 0 && film_stride < cin) return fail(NTM_EINVAL, w + ": film_stride must be 0 or at least c0 + c1");
    if (!w_res && cin != blk->c_out) return fail(NTM_EINVAL, w + ": an identity residual (w_res == NULL) needs c0 + c1 == c_out");
    if (B > 0 && (!src0 || !film || !w_first || !w_gated || (blk->c1 > 0 && !src1) || (blk->init && !init_w)))
        return fail(NTM_EINVAL, w + ": null pointer");
    return NTM_OK;
}

int ntm_unet_resblock_forward_save(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                                   const float *w_first, const float *w_gated, const float *w_res, int64_t B,
                                   const ntm_unet_block *blk, float *ysave, float *out, void *stream)
{
    const std::string w("ntm_unet_resblock_forward_save");
    if (int rc = unet_train_operands(w, src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, B, blk)) return rc;
    if (B == 0) return NTM_OK;
    if (!ysave || !out) return fail(NTM_EINVAL, w + ": null pointer");
    if (out == src0 || out == src1) return fail(NTM_EINVAL, w + ": out must not alias a source");
    hipError_t e = ntm::launch_unet_block_save(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, B, *blk, ysave, out,
                                               (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_resblock_forward_save");
}

int ntm_unet_resblock_backward(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                               const float *w_first, const float *w_gated, const float *w_res, int64_t B, const ntm_unet_block *blk,
                               const float *ysave, const float *gout, float *ws, float *g_src0, float *g_src1, float *gfilm,
                               float *partials, void *stream)
{
    const std::string w("ntm_unet_resblock_backward");
    if (int rc = unet_train_operands(w, src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, B, blk)) return rc;
    if (blk->init && g_src0) return fail(NTM_EINVAL, w + ": with init the waveform takes no gradient (g_src0 must be NULL)");
    if (blk->c1 == 0 && g_src1) return fail(NTM_EINVAL, w + ": g_src1 without a second source");
    if (B == 0) return NTM_OK;
    if (!ysave || !gout || !ws || !gfilm || !partials) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_unet_block_backward(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, B, *blk, ysave, gout,
                                                   ws, g_src0, g_src1, gfilm, partials, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_resblock_backward");
}

int64_t ntm_unet_resblock_tiled_save_floats(int64_t B, const ntm_unet_block *blk)
{
    if (unet_train_check("ntm_unet_resblock_tiled_save_floats", B, blk, true) != NTM_OK) return -1;
    return B * blk->n_layers * blk->c_out * blk->T;
}

int64_t ntm_unet_resblock_tiled_workspace_floats(int64_t B, const ntm_unet_block *blk)
{
    if (unet_train_check("ntm_unet_resblock_tiled_workspace_floats", B, blk, true) != NTM_OK) return -1;
    return ntm::unet_block_tiled_workspace(B, *blk);
}

int64_t ntm_unet_resblock_tiled_wgrad_floats(const ntm_unet_block *blk)
{
    if (unet_train_check("ntm_unet_resblock_tiled_wgrad_floats", 0, blk, true) != NTM_OK) return -1;
    return ntm::unet_block_wgrad_floats(*blk);
}

int64_t ntm_unet_resblock_tiled_partial_floats(int64_t B, const ntm_unet_block *blk)
{
    if (unet_train_check("ntm_unet_resblock_tiled_partial_floats", B, blk, true) != NTM_OK) return -1;
    return ntm::unet_block_tiled_partials(B, *blk) * ntm::unet_block_wgrad_floats(*blk);
}

int ntm_unet_resblock_tiled_forward_save(const float *src0, const float *src1, const float *init_w, const float *film,
                                         int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res,
                                         int64_t B, const ntm_unet_block *blk, float *ysave, float *out, void *stream)
{
    const std::string w("ntm_unet_resblock_tiled_forward_save");
    if (int rc = unet_train_operands(w, src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, B, blk, true)) return rc;
    if (B == 0) return NTM_OK;
    if (!ysave || !out) return fail(NTM_EINVAL, w + ": null pointer");
    if (out == src0 || out == src1) return fail(NTM_EINVAL, w + ": out must not alias a source");
    hipError_t e = ntm::launch_unet_block_tiled_save(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, B, *blk, ysave,
                                                     out, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_resblock_tiled_forward_save");
}

int ntm_unet_resblock_tiled_backward(const float *src0, const float *src1, const float *init_w, const float *film,
                                     int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res, int64_t B,
                                     const ntm_unet_block *blk, const float *ysave, const float *gout, float *ws, float *g_src0,
                                     float *g_src1, float *gfilm, float *partials, void *stream)
{
    const std::string w("ntm_unet_resblock_tiled_backward");
    if (int rc = unet_train_operands(w, src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, B, blk, true)) return rc;
    if (blk->init && g_src0) return fail(NTM_EINVAL, w + ": with init the waveform takes no gradient (g_src0 must be NULL)");
    if (blk->c1 == 0 && g_src1) return fail(NTM_EINVAL, w + ": g_src1 without a second source");
    if (B == 0) return NTM_OK;
    if (!ysave || !gout || !ws || !gfilm || !partials) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_unet_block_tiled_backward(src0, src1, init_w, film, film_stride, w_first, w_gated, w_res, B, *blk, ysave,
                                                         gout, ws, g_src0, g_src1, gfilm, partials, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_resblock_tiled_backward");
}

int ntm_unet_wgrad_reduce(const float *partials, int64_t count, int64_t n, float *out, void *stream)
{
    if (count < 0 || n < 0) return fail(NTM_EINVAL, "ntm_unet_wgrad_reduce: negative size");
    if (n / 256 > 0x7fffffff) return fail(NTM_EINVAL, "ntm_unet_wgrad_reduce: n must be below 2^39");
    if (n == 0) return NTM_OK;
    if (!out || (count > 0 && !partials)) return fail(NTM_EINVAL, "ntm_unet_wgrad_reduce: null pointer");
    hipError_t e = ntm::launch_unet_wgrad_reduce(partials, count, n, out, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_wgrad_reduce");
}

// the size checks of the three resampling entry points
static int unet_resample_check(const std::string &w, int64_t B, int C, int64_t F, int S, int width, int taps, int64_t Fo)
{
    if (B < 0 || B > 65535) return fail(NTM_EINVAL, w + ": B must lie in [0, 65535]");
    if (C < 1 || C > 32) return fail(NTM_EINVAL, w + ": C must lie in [1, 32]");
    if (F < 1) return fail(NTM_EINVAL, w + ": F must be positive");
    if (S < 1 || S > 1024) return fail(NTM_EINVAL, w + ": S must lie in [1, 1024]");
    if (width < 0 || taps < 0 || taps > 64) return fail(NTM_EINVAL, w + ": width must not be negative, taps at most 64");
    if (F > 0x7fffffff / 2 || Fo > 0x7fffffff / C) return fail(NTM_EINVAL, w + ": C * frames must be below 2^31");
    return NTM_OK;
}

int ntm_unet_down_combine(const float *x, const float *pyr, const float *ker, const float *wc, int64_t B, int C, int64_t F, int S,
                          int width, int taps, float *x_out, float *pyr_out, void *stream)
{
    const std::string w("ntm_unet_down_combine");
    if (int rc = unet_resample_check(w, B, C, F, S, width, taps, F)) return rc;
    if (taps != 2 * width + S) return fail(NTM_EINVAL, w + ": taps must be 2 * width + S");
    if (B == 0) return NTM_OK;
    if (!x || !pyr || !ker || !wc || !x_out || !pyr_out) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_unet_down(x, pyr, ker, wc, B, C, F, S, width, taps, x_out, pyr_out, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_down_combine");
}

int ntm_unet_up_combine(const float *x, const float *pyr, int64_t pyr_T, const float *ker, const float *wc, int64_t B, int C,
                        int64_t F, int S, int width, int taps, float *x_out, float *pyr_out, void *stream)
{
    const std::string w("ntm_unet_up_combine");
    if (int rc = unet_resample_check(w, B, C, F, S, width, taps, (int64_t)S * F)) return rc;
    if (S == 1 ? (taps != 0 || width != 0) : taps != 2 * width + 1)
        return fail(NTM_EINVAL, w + ": taps must be 2 * width + 1 (S == 1: no filter, width == taps == 0)");
    if (pyr && pyr_T < F) return fail(NTM_EINVAL, w + ": the pyramid is shorter than F");
    if (B == 0) return NTM_OK;
    if (!x || !wc || !pyr_out || (S > 1 && (!ker || !x_out))) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_unet_up(x, pyr, pyr_T, ker, wc, B, C, F, S, width, taps, S > 1 ? x_out : nullptr, pyr_out,
                                       (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_up_combine");
}

int ntm_unet_upsample(const float *x, const float *ker, int64_t B, int64_t F, int S, int width, int taps, float *out, void *stream)
{
    const std::string w("ntm_unet_upsample");
    if (int rc = unet_resample_check(w, B, 1, F, S, width, taps, (int64_t)S * F)) return rc;
    if (S < 2 || taps != 2 * width + 1) return fail(NTM_EINVAL, w + ": S must be at least 2 and taps 2 * width + 1");
    if (B == 0) return NTM_OK;
    if (!x || !ker || !out) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_unet_up(x, nullptr, 0, ker, nullptr, B, 1, F, S, width, taps, nullptr, out, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_upsample");
}

int ntm_unet_down_combine_backward(const float *pyr_d, const float *ker, const float *wc, const float *g_xo, const float *g_po,
                                   int64_t B, int C, int64_t F, int S, int width, int taps, float *g_x, float *g_pyr, float *partials,
                                   void *stream)
{
    const std::string w("ntm_unet_down_combine_backward");
    if (int rc = unet_resample_check(w, B, C, F, S, width, taps, F)) return rc;
    if (taps != 2 * width + S) return fail(NTM_EINVAL, w + ": taps must be 2 * width + S");
    if (B == 0) return NTM_OK;
    if (!g_xo && !g_po) return fail(NTM_EINVAL, w + ": g_xo and g_po are both null: no gradient to take");
    if (!g_x && !g_pyr && !partials) return fail(NTM_EINVAL, w + ": g_x, g_pyr and partials are all null: nothing to write");
    if (!ker || !wc || (partials && !pyr_d)) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_unet_down_backward(pyr_d, ker, wc, g_xo, g_po, B, C, F, S, width, taps, g_x, g_pyr, partials,
                                                  (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_down_combine_backward");
}

int64_t ntm_unet_up_combine_backward_partials(int64_t F)
{
    if (F < 1 || F > 0x7fffffff / 2) {
        fail(NTM_EINVAL, "ntm_unet_up_combine_backward_partials: F must lie in [1, 2^30)");
        return -1;
    }
    return ntm::unet_up_backward_tiles(F);
}

int ntm_unet_up_combine_backward(const float *x, const float *ker, const float *wc, const float *g_xo, const float *g_po, int64_t B,
                                 int C, int64_t F, int S, int width, int taps, int64_t pyr_T, float *g_x, float *g_pyr,
                                 float *partials, void *stream)
{
    const std::string w("ntm_unet_up_combine_backward");
    if (int rc = unet_resample_check(w, B, C, F, S, width, taps, (int64_t)S * F)) return rc;
    if (S == 1 ? (taps != 0 || width != 0) : taps != 2 * width + 1)
        return fail(NTM_EINVAL, w + ": taps must be 2 * width + 1 (S == 1: no filter, width == taps == 0)");
    if (pyr_T != 0 && pyr_T < F) return fail(NTM_EINVAL, w + ": the pyramid is shorter than F (pyr_T == 0: no pyramid)");
    if (pyr_T > 0x7fffffff) return fail(NTM_EINVAL, w + ": pyr_T must be below 2^31");
    if (S == 1 && (ker || g_xo)) return fail(NTM_EINVAL, w + ": S == 1 is the combiner alone: ker and g_xo must be NULL");
    if (pyr_T == 0 && g_pyr) return fail(NTM_EINVAL, w + ": g_pyr without a pyramid (pyr_T == 0)");
    if (B == 0) return NTM_OK;
    if (!g_xo && !g_po) return fail(NTM_EINVAL, w + ": g_xo and g_po are both null: no gradient to take");
    if (!g_x && !g_pyr && !partials) return fail(NTM_EINVAL, w + ": g_x, g_pyr and partials are all null: nothing to write");
    if (!wc || (S > 1 && !ker) || (partials && !x)) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_unet_up_backward(x, ker, wc, g_xo, g_po, B, C, F, S, width, taps, pyr_T, g_x, g_pyr, partials,
                                                (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_up_combine_backward");
}

int ntm_edm_pre(const float *z, const float *eps, float eps_scale, float snoise, const float *mask, int64_t mask_stride,
                const float *x_out, const float *n, float sigma0, float cin, int64_t B, int64_t T, float *z_out, float *net_in,
                void *stream)
{
    if (B < 0 || T < 0) return fail(NTM_EINVAL, "ntm_edm_pre: negative size");
    if (mask && mask_stride != 0 && mask_stride != T) return fail(NTM_EINVAL, "ntm_edm_pre: mask_stride must be 0 or T");
    if (mask && (!x_out || !n)) return fail(NTM_EINVAL, "ntm_edm_pre: null pointer (a mask comes with x_out and n)");
    if (B == 0 || T == 0) return NTM_OK;
    if (!z || !z_out || !net_in) return fail(NTM_EINVAL, "ntm_edm_pre: null pointer");
    if (B * T / 256 > 0x7fffffff) return fail(NTM_EINVAL, "ntm_edm_pre: B * T must be below 2^39");
    hipError_t e = ntm::launch_edm_pre(z, eps, eps_scale, snoise, mask, mask_stride, x_out, n, sigma0, cin, B, T, z_out, net_in,
                                       (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_edm_pre");
}

int ntm_edm_post(const float *z, const float *F, float cskip, float cout, float b2, float k, int64_t N, float *out, void *stream)
{
    if (N < 0) return fail(NTM_EINVAL, "ntm_edm_post: negative size");
    if (N == 0) return NTM_OK;
    if (!z || !F || !out) return fail(NTM_EINVAL, "ntm_edm_post: null pointer");
    if (N / 256 > 0x7fffffff) return fail(NTM_EINVAL, "ntm_edm_post: N must be below 2^39");
    hipError_t e = ntm::launch_edm_post(z, F, cskip, cout, b2, k, N, out, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_edm_post");
}

// the size checks ntm_unet_sample_workspace_floats and _one_launch share
static int unet_sample_sizes(const std::string &w, int64_t B, int64_t T)
{
    if (B < 0 || B > 65535) return fail(NTM_EINVAL, w + ": B must lie in [0, 65535]");
    if (T < 1 || T > NTM_UNET_WHOLE_MAX_T) return fail(NTM_EINVAL, w + ": T must lie in [1, 1024]");
    return NTM_OK;
}

int64_t ntm_unet_sample_workspace_floats(int64_t B, int64_t T)
{
    if (unet_sample_sizes("ntm_unet_sample_workspace_floats", B, T) != NTM_OK) return -1;
    return 3 * B * T;
}

// one record of the stage table against the caps the kernel's loops rely on: what the stage's own entry point checks, the whole
// form, and the null pointers that stand for the network's input and output
static int unet_stage_check(const std::string &w, const ntm_unet_stage &st, int64_t B, int64_t T, int64_t film_len)
{
    if (st.kind == NTM_USTAGE_BLOCK) {
        const ntm_unet_block &k = st.blk;
        if (int rc = unet_block_check(w, B, &k)) return rc;
        if (k.form == NTM_UNET_TILED || k.T > NTM_UNET_WHOLE_MAX_T)
            return fail(NTM_EINVAL, w + ": a block of " + std::to_string(k.T) + " frames: the whole form only, T <= 1024");
        const int cin = k.c0 + k.c1;
        if (st.film_off < 0 || st.film_off + cin > film_len) return fail(NTM_EINVAL, w + ": film_off + c0 + c1 must lie within film_len");
        if (!st.w2 && cin != k.c_out) return fail(NTM_EINVAL, w + ": an identity residual (w2 == NULL) needs c0 + c1 == c_out");
        if (!st.a && !(k.init && k.T0 == T)) return fail(NTM_EINVAL, w + ": a == NULL (the network's input) needs blk.init and blk.T0 == T");
        if (!st.w0 || !st.w1 || !st.o0 || (k.c1 > 0 && !st.b) || (k.init && !st.w3)) return fail(NTM_EINVAL, w + ": null pointer (block stage)");
        if (st.o0 == st.a || st.o0 == st.b) return fail(NTM_EINVAL, w + ": a block's out must not alias a source");
        return NTM_OK;
    }
    if (st.kind == NTM_USTAGE_DOWN) {
        if (int rc = unet_resample_check(w, B, st.C, st.F, st.S, st.width, st.taps, st.F)) return rc;
        if (st.taps != 2 * st.width + st.S) return fail(NTM_EINVAL, w + ": taps must be 2 * width + S (down stage)");
        if (st.F > NTM_UNET_WHOLE_MAX_T) return fail(NTM_EINVAL, w + ": a down stage takes F <= 1024");
        if (!st.b && st.F != T) return fail(NTM_EINVAL, w + ": b == NULL (the network's input) needs F == T");
        if (!st.a || !st.w0 || !st.w1 || !st.o0 || !st.o1) return fail(NTM_EINVAL, w + ": null pointer (down stage)");
        return NTM_OK;
    }
    if (st.kind == NTM_USTAGE_UP || st.kind == NTM_USTAGE_FINAL) {
        const bool fin = st.kind == NTM_USTAGE_FINAL;
        if (int rc = unet_resample_check(w, B, st.C, st.F, st.S, st.width, st.taps, (int64_t)st.S * st.F)) return rc;
        if (fin ? (st.S != 1 || st.taps != 0 || st.width != 0) : (st.S < 2 || st.taps != 2 * st.width + 1))
            return fail(NTM_EINVAL, w + ": an up stage has S >= 2 and taps == 2 * width + 1, the final one S == 1 and no filter");
        if (st.F > NTM_UNET_WHOLE_MAX_T || (int64_t)st.S * st.F > 2 * NTM_UNET_WHOLE_MAX_T)
            return fail(NTM_EINVAL, w + ": an up stage takes F <= 1024 and S F <= 2048");
        if (st.b && st.pyr_T < st.F) return fail(NTM_EINVAL, w + ": the pyramid is shorter than F");
        if (st.b && st.pyr_T > 0x7fffffff) return fail(NTM_EINVAL, w + ": pyr_T must be below 2^31");
        if (!st.a || !st.w1 || (!fin && (!st.w0 || !st.o0 || !st.o1))) return fail(NTM_EINVAL, w + ": null pointer (up stage)");
        if (fin && !st.o1 && st.F != T) return fail(NTM_EINVAL, w + ": o1 == NULL (the network's output) needs F == T");
        return NTM_OK;
    }
    return fail(NTM_EINVAL, w + ": unknown stage kind " + std::to_string(st.kind));
}

int ntm_unet_sample_one_launch(const ntm_unet_stage *stages, const ntm_unet_stage *stages_dev, int n_stages, const float *scal,
                               const float *films, int64_t film_len, int n_steps, uint64_t eps_steps, const float *z0,
                               const float *draws, int n_draws, const float *x_outpaint, const float *mask, int64_t mask_stride,
                               int64_t B, int64_t T, float *ws, float *z, void *stream)
{
    const std::string w("ntm_unet_sample_one_launch");
    if (int rc = unet_sample_sizes(w, B, T)) return rc;
    if (n_stages < 1 || n_stages > NTM_UNET_SAMPLE_MAX_STAGES) return fail(NTM_EINVAL, w + ": n_stages must lie in [1, 64]");
    if (n_steps < 1 || n_steps > NTM_UNET_SAMPLE_MAX_STEPS) return fail(NTM_EINVAL, w + ": n_steps must lie in [1, 64]");
    if (film_len < 1 || film_len > 0x7fffffff / NTM_UNET_SAMPLE_MAX_STEPS) return fail(NTM_EINVAL, w + ": film_len must lie in [1, 2^25)");
    if (!stages) return fail(NTM_EINVAL, w + ": null pointer (stages)");
    for (int q = 0; q < n_stages; ++q)
        if (int rc = unet_stage_check(w + ", stage " + std::to_string(q), stages[q], B, T, film_len)) return rc;
    if (mask && mask_stride != 0 && mask_stride != T) return fail(NTM_EINVAL, w + ": mask_stride must be 0 or T");
    if (mask ? !x_outpaint : x_outpaint != nullptr) return fail(NTM_EINVAL, w + ": mask and x_outpaint come together");
    int want = mask ? n_steps : 0;
    for (int i = 0; i < n_steps; ++i) want += (int)((eps_steps >> i) & 1);
    if (n_draws != want) return fail(NTM_EINVAL, w + ": n_draws must be " + std::to_string(want) + " (an eps draw per step of eps_steps, "
                                                     "an outpainting draw per step with a mask)");
    if (B == 0) return NTM_OK;
    if (!stages_dev || !scal || !films || !z0 || !ws || !z || (n_draws > 0 && !draws)) return fail(NTM_EINVAL, w + ": null pointer");
    if (z == z0 || z == draws || z == x_outpaint || z == mask || z == ws) return fail(NTM_EINVAL, w + ": z must not alias an input or ws");
    hipError_t e = ntm::launch_unet_sampler(stages, stages_dev, n_stages, scal, films, film_len, n_steps, eps_steps, z0, draws,
                                            x_outpaint, mask, mask_stride, B, T, ws, z, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_unet_sample_one_launch");
}

// ntm_diffdel_gru_forward[_ex] (ls == NULL) and ntm_diffdel_gru_forward_esr / _losses share this body
static int diffdel_impl(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o, int H,
                        const float *x, const float *d, float *y, float *pre_d, int64_t B, int64_t T, float *h_state,
                        float *dl_state, int D, int warmup, int32_t *err_flag, int mode, const LossSums *ls, void *stream)
{
    const char *who = ls ? "ntm_diffdel_gru_forward_esr" : "ntm_diffdel_gru_forward";
    // every argument is checked BEFORE anything is enqueued: an NTM_EINVAL leaves y, pre_d, the states and the sums untouched
    if (B < 0 || T < 0 || D < 0) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward: negative size");
    if (H < 1 || H > NTM_MAX_HIDDEN) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward: hidden size must lie in [1, 1024]");
    if (B == 0) return NTM_OK;
    if (!pre_d || pre_d == y) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward: pre_d must be a distinct buffer");
    if (mode != NTM_DIFFDEL_AUTO && mode != NTM_DIFFDEL_TWO_PASS && mode != NTM_DIFFDEL_FUSED)
        return fail(NTM_EINVAL, "ntm_diffdel_gru_forward: unknown mode");
    if (mode == NTM_DIFFDEL_FUSED && H != NTM_HIDDEN)
        return fail(NTM_EINVAL, "ntm_diffdel_gru_forward: the fused kernel is compiled for hidden size 64 only");
    constexpr int64_t kFusedMaxT = (int64_t)1 << 26;     // the fused kernel addresses a 16-row block with 32-bit byte offsets
    if (mode == NTM_DIFFDEL_FUSED && T >= kFusedMaxT)
        return fail(NTM_EINVAL, "ntm_diffdel_gru_forward: the fused kernel takes T < 2^26 samples per call");
    if (T == 0) return ls ? zero_sums(*ls, B, who, stream) : NTM_OK;
    if (!w_ih || !w_hh || !b_ih || !b_hh || !w_o || !x || !d || !y || (D > 0 && !dl_state))
        return fail(NTM_EINVAL, "ntm_diffdel_gru_forward: null pointer");
    // how many streams take the fused matrix-pipe kernel: all of them when forced; under AUTO the streams ntm_gru_forward
    // would give to that kernel (the rest: the low-latency kernel + the streaming delay pass, as there).  A warm-up call
    // (code/model.py:288-292: the delay line only moves its buffer on, y = pre_d) takes the two-pass form in every mode: the
    // fused kernel's delay stage is idle then and reads no delays, while the reference evaluates its range assert BEFORE the
    // warm-up branch (code/model.py:284 vs :288) -- delay_apply_kernel does, in warm-up too.
    const int64_t fused = warmup ? 0
                        : mode == NTM_DIFFDEL_FUSED ? B
                        : (mode == NTM_DIFFDEL_AUTO && H == NTM_HIDDEN && T < kFusedMaxT) ? mfma2_streams(B) : 0;
    // the sums ride in the fused launch where skip is a multiple of 4; the streaming passes form them everywhere else
    const int64_t from = (ls && (ls->skip & 3) == 0) ? fused : 0;
    if (fused > 0) {
        if (x == y || x == pre_d || d == y || d == pre_d)
            return fail(NTM_EINVAL, "ntm_diffdel_gru_forward: outputs must not alias x or d");
        ntm::GruArgs a{w_ih, w_hh, b_ih, b_hh, w_o, nullptr, x, pre_d, h_state, fused, T, T, T, nullptr, 0, 0};
        a.dd = d;
        a.yd = y;
        a.dl_buf = dl_state;
        a.dl_flag = err_flag;
        a.D = D;
        if (from > 0) {
            a.tgt = ls->target;
            a.esr_out = ls->esr_out;
            a.esr_skip = ls->skip;
            a.dcp_out = ls->dcp_out;
            a.dcp_R = ls->R;
        }
        hipError_t e = ntm::launch_gru_mfma2(a, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "ntm_diffdel_gru_forward");
    }
    if (fused < B) {            // the streams the fused kernel did not take: GRU launch, then the streaming delay pass
        const int64_t r = B - fused, o = fused * T;
        // (a warm-up call under NTM_DIFFDEL_FUSED keeps the matrix-pipe GRU kernel the fused launch would have run, so that
        // the state a forced mode leaves behind does not depend on which calls were warm-ups)
        const int gv = (warmup && mode == NTM_DIFFDEL_FUSED) ? NTM_GRU_MFMA2 : NTM_GRU_AUTO;
        int rc = ntm_gru_forward_ex(w_ih, w_hh, b_ih, b_hh, w_o, nullptr, H, x + o, pre_d + o, r, T, T, T,
                                    h_state ? h_state + fused * H : nullptr, gv, stream);
        if (rc != NTM_OK) return rc;
        if (fused == 0) {
            rc = ntm_delay_forward(pre_d, d, y, B, T, dl_state, D, warmup, err_flag, stream);
            if (rc != NTM_OK) return rc;
        } else {    // mixed: interpolate the remainder here; the ONE buffer update below reads the flag both parts raise
            hipError_t e = ntm::launch_delay_apply(pre_d + o, d + o, y + o, r, T, dl_state ? dl_state + fused * D : nullptr, D,
                                                   warmup, err_flag, (hipStream_t)stream);
            if (e != hipSuccess) return hip_fail(e, "ntm_diffdel_gru_forward");
        }
    }
    if (fused > 0) {
        hipError_t e = ntm::launch_delay_update(pre_d, B, T, dl_state, D, err_flag, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "ntm_diffdel_gru_forward");
    }
    return ls && from < B ? loss_passes(*ls, y, from, B, T, who, stream) : NTM_OK;
}

int ntm_diffdel_gru_forward_ex(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                               const float *w_o, int H, const float *x, const float *d, float *y, float *pre_d,
                               int64_t B, int64_t T, float *h_state, float *dl_state, int D, int warmup,
                               int32_t *err_flag, int mode, void *stream)
{
    return diffdel_impl(w_ih, w_hh, b_ih, b_hh, w_o, H, x, d, y, pre_d, B, T, h_state, dl_state, D, warmup, err_flag, mode, nullptr,
                        stream);
}

int ntm_diffdel_gru_forward_esr(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                const float *w_o, int H, const float *x, const float *d, float *y, float *pre_d,
                                int64_t B, int64_t T, float *h_state, float *dl_state, int D, int32_t *err_flag,
                                const float *target, int64_t skip, double *esr_out, void *stream)
{
    if (!target || !esr_out) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward_esr: null pointer");
    if (skip < 0 || skip > T) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward_esr: bad skip");
    if (target == y || target == pre_d) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward_esr: target must not alias an output");
    const LossSums ls{target, skip, esr_out, 0.0f, nullptr};
    return diffdel_impl(w_ih, w_hh, b_ih, b_hh, w_o, H, x, d, y, pre_d, B, T, h_state, dl_state, D, 0, err_flag, NTM_DIFFDEL_AUTO, &ls,
                        stream);
}

int ntm_diffdel_gru_forward_losses(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                   const float *w_o, int H, const float *x, const float *d, float *y, float *pre_d,
                                   int64_t B, int64_t T, float *h_state, float *dl_state, int D, int32_t *err_flag,
                                   const float *target, int64_t skip, double *esr_out, float dcpre_R, double *dcpre_out, void *stream)
{
    if (!target || !esr_out || !dcpre_out) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward_losses: null pointer");
    if (dcpre_out == esr_out) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward_losses: esr_out and dcpre_out must be distinct");
    if (!(dcpre_R >= 0.0f && dcpre_R < 1.0f)) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward_losses: R must be in [0,1)");
    if (skip < 0 || skip > T) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward_losses: bad skip");
    if (target == y || target == pre_d) return fail(NTM_EINVAL, "ntm_diffdel_gru_forward_losses: target must not alias an output");
    const LossSums ls{target, skip, esr_out, dcpre_R, dcpre_out};
    return diffdel_impl(w_ih, w_hh, b_ih, b_hh, w_o, H, x, d, y, pre_d, B, T, h_state, dl_state, D, 0, err_flag, NTM_DIFFDEL_AUTO, &ls,
                        stream);
}

int ntm_diffdel_gru_forward(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                            const float *w_o, int H, const float *x, const float *d, float *y, float *pre_d,
                            int64_t B, int64_t T, float *h_state, float *dl_state, int D, int warmup,
                            int32_t *err_flag, void *stream)
{
    return ntm_diffdel_gru_forward_ex(w_ih, w_hh, b_ih, b_hh, w_o, H, x, d, y, pre_d, B, T, h_state, dl_state, D, warmup,
                                      err_flag, NTM_DIFFDEL_AUTO, stream);
}

int ntm_esr_splits(int64_t B, int64_t T, int64_t skip) { return ntm::esr_default_splits(B, T, skip); }

int ntm_esr_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int splits, double *out, void *stream)
{
    if (B < 0 || T < 0 || skip < 0 || skip > T) return fail(NTM_EINVAL, "ntm_esr_sums: bad size");
    if (splits < 1 || splits > 65535) return fail(NTM_EINVAL, "ntm_esr_sums: splits must be in [1, 65535]");
    if (B == 0) return NTM_OK;
    if (!y || !t || !out) return fail(NTM_EINVAL, "ntm_esr_sums: null pointer");
    hipError_t e = ntm::launch_esr(y, t, B, T, skip, splits, out, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_esr_sums");
}

int ntm_loss_scalars(const double *esr_rows, int64_t B, int64_t n_samples, double eps, double *out4, void *stream)
{
    if (B < 0 || n_samples <= 0 || !(eps >= 0.0)) return fail(NTM_EINVAL, "ntm_loss_scalars: bad size or eps");
    if (!out4 || (B > 0 && !esr_rows)) return fail(NTM_EINVAL, "ntm_loss_scalars: null pointer");
    hipError_t e = ntm::launch_loss_scalars(esr_rows, B, (double)n_samples, eps, out4, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_loss_scalars");
}

int ntm_esr_dcpre_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, float R, double *out,
                       void *stream)
{
    if (B < 0 || T < 0 || skip < 0 || skip > T) return fail(NTM_EINVAL, "ntm_esr_dcpre_sums: bad size");
    if (!(R >= 0.0f && R < 1.0f)) return fail(NTM_EINVAL, "ntm_esr_dcpre_sums: R must be in [0,1)");
    if (B == 0) return NTM_OK;
    if (!y || !t || !out) return fail(NTM_EINVAL, "ntm_esr_dcpre_sums: null pointer");
    hipError_t e = ntm::launch_esr_dcpre(y, t, B, T, skip, R, out, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_esr_dcpre_sums");
}

static int stft_common(const char *who, const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop,
                       int win_length, float floor_, int chunks, int mode, double *out, void *stream, int n_mels = 0,
                       const int *mel_first = nullptr, const int *mel_start = nullptr, const float *mel_w = nullptr)
{
    const std::string w(who);
    if (B < 0 || T < 0 || skip < 0 || skip > T) return fail(NTM_EINVAL, w + ": bad size");
    if (n_fft != 64 && n_fft != 128 && n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048)
        return fail(NTM_EINVAL, w + ": n_fft must be a power of two from 64 to 2048");
    if (hop <= 0 || win_length <= 0 || win_length > n_fft) return fail(NTM_EINVAL, w + ": bad hop or win_length");
    if (!(floor_ > 0.0f)) return fail(NTM_EINVAL, w + ": the power floor must be positive");
    if (chunks < 1 || B * (int64_t)chunks > 0x7fffffff) return fail(NTM_EINVAL, w + ": bad chunks");
    if (B == 0) return NTM_OK;
    if (T - skip <= n_fft / 2) return fail(NTM_EINVAL, w + ": reflect padding needs T - skip > n_fft/2");
    if (T - skip > 0x7fffffff - 4096) return fail(NTM_EINVAL, w + ": T - skip must be below 2^31 - 4096");
    if (!y || !t || !out) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_stft_sums(y, t, B, T, skip, n_fft, hop, win_length, floor_, chunks, mode, out, (hipStream_t)stream,
                                         n_mels, mel_first, mel_start, mel_w);
    return e == hipSuccess ? NTM_OK : hip_fail(e, who);
}

int ntm_stft_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop, int win_length,
                  float power_eps, int chunks, double *out, void *stream)
{
    return stft_common("ntm_stft_sums", y, t, B, T, skip, n_fft, hop, win_length, power_eps, chunks, 0, out, stream);
}

int ntm_spec_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop, int win_length,
                  float log_floor, int chunks, double *out, void *stream)
{
    return stft_common("ntm_spec_sums", y, t, B, T, skip, n_fft, hop, win_length, log_floor, chunks, 1, out, stream);
}

int ntm_mel_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop, int win_length,
                 float log_floor, int chunks, int n_mels, const int32_t *mel_first, const int32_t *mel_start, const float *mel_w,
                 double *out, void *stream)
{
    if (n_fft != 1024 && n_fft != 2048) return fail(NTM_EINVAL, "ntm_mel_sums: n_fft must be 1024 or 2048");
    if (n_mels < 1 || n_mels > 4096) return fail(NTM_EINVAL, "ntm_mel_sums: bad n_mels");
    if (B > 0 && (!mel_first || !mel_start || !mel_w)) return fail(NTM_EINVAL, "ntm_mel_sums: null filter-bank pointer");
    return stft_common("ntm_mel_sums", y, t, B, T, skip, n_fft, hop, win_length, log_floor, chunks, 2, out, stream, n_mels,
                       mel_first, mel_start, mel_w);
}

// the argument checks of stft_common on the sizes of the adjoint (no chunk count: the launcher chooses the split)
static int stft_grad_sizes(const std::string &w, int64_t B, int64_t T, int64_t skip, int n_fft, int hop)
{
    if (B < 0 || T < 0 || skip < 0 || skip > T) return fail(NTM_EINVAL, w + ": bad size");
    if (n_fft != 64 && n_fft != 128 && n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048)
        return fail(NTM_EINVAL, w + ": n_fft must be a power of two from 64 to 2048");
    if (hop <= 0) return fail(NTM_EINVAL, w + ": bad hop or win_length");
    if (B == 0) return NTM_OK;
    if (T - skip <= n_fft / 2) return fail(NTM_EINVAL, w + ": reflect padding needs T - skip > n_fft/2");
    if (T - skip > 0x7fffffff - 4096) return fail(NTM_EINVAL, w + ": T - skip must be below 2^31 - 4096");
    // one frame-kernel workgroup per (stream, chunk), at most one chunk per frame; one gather thread per sample
    if (B * (1 + (T - skip) / hop) > 0x7fffffff || B * T > (int64_t)0x7fffffff * 256)
        return fail(NTM_EINVAL, w + ": B * frames and B * T / 256 must be below 2^31");
    return NTM_OK;
}

int64_t ntm_stft_grad_workspace_floats(int64_t B, int64_t T, int64_t skip, int n_fft, int hop)
{
    if (stft_grad_sizes("ntm_stft_grad_workspace_floats", B, T, skip, n_fft, hop) != NTM_OK) return -1;
    return B * (1 + (T - skip) / hop) * n_fft;
}

int ntm_stft_grad(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop, int win_length,
                  float power_eps, const float *coef, float *ws, float *dy, int accumulate, void *stream)
{
    const std::string w("ntm_stft_grad");
    if (int rc = stft_grad_sizes(w, B, T, skip, n_fft, hop)) return rc;
    if (win_length <= 0 || win_length > n_fft) return fail(NTM_EINVAL, w + ": bad hop or win_length");
    if (!(power_eps > 0.0f)) return fail(NTM_EINVAL, w + ": the power floor must be positive");
    if (B == 0) return NTM_OK;
    if (!y || !t || !coef || !ws || !dy) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_stft_grad(y, t, B, T, skip, n_fft, hop, win_length, power_eps, coef, ws, dy, accumulate,
                                         (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_stft_grad");
}

// the argument checks ntm_spectrogram and ntm_spectrogram_grad share (those of ntm_stft_sums without skip, floor and chunks)
static int spectrogram_sizes(const std::string &w, int64_t B, int64_t T, int n_fft, int hop, int win_length)
{
    if (int rc = stft_grad_sizes(w, B, T, 0, n_fft, hop)) return rc;
    if (win_length <= 0 || win_length > n_fft) return fail(NTM_EINVAL, w + ": bad hop or win_length");
    return NTM_OK;
}

int ntm_spectrogram(const float *y, int64_t B, int64_t T, int n_fft, int hop, int win_length, float *P, void *stream)
{
    const std::string w("ntm_spectrogram");
    if (int rc = spectrogram_sizes(w, B, T, n_fft, hop, win_length)) return rc;
    if (B == 0) return NTM_OK;
    if (!y || !P) return fail(NTM_EINVAL, w + ": null pointer");
    if (P == y) return fail(NTM_EINVAL, w + ": P must not alias y");
    hipError_t e = ntm::launch_spectrogram(y, B, T, n_fft, hop, win_length, P, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_spectrogram");
}

int ntm_spectrogram_grad(const float *y, const float *gP, int64_t B, int64_t T, int n_fft, int hop, int win_length, float *ws,
                         float *dy, int accumulate, void *stream)
{
    const std::string w("ntm_spectrogram_grad");
    if (int rc = spectrogram_sizes(w, B, T, n_fft, hop, win_length)) return rc;
    if (B == 0) return NTM_OK;
    if (!y || !gP || !ws || !dy) return fail(NTM_EINVAL, w + ": null pointer");
    if (dy == y || dy == gP || ws == y || ws == gP || ws == dy) return fail(NTM_EINVAL, w + ": dy and ws must not alias y, gP or each other");
    hipError_t e = ntm::launch_spectrogram_grad(y, gP, B, T, n_fft, hop, win_length, ws, dy, accumulate, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_spectrogram_grad");
}

// ---- the three critic conv stacks (the size checks they share: stack_sizes, above) ----
static int speccrit_sizes(const std::string &w, int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer *layers,
                          ntm::StackPlan &p)
{
    const int rc = stack_sizes(
        w, B, C0, F0, n_layers, layers, 8, true, [](int, const ntm_conv1d_layer &, int64_t) { return NTM_OK; },
        [&](int, const ntm_conv1d_layer &y, int64_t c, int64_t &F) {
            if (y.k > F) return fail(NTM_EINVAL, w + ": k is larger than the frames that reach the layer");
            if (B * c * F > 0x7fffffff) return fail(NTM_EINVAL, w + ": B * C * F must be below 2^31");
            F -= y.k - 1;
            return NTM_OK;
        });
    if (rc == NTM_OK) ntm::crit_plan(p, B, C0, F0, n_layers, layers);
    return rc;
}

static int convstack_sizes(const std::string &w, int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_d *layers,
                           ntm::StackPlan &p)
{
    const int rc = stack_sizes(
        w, B, C0, F0, n_layers, layers, ntm::kStackMaxLayers, false,
        [&](int, const ntm_conv1d_layer_d &y, int64_t) {
            if (y.dilation < 1 || y.dilation > (1 << 20)) return fail(NTM_EINVAL, w + ": dilation must lie in [1, 2^20]");
            return NTM_OK;
        },
        [&](int, const ntm_conv1d_layer_d &y, int64_t c, int64_t &F) {
            const int64_t span = (int64_t)(y.k - 1) * y.dilation;
            if (span + 1 > F) return fail(NTM_EINVAL, w + ": (k - 1) * dilation + 1 is larger than the frames that reach the layer");
            if (B * c * F > 0x7fffffff) return fail(NTM_EINVAL, w + ": B * C * F must be below 2^31");
            F -= span;
            return NTM_OK;
        });
    if (rc == NTM_OK) ntm::convstack_plan(p, B, C0, F0, n_layers, layers);
    return rc;
}

static int sconvstack_sizes(const std::string &w, int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_s *layers,
                            ntm::StackPlan &p)
{
    const int rc = stack_sizes(
        w, B, C0, F0, n_layers, layers, ntm::kStackMaxLayers, false,
        [&](int l, const ntm_conv1d_layer_s &y, int64_t F) {
            if (y.stride < 1 || y.stride > 64) return fail(NTM_EINVAL, w + ": stride must lie in [1, 64]");
            if (y.pad < 0 || y.pad > y.k - 1) return fail(NTM_EINVAL, w + ": pad must lie in [0, k - 1]");
            if (y.pad_mode != 0 && y.pad_mode != 1) return fail(NTM_EINVAL, w + ": pad_mode must be 0 (zeros) or 1 (reflect)");
            if (y.pad_mode == 1 && l != 0) return fail(NTM_EINVAL, w + ": pad_mode 1 (reflect) is built for the first layer only");
            if (y.pad_mode == 1 && y.pad >= F) return fail(NTM_EINVAL, w + ": a reflected pad must be smaller than F0");
            return NTM_OK;
        },
        [&](int l, const ntm_conv1d_layer_s &y, int64_t c, int64_t &F) {
            if (F + 2 * (int64_t)y.pad < y.k) return fail(NTM_EINVAL, w + ": a layer has no output frame (F + 2 pad < k)");
            if (B * c * (F + (l == 0 ? 2 * (int64_t)y.pad : 0)) > 0x7fffffff) return fail(NTM_EINVAL, w + ": B * C * F must be below 2^31");
            // one workgroup of 256 threads per (stream, 64 output frames) forward, per (stream, phase, 64 columns) in the data
            // gradient, whose columns are the frames of the (padded) input over the stride: both below 2^24 workgroups (2^32
            // threads per launch)
            const int64_t Fin = F + (y.pad_mode == 1 ? 2 * (int64_t)y.pad : 0), pad_eff = y.pad_mode == 1 ? 0 : y.pad;
            F = (F + 2 * (int64_t)y.pad - y.k) / y.stride + 1;
            if (B * y.c_out * F > 0x7fffffff) return fail(NTM_EINVAL, w + ": B * C * F must be below 2^31");
            const int64_t cols = (Fin - 1 + pad_eff) / y.stride + 1;
            if (B * ((F + 63) / 64) >= (1 << 24) || B * y.stride * ((cols + 63) / 64) >= (1 << 24))
                return fail(NTM_EINVAL, w + ": B * stride * ceil(frames / (64 stride)) must be below 2^24 (workgroups of one launch)");
            return NTM_OK;
        });
    if (rc == NTM_OK) ntm::sconv_plan(p, B, C0, F0, n_layers, layers);
    return rc;
}

// the pointer checks of a forward entry point; out: the output, or the strided family's array of them, outs (else null)
static int stack_forward_ptrs(const std::string &w, int n_layers, const float *x, const float *const *g, const float *const *v,
                              const float *const *bias, const float *saved, const void *out, float *const *outs)
{
    if (!x || !g || !v || !bias || !saved || !out) return fail(NTM_EINVAL, w + ": null pointer");
    for (int l = 0; l < n_layers; ++l)
        if (!g[l] || !v[l] || !bias[l] || (outs && !outs[l])) return fail(NTM_EINVAL, w + ": null pointer");
    return NTM_OK;
}

// ... of a backward entry point: the gradient arrives at the output (gout), or per_layer (the strided family) at the outputs of
// the layers: outs and gouts, one tensor per layer, of which at least one gouts entry is not null; gx aliases none of them
static int stack_backward_ptrs(const std::string &w, int n_layers, const float *x, const float *const *g, const float *const *v,
                               const float *saved, const float *gx, float *const *dg, float *const *dv, float *const *dbias,
                               const float *ws, const float *gout, bool per_layer, const float *const *outs,
                               const float *const *gouts)
{
    if (!x || !g || !v || !saved || (per_layer ? !outs || !gouts : !gout) || !ws) return fail(NTM_EINVAL, w + ": null pointer");
    if (dg && (!dv || !dbias)) return fail(NTM_EINVAL, w + ": null pointer (dg, dv and dbias come together)");
    const std::string alias = w + (per_layer ? ": gx must not alias x, outs or gouts" : ": gx must not alias x or gout");
    bool any = !per_layer;
    for (int l = 0; l < n_layers; ++l) {
        if (!g[l] || !v[l] || (per_layer && !outs[l]) || (dg && (!dg[l] || !dv[l] || !dbias[l])))
            return fail(NTM_EINVAL, w + ": null pointer");
        if (!per_layer) continue;
        any = any || gouts[l];
        if (gx && (gx == outs[l] || gx == gouts[l])) return fail(NTM_EINVAL, alias);
    }
    if (!any) return fail(NTM_EINVAL, w + ": every entry of gouts is null (at least one gradient must arrive)");
    if (gx && (gx == x || gx == gout)) return fail(NTM_EINVAL, alias);
    return NTM_OK;
}

static int speccrit_floor(const std::string &w, float log_floor)
{
    return log_floor >= 0.0f ? NTM_OK : fail(NTM_EINVAL, w + ": log_floor must be positive, or 0 for no log");
}

static int stack_slope(const std::string &w, float slope)
{
    return slope > 0.0f && slope < 1.0f ? NTM_OK : fail(NTM_EINVAL, w + ": slope must lie in (0, 1)");
}

int64_t ntm_speccrit_saved_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer *layers)
{
    ntm::StackPlan p;
    return speccrit_sizes("ntm_speccrit_saved_floats", B, C0, F0, n_layers, layers, p) == NTM_OK ? p.saved_total : -1;
}

int64_t ntm_speccrit_workspace_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer *layers)
{
    ntm::StackPlan p;
    return speccrit_sizes("ntm_speccrit_workspace_floats", B, C0, F0, n_layers, layers, p) == NTM_OK ? p.ws_total : -1;
}

int ntm_speccrit_forward(const float *x, int64_t B, int64_t C0, int64_t F0, float log_floor, int n_layers,
                         const ntm_conv1d_layer *layers, const float *const *g, const float *const *v, const float *const *bias,
                         float *saved, float *out, void *stream)
{
    const std::string w("ntm_speccrit_forward");
    ntm::StackPlan p;
    if (int rc = speccrit_sizes(w, B, C0, F0, n_layers, layers, p)) return rc;
    if (int rc = speccrit_floor(w, log_floor)) return rc;
    if (B == 0) return NTM_OK;
    if (int rc = stack_forward_ptrs(w, n_layers, x, g, v, bias, saved, out, nullptr)) return rc;
    hipError_t e = ntm::launch_speccrit_forward(p, x, B, log_floor, g, v, bias, saved, out, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_speccrit_forward");
}

int ntm_speccrit_backward(const float *x, int64_t B, int64_t C0, int64_t F0, float log_floor, int n_layers,
                          const ntm_conv1d_layer *layers, const float *const *g, const float *const *v, const float *saved,
                          const float *gout, float *gx, float *const *dg, float *const *dv, float *const *dbias, float *ws,
                          void *stream)
{
    const std::string w("ntm_speccrit_backward");
    ntm::StackPlan p;
    if (int rc = speccrit_sizes(w, B, C0, F0, n_layers, layers, p)) return rc;
    if (int rc = speccrit_floor(w, log_floor)) return rc;
    if (B == 0) return NTM_OK;
    if (int rc = stack_backward_ptrs(w, n_layers, x, g, v, saved, gx, dg, dv, dbias, ws, gout, false, nullptr, nullptr)) return rc;
    hipError_t e = ntm::launch_speccrit_backward(p, x, B, log_floor, g, v, saved, gout, gx, dg, dv, dbias, ws, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_speccrit_backward");
}

int64_t ntm_convstack_saved_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_d *layers)
{
    ntm::StackPlan p;
    return convstack_sizes("ntm_convstack_saved_floats", B, C0, F0, n_layers, layers, p) == NTM_OK ? p.saved_total : -1;
}

int64_t ntm_convstack_workspace_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_d *layers)
{
    ntm::StackPlan p;
    return convstack_sizes("ntm_convstack_workspace_floats", B, C0, F0, n_layers, layers, p) == NTM_OK ? p.ws_total : -1;
}

int ntm_convstack_forward(const float *x, int64_t B, int64_t C0, int64_t F0, float slope, int n_layers,
                          const ntm_conv1d_layer_d *layers, const float *const *g, const float *const *v, const float *const *bias,
                          float *saved, float *out, void *stream)
{
    const std::string w("ntm_convstack_forward");
    ntm::StackPlan p;
    if (int rc = convstack_sizes(w, B, C0, F0, n_layers, layers, p)) return rc;
    if (int rc = stack_slope(w, slope)) return rc;
    if (B == 0) return NTM_OK;
    if (int rc = stack_forward_ptrs(w, n_layers, x, g, v, bias, saved, out, nullptr)) return rc;
    hipError_t e = ntm::launch_convstack_forward(p, x, B, slope, g, v, bias, saved, out, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_convstack_forward");
}

int ntm_convstack_backward(const float *x, int64_t B, int64_t C0, int64_t F0, float slope, int n_layers,
                           const ntm_conv1d_layer_d *layers, const float *const *g, const float *const *v, const float *saved,
                           const float *gout, float *gx, float *const *dg, float *const *dv, float *const *dbias, float *ws,
                           void *stream)
{
    const std::string w("ntm_convstack_backward");
    ntm::StackPlan p;
    if (int rc = convstack_sizes(w, B, C0, F0, n_layers, layers, p)) return rc;
    if (int rc = stack_slope(w, slope)) return rc;
    if (B == 0) return NTM_OK;
    if (int rc = stack_backward_ptrs(w, n_layers, x, g, v, saved, gx, dg, dv, dbias, ws, gout, false, nullptr, nullptr)) return rc;
    hipError_t e = ntm::launch_convstack_backward(p, x, B, slope, g, v, saved, gout, gx, dg, dv, dbias, ws, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_convstack_backward");
}

int64_t ntm_sconvstack_saved_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_s *layers)
{
    ntm::StackPlan p;
    return sconvstack_sizes("ntm_sconvstack_saved_floats", B, C0, F0, n_layers, layers, p) == NTM_OK ? p.saved_total : -1;
}

int64_t ntm_sconvstack_workspace_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_s *layers)
{
    ntm::StackPlan p;
    return sconvstack_sizes("ntm_sconvstack_workspace_floats", B, C0, F0, n_layers, layers, p) == NTM_OK ? p.ws_total : -1;
}

int ntm_sconvstack_forward(const float *x, int64_t B, int64_t C0, int64_t F0, float slope, int n_layers,
                           const ntm_conv1d_layer_s *layers, const float *const *g, const float *const *v,
                           const float *const *bias, float *saved, float *const *outs, void *stream)
{
    const std::string w("ntm_sconvstack_forward");
    ntm::StackPlan p;
    if (int rc = sconvstack_sizes(w, B, C0, F0, n_layers, layers, p)) return rc;
    if (int rc = stack_slope(w, slope)) return rc;
    if (B == 0) return NTM_OK;
    if (int rc = stack_forward_ptrs(w, n_layers, x, g, v, bias, saved, outs, outs)) return rc;
    hipError_t e = ntm::launch_sconvstack_forward(p, x, B, slope, g, v, bias, saved, outs, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_sconvstack_forward");
}

int ntm_sconvstack_backward(const float *x, int64_t B, int64_t C0, int64_t F0, float slope, int n_layers,
                            const ntm_conv1d_layer_s *layers, const float *const *g, const float *const *v,
                            const float *saved, const float *const *outs, const float *const *gouts, float *gx,
                            float *const *dg, float *const *dv, float *const *dbias, float *ws, void *stream)
{
    const std::string w("ntm_sconvstack_backward");
    ntm::StackPlan p;
    if (int rc = sconvstack_sizes(w, B, C0, F0, n_layers, layers, p)) return rc;
    if (int rc = stack_slope(w, slope)) return rc;
    if (B == 0) return NTM_OK;
    if (int rc = stack_backward_ptrs(w, n_layers, x, g, v, saved, gx, dg, dv, dbias, ws, nullptr, true, outs, gouts)) return rc;
    hipError_t e = ntm::launch_sconvstack_backward(p, x, B, slope, g, v, saved, outs, gouts, gx, dg, dv, dbias, ws, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_sconvstack_backward");
}

int ntm_copy2d_async(void *dst, int64_t dst_pitch_bytes, const void *src, int64_t src_pitch_bytes, int64_t width_bytes,
                     int64_t rows, int kind, void *stream)
{
    if (width_bytes < 0 || rows < 0 || dst_pitch_bytes < width_bytes || src_pitch_bytes < width_bytes)
        return fail(NTM_EINVAL, "ntm_copy2d_async: bad size or pitch");
    if (kind != 0 && kind != 1) return fail(NTM_EINVAL, "ntm_copy2d_async: kind must be 0 (H2D) or 1 (D2H)");
    if (width_bytes == 0 || rows == 0) return NTM_OK;
    if (!dst || !src) return fail(NTM_EINVAL, "ntm_copy2d_async: null pointer");
    hipError_t e = hipMemcpy2DAsync(dst, (size_t)dst_pitch_bytes, src, (size_t)src_pitch_bytes, (size_t)width_bytes,
                                    (size_t)rows, kind == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost,
                                    (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_copy2d_async");
}

int ntm_demodulate(const float *x, float *out, int C, int64_t N, const int64_t *y_idx, int P, int64_t period, int64_t shift,
                   double *scratch, void *stream)
{
    if (C < 0 || N < 0) return fail(NTM_EINVAL, "ntm_demodulate: negative size");
    if (P < 2) return fail(NTM_EINVAL, "ntm_demodulate: at least two pulses are needed");
    if (period <= 0) return fail(NTM_EINVAL, "ntm_demodulate: pulse period must be positive");
    if (C == 0 || N == 0) return NTM_OK;
    if (N < 2) return fail(NTM_EINVAL, "ntm_demodulate: N must be at least 2");
    if (!x || !out || !y_idx || !scratch) return fail(NTM_EINVAL, "ntm_demodulate: null pointer");
    if (x == out) return fail(NTM_EINVAL, "ntm_demodulate: out must not alias x");
    hipError_t e = ntm::launch_demodulate(x, out, C, N, y_idx, P, period, shift, scratch, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_demodulate");
}

int ntm_tape_record_field(const double *I, const double *bias, double *H, int64_t B, int64_t N, double gain, double gap,
                          void *stream)
{
    if (B < 0 || N < 0 || !(gap < 0.0 || gap > 0.0)) return fail(NTM_EINVAL, "ntm_tape_record_field: bad size or gap");   // 0 and NaN
    if (B == 0 || N == 0) return NTM_OK;
    if (!I || !H) return fail(NTM_EINVAL, "ntm_tape_record_field: null pointer");
    hipError_t e = ntm::launch_tape_record_field(I, bias, H, B, N, gain, gap, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_tape_record_field");
}

int ntm_tape_hmag(const double *H, double *M, int64_t B, int64_t N, double *state, double Ts, const double *params5,
                  void *stream)
{
    if (B < 0 || N < 0 || !(Ts > 0.0)) return fail(NTM_EINVAL, "ntm_tape_hmag: bad size or Ts");
    if (B == 0 || N == 0) return NTM_OK;
    if (!H || !M || !state || !params5) return fail(NTM_EINVAL, "ntm_tape_hmag: null pointer");
    hipError_t e = ntm::launch_tape_hmag(H, M, B, N, state, Ts, params5, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_tape_hmag");
}

int ntm_resample_fir(const double *x, double *y, int64_t B, int64_t N, int64_t M, int up, int down, int width,
                     const double *kernel, void *stream)
{
    if (B < 0 || N < 0 || M < 0 || up < 1 || down < 1 || width < 0) return fail(NTM_EINVAL, "ntm_resample_fir: bad size");
    if (B > 65535) return fail(NTM_EINVAL, "ntm_resample_fir: at most 65535 streams per call");
    if (B == 0 || M == 0) return NTM_OK;
    if (!x || !y || !kernel || x == y) return fail(NTM_EINVAL, "ntm_resample_fir: null or aliased pointer");
    hipError_t e = ntm::launch_resample_fir(x, y, B, N, M, up, down, width, kernel, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_resample_fir");
}

int ntm_fir_f64(const double *x, double *y, int64_t B, int64_t N, const double *h, int taps, int clamp, void *stream)
{
    if (B < 0 || N < 0 || taps < 1) return fail(NTM_EINVAL, "ntm_fir_f64: bad size");
    if (B > 65535) return fail(NTM_EINVAL, "ntm_fir_f64: at most 65535 streams per call");
    if (B == 0 || N == 0) return NTM_OK;
    if (!x || !y || !h || x == y) return fail(NTM_EINVAL, "ntm_fir_f64: null or aliased pointer");
    hipError_t e = ntm::launch_fir_f64(x, y, B, N, h, taps, clamp, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_fir_f64");
}

namespace {
constexpr int kMaxDevices = 64;
struct TcnLanes {
    std::mutex mu;
    bool ready = false;
    hipStream_t lane[2] = {nullptr, nullptr};
    hipEvent_t fork = nullptr, done[2] = {nullptr, nullptr};
};
TcnLanes g_tcn_lanes[kMaxDevices];      // never destroyed: the runtime may already be gone when statics are torn down
}  // namespace

// The batch is processed in chunks of streams (streams are independent): the scratch is bounded by TCN_SCRATCH_BUDGET floats
// whatever B is -- 4096 x 65 536 x 32 ch took two 34.4 GB buffers as one launch set, and the per-GPU shapes of BASELINE
// configs[4] (B >= 8192) did not fit at all.  A batch that needs more than one chunk runs on TWO lanes: chunk k goes to lane
// k & 1, each lane has its own pair of activation buffers and its own HIP stream (forked from / joined to the caller's
// stream by events), so the drain of one chunk's launch is filled by the other
// lane's launch and the HBM-bound first block of one chunk runs under the matrix-pipe blocks of the other.  Chunks are
// equal-sized (the last may be smaller).  (The lane streams / events live in a per-device pool: this is the library's only
// state besides the thread-local error string, and it holds no data.)
static const int64_t TCN_SCRATCH_BUDGET = 2000000000;      // floats in total (8 GB): 2 lanes x 2 activation buffers
static int64_t tcn_chunk_streams(int64_t B, int64_t T, int C)
{
    const int64_t per = T * (int64_t)C;
    if (B * per <= TCN_SCRATCH_BUDGET / 2) return B;       // one chunk, two buffers, the caller's stream
    int64_t most = TCN_SCRATCH_BUDGET / 4 / per;
    if (most < 1) most = 1;                                // one stream longer than the budget: that stream alone
    const int64_t chunks = (B + most - 1) / most;
    return (B + chunks - 1) / chunks;
}

int64_t ntm_tcn_chunk_streams(int64_t B, int64_t T, int C)
{
    if (B <= 0 || T <= 0 || C <= 0) return 0;
    return tcn_chunk_streams(B, T, C);
}

int64_t ntm_tcn_scratch_floats(int64_t B, int64_t T, int C)
{
    if (B <= 0 || T <= 0 || C <= 0) return 0;
    const int64_t bc = tcn_chunk_streams(B, T, C);
    // per lane: two activation buffers, each padded by one 16-row block; two lanes when the batch is chunked
    return (bc < B ? 2 : 1) * 2 * (bc * T * (int64_t)C + 16 * (int64_t)C);
}

int ntm_tcn_forward(const float *params, int L, int C, int K, const int *dil, const float *x, float *y, int64_t B,
                    int64_t T, float *scratch, void *stream)
{
    if (L <= 0 || K <= 0 || B < 0 || T < 0) return fail(NTM_EINVAL, "ntm_tcn_forward: bad size");
    if (C != 32 || K != 13) return fail(NTM_EINVAL, "ntm_tcn_forward: only C = 32 channels, K = 13 taps is compiled");
    if (B == 0 || T == 0) return NTM_OK;
    if (!params || !dil || !x || !y || !scratch) return fail(NTM_EINVAL, "ntm_tcn_forward: null pointer");
    if ((reinterpret_cast<uintptr_t>(params) & 15) || (reinterpret_cast<uintptr_t>(scratch) & 15))
        return fail(NTM_EINVAL, "ntm_tcn_forward: params and scratch must be 16-byte aligned");
    if (T >= ((int64_t)1 << 31) - (1 << 25)) return fail(NTM_EINVAL, "ntm_tcn_forward: T must be below 2^31 - 2^25 samples");
    for (int l = 0; l < L; ++l)
        if (dil[l] <= 0 || dil[l] > (1 << 20)) return fail(NTM_EINVAL, "ntm_tcn_forward: dilations must lie in [1, 2^20]");
    const int64_t bc = tcn_chunk_streams(B, T, C);
    hipStream_t user = (hipStream_t)stream;
    if (bc >= B) {
        hipError_t e = ntm::launch_tcn(params, L, C, K, dil, x, y, B, T, scratch, user);
        return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_tcn_forward");
    }
    // two lanes: the side streams and the three events are created once per device and kept for the life of the process
    // (round 4 created and destroyed them per call -- hipStreamDestroy may wait for the queue to drain, which would have
    // turned "asynchronous on `stream`" into a host-blocking call for every chunked batch, and stream creation cannot be
    // captured into a graph).  The pool's mutex is held while the call ENQUEUES (microseconds): calls on one device share
    // the lanes, which only serialises work that would contend for the same CUs anyway.
    const int64_t lane_floats = 2 * (bc * T * (int64_t)C + 16 * (int64_t)C);
    // A call under stream capture keeps to the caller's stream: the pooled lanes are shared by every caller on the device, and
    // a lane forked into one caller's capture would drag a concurrent, un-captured call of another thread into that capture
    // (or fail it with a capture-isolation error); stream and event creation cannot be captured either.  The chunks then run
    // one after the other on `stream`, still alternating the two scratch halves -- same results, no lane overlap in the graph.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(user, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    if (cap != hipStreamCaptureStatusNone) {
        hipError_t ec = hipSuccess;
        int kc = 0;
        for (int64_t b0 = 0; b0 < B && ec == hipSuccess; b0 += bc, ++kc) {
            const int64_t n = B - b0 < bc ? B - b0 : bc;
            ec = ntm::launch_tcn(params, L, C, K, dil, x + b0 * T, y + b0 * T, n, T, scratch + (kc & 1) * lane_floats, user);
        }
        return ec == hipSuccess ? NTM_OK : hip_fail(ec, "ntm_tcn_forward");
    }
    int devi = 0;
    hipError_t e = hipGetDevice(&devi);
    if (e != hipSuccess) return hip_fail(e, "ntm_tcn_forward");
    if (devi < 0 || devi >= kMaxDevices) return fail(NTM_EINVAL, "ntm_tcn_forward: device ordinal beyond the lane pool");
    TcnLanes &P = g_tcn_lanes[devi];
    std::lock_guard<std::mutex> hold(P.mu);
    if (!P.ready) {
        // built into locals and committed only when all five handles exist: a failure half way destroys what it made
        // (a retry used to overwrite, i.e. leak, the handles of the first attempt)
        hipEvent_t fork = nullptr, done[2] = {nullptr, nullptr};
        hipStream_t lane[2] = {nullptr, nullptr};
        e = hipEventCreateWithFlags(&fork, hipEventDisableTiming);
        for (int i = 0; i < 2 && e == hipSuccess; ++i) {
            e = hipStreamCreateWithFlags(&lane[i], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&done[i], hipEventDisableTiming);
        }
        if (e != hipSuccess) {
            if (fork) (void)hipEventDestroy(fork);
            for (int i = 0; i < 2; ++i) {
                if (done[i]) (void)hipEventDestroy(done[i]);
                if (lane[i]) (void)hipStreamDestroy(lane[i]);
            }
            return hip_fail(e, "ntm_tcn_forward");
        }
        P.fork = fork;
        for (int i = 0; i < 2; ++i) { P.lane[i] = lane[i]; P.done[i] = done[i]; }
        P.ready = true;
    }
    e = hipEventRecord(P.fork, user);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipStreamWaitEvent(P.lane[i], P.fork, 0);
    int k = 0;
    for (int64_t b0 = 0; b0 < B && e == hipSuccess; b0 += bc, ++k) {
        const int64_t n = B - b0 < bc ? B - b0 : bc;
        e = ntm::launch_tcn(params, L, C, K, dil, x + b0 * T, y + b0 * T, n, T, scratch + (k & 1) * lane_floats, P.lane[k & 1]);
    }
    for (int i = 0; i < 2; ++i) {              // join -- also after an error, so that nothing outlives the caller's ordering
        if (hipEventRecord(P.done[i], P.lane[i]) == hipSuccess) (void)hipStreamWaitEvent(user, P.done[i], 0);
    }
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_tcn_forward");
}

// ---- training of GRU-HS[64] (csrc/gru_train.hip)
int64_t ntm_gru_train_workspace_floats(int64_t B, int64_t T)
{
    return (B < 0 || T < 0) ? 0 : B * T * NTM_TRAIN_SAVED * NTM_HIDDEN;
}

// R replicas in one launch each (stream s of R * Bper belongs to replica s / Bper): what every `_replicas` entry refuses first
static int bad_replicas(const char *who, int64_t R, int64_t Bper)
{
    const std::string w(who);
    if (R <= 0 || Bper <= 0) return fail(NTM_EINVAL, w + ": R and Bper must be positive");
    if (R > 65535) return fail(NTM_EINVAL, w + ": at most 65535 replicas per call");
    if (Bper > 0x7fffffff / R) return fail(NTM_EINVAL, w + ": at most 2^31 - 1 streams per call");
    return NTM_OK;
}

// Each single-model entry point and its `_replicas` form share one body: `rep` says which of the two `who` is.  The single form
// passes R = 1, Bper = B and keeps its own refusals and its B == 0 / T == 0 early returns (a replica call has Bper > 0).
static int bad_train_sizes(const char *who, bool rep, int64_t R, int64_t Bper, int64_t T)
{
    if (!rep) return (Bper < 0 || T < 0) ? fail(NTM_EINVAL, std::string(who) + ": negative B or T") : NTM_OK;
    if (int rc = bad_replicas(who, R, Bper)) return rc;
    return T < 0 ? fail(NTM_EINVAL, std::string(who) + ": negative T") : NTM_OK;
}

static int train_forward_impl(const char *who, bool rep, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                              const float *w_o, const float *b_o, const float *x, float *y, int64_t R, int64_t Bper, int64_t T,
                              int64_t x_stride_b, int64_t y_stride_b, float *h_state, float *ws, void *stream)
{
    static_assert(NTM_TRAIN_SAVED * NTM_HIDDEN == 5 * ntm::kH, "workspace layout");
    const std::string w(who);
    if (int rc = bad_train_sizes(who, rep, R, Bper, T)) return rc;
    if (Bper == 0 || T == 0) return NTM_OK;
    if (!w_ih || !w_hh || !b_ih || !b_hh || !w_o || !x || !y || !ws) return fail(NTM_EINVAL, w + ": null pointer");
    if (x_stride_b < T || y_stride_b < T) return fail(NTM_EINVAL, w + ": row stride below T");
    if (!rep && Bper > 0x7fffffff) return fail(NTM_EINVAL, w + ": at most 2^31 - 1 streams per call");
    if (x == y) return fail(NTM_EINVAL, w + ": y must not alias x");
    ntm::GruArgs a{w_ih, w_hh, b_ih, b_hh, w_o, b_o, x, y, h_state, R * Bper, T, x_stride_b, y_stride_b, nullptr, 0, 0};
    hipError_t e = ntm::launch_gru_train_fwd(a, ws, rep ? Bper : 0, (hipStream_t)stream);      // 0: the plain kernel
    return e == hipSuccess ? NTM_OK : hip_fail(e, who);
}

static int train_backward_impl(const char *who, bool rep, const float *w_hh, const float *w_o, const float *x, int64_t x_stride_b,
                               const float *ws, const float *dy, int64_t dy_stride_b, const float *dh_T, int64_t R, int64_t Bper,
                               int64_t T, float *dh0, float *part, void *stream)
{
    const std::string w(who);
    if (int rc = bad_train_sizes(who, rep, R, Bper, T)) return rc;
    if (Bper == 0) return NTM_OK;
    if (!w_hh || !w_o || !part || (T > 0 && (!x || !ws))) return fail(NTM_EINVAL, w + ": null pointer");
    if (x_stride_b < T || (dy && dy_stride_b < T)) return fail(NTM_EINVAL, w + ": row stride below T");
    if (!rep && Bper > 0x7fffffff) return fail(NTM_EINVAL, w + ": at most 2^31 - 1 streams per call");
    static_assert(NTM_TRAIN_GRAD_FLOATS == 12929, "parameter count of GRU(1, 64) + Linear(64, 1)");
    if (ntm::train_grad_floats() != NTM_TRAIN_GRAD_FLOATS) return fail(NTM_EINVAL, w + ": layout mismatch");
    hipError_t e = ntm::launch_gru_train_bwd(w_hh, w_o, x, x_stride_b, ws, dy, dy_stride_b, dh_T, R * Bper, T, dh0, part,
                                             rep ? Bper : 0, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, who);
}

// one model with B = 0: launched all the same, grad <- 0
static int train_reduce_impl(const char *who, bool rep, const float *part, int64_t R, int64_t Bper, float *grad, void *stream)
{
    const std::string w(who);
    if (rep) {
        if (int rc = bad_replicas(who, R, Bper)) return rc;
    } else if (Bper < 0) return fail(NTM_EINVAL, w + ": negative B");
    if (!grad || (Bper > 0 && !part)) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_gru_train_reduce_replicas(part, R, Bper, grad, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, who);
}

// the adjoint of ESR (pole null) or of DCPreESR with that pole
static int loss_grad_impl(const char *who, bool rep, const float *y, const float *t, int64_t R, int64_t Bper, int64_t T,
                          const float *pole, const double *sums2, const float *gout, double eps, float *dy, void *stream)
{
    const std::string w(who);
    if (rep)
        if (int rc = bad_replicas(who, R, Bper)) return rc;
    if (Bper < 0 || T < 0 || !(eps >= 0.0)) return fail(NTM_EINVAL, w + ": bad size or eps");
    if (pole && !(*pole >= 0.0f && *pole < 1.0f)) return fail(NTM_EINVAL, w + ": R must be in [0,1)");
    if (Bper == 0 || T == 0) return NTM_OK;
    if (!y || !t || !sums2 || !gout || !dy) return fail(NTM_EINVAL, w + ": null pointer");
    if (pole && !rep && Bper > 0x7fffffff) return fail(NTM_EINVAL, w + ": at most 2^31 - 1 streams per call");
    hipError_t e = pole ? ntm::launch_esr_dcpre_grad_replicas(y, t, R, Bper, T, *pole, sums2, gout, eps, dy, (hipStream_t)stream)
                        : ntm::launch_esr_grad_replicas(y, t, R, Bper * T, sums2, gout, eps, dy, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, who);
}

int ntm_gru_train_forward(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                          const float *b_o, const float *x, float *y, int64_t B, int64_t T, int64_t x_stride_b,
                          int64_t y_stride_b, float *h_state, float *ws, void *stream)
{
    return train_forward_impl("ntm_gru_train_forward", false, w_ih, w_hh, b_ih, b_hh, w_o, b_o, x, y, 1, B, T, x_stride_b, y_stride_b,
                              h_state, ws, stream);
}

int ntm_gru_train_forward_replicas(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                                   const float *b_o, const float *x, float *y, int64_t R, int64_t Bper, int64_t T,
                                   int64_t x_stride_b, int64_t y_stride_b, float *h_state, float *ws, void *stream)
{
    return train_forward_impl("ntm_gru_train_forward_replicas", true, w_ih, w_hh, b_ih, b_hh, w_o, b_o, x, y, R, Bper, T, x_stride_b,
                              y_stride_b, h_state, ws, stream);
}

int ntm_gru_train_backward(const float *w_hh, const float *w_o, const float *x, int64_t x_stride_b, const float *ws,
                           const float *dy, int64_t dy_stride_b, const float *dh_T, int64_t B, int64_t T, float *dh0,
                           float *part, void *stream)
{
    return train_backward_impl("ntm_gru_train_backward", false, w_hh, w_o, x, x_stride_b, ws, dy, dy_stride_b, dh_T, 1, B, T, dh0, part,
                               stream);
}

int ntm_gru_train_backward_replicas(const float *w_hh, const float *w_o, const float *x, int64_t x_stride_b, const float *ws,
                                    const float *dy, int64_t dy_stride_b, const float *dh_T, int64_t R, int64_t Bper, int64_t T,
                                    float *dh0, float *part, void *stream)
{
    return train_backward_impl("ntm_gru_train_backward_replicas", true, w_hh, w_o, x, x_stride_b, ws, dy, dy_stride_b, dh_T, R, Bper, T,
                               dh0, part, stream);
}

int ntm_gru_train_reduce(const float *part, int64_t B, float *grad, void *stream)
{
    return train_reduce_impl("ntm_gru_train_reduce", false, part, 1, B, grad, stream);
}

int ntm_gru_train_reduce_replicas(const float *part, int64_t R, int64_t Bper, float *grad, void *stream)
{
    return train_reduce_impl("ntm_gru_train_reduce_replicas", true, part, R, Bper, grad, stream);
}

int ntm_esr_grad(const float *y, const float *t, int64_t B, int64_t T, const double *sums2, const float *gout, double eps,
                 float *dy, void *stream)
{
    return loss_grad_impl("ntm_esr_grad", false, y, t, 1, B, T, nullptr, sums2, gout, eps, dy, stream);
}

int ntm_esr_grad_replicas(const float *y, const float *t, int64_t R, int64_t Bper, int64_t T, const double *sums2, const float *gout,
                          double eps, float *dy, void *stream)
{
    return loss_grad_impl("ntm_esr_grad_replicas", true, y, t, R, Bper, T, nullptr, sums2, gout, eps, dy, stream);
}

int ntm_esr_dcpre_grad(const float *y, const float *t, int64_t B, int64_t T, float R, const double *sums2, const float *gout,
                       double eps, float *dy, void *stream)
{
    return loss_grad_impl("ntm_esr_dcpre_grad", false, y, t, 1, B, T, &R, sums2, gout, eps, dy, stream);
}

int ntm_esr_dcpre_grad_replicas(const float *y, const float *t, int64_t R, int64_t Bper, int64_t T, float pole, const double *sums2,
                                const float *gout, double eps, float *dy, void *stream)
{
    return loss_grad_impl("ntm_esr_dcpre_grad_replicas", true, y, t, R, Bper, T, &pole, sums2, gout, eps, dy, stream);
}

int ntm_loss_sums_replicas(const double *rows, int64_t R, int64_t Bper, int splits, double *sums2, void *stream)
{
    if (int rc = bad_replicas("ntm_loss_sums_replicas", R, Bper)) return rc;
    if (splits < 1 || splits > 255) return fail(NTM_EINVAL, "ntm_loss_sums_replicas: splits must be in [1, 255]");
    if (!rows || !sums2) return fail(NTM_EINVAL, "ntm_loss_sums_replicas: null pointer");
    hipError_t e = ntm::launch_loss_sums_replicas(rows, R, Bper, splits, sums2, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_loss_sums_replicas");
}

// inference of R stacked replicas: ALWAYS the low-latency kernel (NTM_GRU_LAT), whatever R * Bper is -- NTM_GRU_AUTO's hand-over
// to the matrix-pipe kernel above NTM_GRU_LAT_MAX_B streams (mfma2_streams) has no counterpart here
int ntm_gru_forward_replicas(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                             const float *b_o, const float *x, float *y, int64_t R, int64_t Bper, int64_t T, int64_t x_stride_b,
                             int64_t y_stride_b, float *h_state, void *stream)
{
    if (int rc = bad_replicas("ntm_gru_forward_replicas", R, Bper)) return rc;
    if (T < 0) return fail(NTM_EINVAL, "ntm_gru_forward_replicas: negative T");
    if (T == 0) return NTM_OK;
    if (!w_ih || !w_hh || !b_ih || !b_hh || !w_o || !x || !y) return fail(NTM_EINVAL, "ntm_gru_forward_replicas: null pointer");
    if (x_stride_b < T || y_stride_b < T) return fail(NTM_EINVAL, "ntm_gru_forward_replicas: row stride below T");
    if (x == y) return fail(NTM_EINVAL, "ntm_gru_forward_replicas: y must not alias x");
    ntm::GruArgs a{w_ih, w_hh, b_ih, b_hh, w_o, b_o, x, y, h_state, R * Bper, T, x_stride_b, y_stride_b, nullptr, 0, 0};
    a.bper = (unsigned)Bper;
    hipError_t e = ntm::launch_gru_lat_replicas(a, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_gru_forward_replicas");
}

int ntm_delay_backward(const float *gy, const float *d, const float *g_newbuf, float *gpre, float *gbuf, int64_t B, int64_t L,
                       int D, int warmup, int flags, void *stream)
{
    if (B < 0 || L < 0 || D < 0) return fail(NTM_EINVAL, "ntm_delay_backward: negative size");
    if (flags & ~NTM_DELAY_BWD_SCAN) return fail(NTM_EINVAL, "ntm_delay_backward: unknown flags");
    if (B == 0 || L + D == 0) return NTM_OK;
    if (L > 0 && !gpre) return fail(NTM_EINVAL, "ntm_delay_backward: null gpre");
    if (!warmup && gy && !d) return fail(NTM_EINVAL, "ntm_delay_backward: null d");
    if ((gy && gy == gpre) || (g_newbuf && g_newbuf == gbuf)) return fail(NTM_EINVAL, "ntm_delay_backward: an output aliases an input");
    if (D > (1 << 24) || L + D > 0x7fffffffLL - 4096) return fail(NTM_EINVAL, "ntm_delay_backward: D above 2^24 or D + L above 2^31");
    if (B > 0x7fffffff) return fail(NTM_EINVAL, "ntm_delay_backward: at most 2^31 - 1 streams per call");
    hipError_t e = ntm::launch_delay_bwd(gy, d, g_newbuf, gpre, gbuf, B, L, D, warmup, flags & NTM_DELAY_BWD_SCAN, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_delay_backward");
}

// ---- DiffDelRNN block by block (csrc/diffdel_stream.hip)
static int64_t stream_ring_floats(int64_t D, int64_t block)
{
    int64_t C = 1;
    while (C < D + block) C <<= 1;
    return C;
}

int64_t ntm_diffdel_stream_ring_floats(int D, int64_t block)
{
    return (D < 0 || block < 0 || block > ((int64_t)1 << 40)) ? 0 : stream_ring_floats(D, block);
}

// what the three calls on a ring refuse first
static int bad_ring(const char *who, int64_t B, int D, int64_t C)
{
    const std::string w(who);
    if (B < 0 || D < 0) return fail(NTM_EINVAL, w + ": negative size");
    if (B > 0x7fffffff) return fail(NTM_EINVAL, w + ": at most 2^31 - 1 streams per call");
    if (C < 1 || (C & (C - 1)) || C < D) return fail(NTM_EINVAL, w + ": C must be a power of two, at least D (ntm_diffdel_stream_ring_floats)");
    return NTM_OK;
}

int ntm_diffdel_stream_seed(const float *dl_state, float *ring, int64_t *pos, int64_t B, int D, int64_t C, void *stream)
{
    if (int rc = bad_ring("ntm_diffdel_stream_seed", B, D, C)) return rc;
    if (B == 0) return NTM_OK;
    if (!ring || !pos || (D > 0 && !dl_state)) return fail(NTM_EINVAL, "ntm_diffdel_stream_seed: null pointer");
    hipError_t e = ntm::launch_diffdel_stream_seed(dl_state, ring, pos, B, D, C, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_diffdel_stream_seed");
}

int ntm_diffdel_stream_export(const float *ring, const int64_t *pos, float *dl_state, int64_t B, int D, int64_t C, void *stream)
{
    if (int rc = bad_ring("ntm_diffdel_stream_export", B, D, C)) return rc;
    if (B == 0 || D == 0) return NTM_OK;
    if (!ring || !pos || !dl_state) return fail(NTM_EINVAL, "ntm_diffdel_stream_export: null pointer");
    hipError_t e = ntm::launch_diffdel_stream_export(ring, pos, dl_state, B, D, C, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_diffdel_stream_export");
}

int ntm_diffdel_stream_block(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                             const float *x, const float *d, float *y, float *pre_d, int64_t B, int64_t block, int64_t x_stride_b,
                             int64_t d_stride_b, int64_t y_stride_b, float *h_state, float *ring, int64_t C, int64_t *pos, int D,
                             int warmup, int32_t *err_flag, void *stream)
{
    // every argument is checked BEFORE anything is enqueued
    if (B < 0 || block < 0 || D < 0) return fail(NTM_EINVAL, "ntm_diffdel_stream_block: negative size");
    if (B == 0 || block == 0) return NTM_OK;
    if (int rc = bad_ring("ntm_diffdel_stream_block", B, D, C)) return rc;
    if (block > C || C - block < D) return fail(NTM_EINVAL, "ntm_diffdel_stream_block: the ring must hold D + block samples (ntm_diffdel_stream_ring_floats)");
    if (!w_ih || !w_hh || !b_ih || !b_hh || !w_o || !x || !d || !y || !h_state || !ring || !pos)
        return fail(NTM_EINVAL, "ntm_diffdel_stream_block: null pointer");
    if (x_stride_b < block || d_stride_b < block || y_stride_b < block) return fail(NTM_EINVAL, "ntm_diffdel_stream_block: row stride below block");
    if (y == x || y == d || pre_d == x || pre_d == d || pre_d == y)
        return fail(NTM_EINVAL, "ntm_diffdel_stream_block: y and pre_d must not alias x, d or each other");
    ntm::StreamArgs sa{};
    sa.g = ntm::GruArgs{w_ih, w_hh, b_ih, b_hh, w_o, nullptr, x, pre_d ? pre_d : y, h_state, B, block, x_stride_b, y_stride_b, nullptr, 0, 0};
    sa.g.dd = d;
    sa.g.yd = y;
    sa.g.dl_flag = err_flag;
    sa.g.D = D;
    sa.g.warmup = warmup != 0;
    sa.ds = d_stride_b;
    sa.ring = ring;
    sa.pos = pos;
    sa.mask = C - 1;
    hipError_t e = ntm::launch_diffdel_stream(sa, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_diffdel_stream_block");
}

// the argument checks the two ntm_adv_head entry points share, then the kernels' record (a.g is left null)
static int adv_head_args(const std::string &w, const float *const *outs, const int64_t *elems, int K, int64_t rows, int64_t n_fake,
                         int mode, ntm::AdvHeadArgs &a)
{
    if (mode != NTM_ADV_HEAD_CRIT && mode != NTM_ADV_HEAD_GEN) return fail(NTM_EINVAL, w + ": mode must be NTM_ADV_HEAD_CRIT or NTM_ADV_HEAD_GEN");
    if (K < 1 || K > NTM_ADV_HEAD_MAX_K) return fail(NTM_EINVAL, w + ": K must lie in [1, 8]");
    if (rows < 1) return fail(NTM_EINVAL, w + ": bad size");
    if (mode == NTM_ADV_HEAD_CRIT && (n_fake < 1 || n_fake >= rows))
        return fail(NTM_EINVAL, w + ": n_fake must lie in [1, rows - 1] (each half has a mean of its own)");
    if (!outs || !elems) return fail(NTM_EINVAL, w + ": null pointer");
    a = ntm::AdvHeadArgs{};
    a.rows = rows;
    a.n_fake = mode == NTM_ADV_HEAD_CRIT ? n_fake : 0;
    a.K = K;
    a.mode = mode;
    for (int k = 0; k < K; ++k) {
        if (elems[k] < 1) return fail(NTM_EINVAL, w + ": bad size");
        if (elems[k] > (int64_t)1 << 40 || rows > (int64_t)1 << 40 || rows * elems[k] > (int64_t)1 << 40)
            return fail(NTM_EINVAL, w + ": an output must hold at most 2^40 floats");
        if (!outs[k]) return fail(NTM_EINVAL, w + ": null pointer");
        a.o[k] = outs[k];
        a.elems[k] = elems[k];
    }
    if (ntm::adv_head_chunks(a) > 0x7fffffff) return fail(NTM_EINVAL, w + ": more than 2^31 - 1 chunks in one half");
    return NTM_OK;
}

int ntm_adv_head_forward(const float *const *outs, const int64_t *elems, int K, int64_t rows, int64_t n_fake, int mode, double *ws,
                         int64_t ws_doubles, float *loss, void *stream)
{
    const std::string w("ntm_adv_head_forward");
    ntm::AdvHeadArgs a;
    if (int rc = adv_head_args(w, outs, elems, K, rows, n_fake, mode, a)) return rc;
    if (!ws || !loss) return fail(NTM_EINVAL, w + ": null pointer");
    if (ws_doubles < (mode == NTM_ADV_HEAD_GEN ? K : 2 * K) * ntm::adv_head_chunks(a))
        return fail(NTM_EINVAL, w + ": the workspace is smaller than segments * chunks doubles");
    hipError_t e = ntm::launch_adv_head_forward(a, ws, loss, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_adv_head_forward");
}

int ntm_adv_head_backward(const float *const *outs, const int64_t *elems, int K, int64_t rows, int64_t n_fake, int mode,
                          const float *gout, float *const *grads, void *stream)
{
    const std::string w("ntm_adv_head_backward");
    ntm::AdvHeadArgs a;
    if (int rc = adv_head_args(w, outs, elems, K, rows, n_fake, mode, a)) return rc;
    if (!gout || !grads) return fail(NTM_EINVAL, w + ": null pointer");
    for (int k = 0; k < K; ++k) {
        if (!grads[k]) return fail(NTM_EINVAL, w + ": null pointer");
        if (grads[k] == outs[k]) return fail(NTM_EINVAL, w + ": grads[k] must not alias outs[k]");
        a.g[k] = grads[k];
    }
    hipError_t e = ntm::launch_adv_head_backward(a, gout, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_adv_head_backward");
}

// ---- the optimiser step over a list of tensors (multi_tensor.hip) ----
extern "C++" {      // templates
constexpr int64_t kMultiMaxFloats = (int64_t)1 << 32;       // per tensor: 2^21 chunks
constexpr int64_t kMultiMaxGrid = (int64_t)1 << 23;         // workgroups per launch: 2^31 threads, below HIP's 2^32 per dimension

static int64_t multi_chunks(int64_t n)
{
    return (n + NTM_MULTI_CHUNK - 1) / NTM_MULTI_CHUNK;
}

// what every ntm_multi entry point checks of its NP lists of `count` device pointers and of n, all before a device is touched
template <int NP>
struct MultiLists {
    const void *const *l[NP];
    const void *const *operator[](int j) const { return l[j]; }
};

template <int NP>
static int multi_check(const std::string &w, const MultiLists<NP> &lists, const int64_t *n, int64_t count)
{
    if (count < 0) return fail(NTM_EINVAL, w + ": negative count");
    if (count == 0) return NTM_OK;
    if (!n) return fail(NTM_EINVAL, w + ": null pointer");
    for (int j = 0; j < NP; ++j)
        if (!lists[j]) return fail(NTM_EINVAL, w + ": null pointer");
    for (int64_t i = 0; i < count; ++i) {
        if (n[i] < 0) return fail(NTM_EINVAL, w + ": negative size (tensor " + std::to_string(i) + ")");
        if (n[i] > kMultiMaxFloats) return fail(NTM_EINVAL, w + ": a tensor must hold at most 2^32 floats");
        for (int j = 0; j < NP; ++j)
            if (n[i] > 0 && !lists[j][i]) return fail(NTM_EINVAL, w + ": null pointer (tensor " + std::to_string(i) + ")");
    }
    return NTM_OK;
}

// cuts the checked lists into tables of at most NTM_MULTI_MAX_TENSORS tensors (and kMultiMaxGrid workgroups) and hands each,
// with the number of chunks before it, to `go`; tensors of zero elements are skipped
template <int NP, class F>
static hipError_t multi_walk(const MultiLists<NP> &lists, const int64_t *n, int64_t count, F &&go)
{
    ntm::MultiTable<NP> t{};
    int64_t base = 0;
    for (int64_t i = 0; i <= count; ++i) {
        const int64_t c = i < count ? multi_chunks(n[i]) : 0;
        const bool full = t.count == NTM_MULTI_MAX_TENSORS || t.first[t.count] + c > kMultiMaxGrid;
        if (t.count > 0 && (i == count || (c > 0 && full))) {
            hipError_t e = go(t, base);
            if (e != hipSuccess) return e;
            base += t.first[t.count];
            t = ntm::MultiTable<NP>{};
        }
        if (c == 0) continue;
        for (int j = 0; j < NP; ++j) t.ptr[j][t.count] = const_cast<void *>(lists[j][i]);
        t.n[t.count] = n[i];
        t.first[t.count + 1] = t.first[t.count] + (int32_t)c;
        ++t.count;
    }
    return hipSuccess;
}

}  // extern "C++"

int64_t ntm_multi_partials(const int64_t *n, int64_t count)
{
    if (count < 0 || (count > 0 && !n)) return -1;
    int64_t total = 0;
    for (int64_t i = 0; i < count; ++i) {
        if (n[i] < 0 || n[i] > kMultiMaxFloats) return -1;
        total += multi_chunks(n[i]);
    }
    return total;
}

int ntm_multi_sqnorm(const float *const *g, const int64_t *n, int64_t count, double *partials, int64_t *n_partials_out, void *stream)
{
    const std::string w("ntm_multi_sqnorm");
    const MultiLists<1> lists{{(const void *const *)g}};
    if (int rc = multi_check(w, lists, n, count)) return rc;
    const int64_t total = ntm_multi_partials(n, count);
    if (total > 0 && !partials) return fail(NTM_EINVAL, w + ": null pointer (partials)");
    hipError_t e = multi_walk(lists, n, count, [&](const ntm::MultiTable<1> &t, int64_t base) {
        return ntm::launch_multi_sqnorm(t, partials, base, (hipStream_t)stream);
    });
    if (e != hipSuccess) return hip_fail(e, "ntm_multi_sqnorm");
    if (n_partials_out) *n_partials_out = total;
    return NTM_OK;
}

int ntm_multi_clip_coef(const double *partials, int64_t n_partials, float max_norm, float *norm_coef, void *stream)
{
    const std::string w("ntm_multi_clip_coef");
    if (n_partials < 0) return fail(NTM_EINVAL, w + ": negative size");
    if (!norm_coef || (n_partials > 0 && !partials)) return fail(NTM_EINVAL, w + ": null pointer");
    hipError_t e = ntm::launch_multi_norm_finalize(partials, n_partials, max_norm, norm_coef, (hipStream_t)stream);
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_multi_clip_coef");
}

int ntm_multi_adam(float *const *p, float *const *g, float *const *m, float *const *v, const int64_t *n, int64_t count,
                   const float *norm_coef, float step_size, float bc2_sqrt, float one_minus_beta1, float beta2, float one_minus_beta2,
                   float eps, void *stream)
{
    const std::string w("ntm_multi_adam");
    const MultiLists<4> lists{{(const void *const *)p, (const void *const *)g, (const void *const *)m, (const void *const *)v}};
    if (int rc = multi_check(w, lists, n, count)) return rc;
    for (int64_t i = 0; i < count; ++i)
        if (n[i] > 0 && (p[i] == m[i] || p[i] == v[i] || m[i] == v[i]))
            return fail(NTM_EINVAL, w + ": p, m and v of a tensor must not alias (tensor " + std::to_string(i) + ")");
    const ntm::MultiAdamScalars s{-step_size, bc2_sqrt, one_minus_beta1, beta2, one_minus_beta2, eps};
    hipError_t e = multi_walk(lists, n, count, [&](const ntm::MultiTable<4> &t, int64_t) {
        return ntm::launch_multi_adam(t, norm_coef, s, (hipStream_t)stream);
    });
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_multi_adam");
}

int ntm_multi_ema(float *const *dst, const float *const *src, const int64_t *n, int64_t count, float s, float one_minus_s, void *stream)
{
    const std::string w("ntm_multi_ema");
    const MultiLists<2> lists{{(const void *const *)dst, (const void *const *)src}};
    if (int rc = multi_check(w, lists, n, count)) return rc;
    hipError_t e = multi_walk(lists, n, count, [&](const ntm::MultiTable<2> &t, int64_t) {
        return ntm::launch_multi_ema(t, s, one_minus_s, (hipStream_t)stream);
    });
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_multi_ema");
}

// ---- the batch feeder of the diffusion trainers (segment_feed.hip) ----
extern "C++" {

// every row is checked before anything is launched
static int segment_check(const std::string &w, const float *bank, int64_t bank_len, const int64_t *start, int64_t B, int64_t L)
{
    if (B < 0) return fail(NTM_EINVAL, w + ": negative B");
    if (L < 1) return fail(NTM_EINVAL, w + ": L must be positive");
    if (!bank || !start) return fail(NTM_EINVAL, w + ": null pointer");
    for (int64_t b = 0; b < B; ++b)
        if (start[b] < 0 || bank_len < L || start[b] > bank_len - L)
            return fail(NTM_EINVAL, w + ": row " + std::to_string(b) + " lies outside the bank");
    return NTM_OK;
}

// the rows in launches of at most NTM_SEGMENT_MAX_ROWS; go(starts, first row, rows)
template <class F>
static hipError_t segment_walk(const int64_t *start, int64_t B, F &&go)
{
    for (int64_t b0 = 0; b0 < B; b0 += NTM_SEGMENT_MAX_ROWS) {
        const int rows = (int)(B - b0 < NTM_SEGMENT_MAX_ROWS ? B - b0 : NTM_SEGMENT_MAX_ROWS);
        ntm::SegStarts st{};
        for (int r = 0; r < rows; ++r) st.s[r] = start[b0 + r];
        hipError_t e = go(st, b0, rows);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // extern "C++"

int ntm_segment_mean(const float *bank, int64_t bank_len, const int64_t *start, int64_t B, int64_t L, float *mean, void *stream)
{
    const std::string w("ntm_segment_mean");
    if (!mean) return fail(NTM_EINVAL, w + ": null pointer");
    if (int rc = segment_check(w, bank, bank_len, start, B, L)) return rc;
    hipError_t e = segment_walk(start, B, [&](const ntm::SegStarts &st, int64_t b0, int rows) {
        return ntm::launch_segment_mean(bank, st, rows, L, mean + b0, (hipStream_t)stream);
    });
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_segment_mean");
}

int ntm_segment_crop(const float *bank, int64_t bank_len, const int64_t *start, const float *mean, int64_t B, int64_t L, float *out,
                     void *stream)
{
    const std::string w("ntm_segment_crop");
    if (!mean || !out) return fail(NTM_EINVAL, w + ": null pointer");
    if (int rc = segment_check(w, bank, bank_len, start, B, L)) return rc;
    hipError_t e = segment_walk(start, B, [&](const ntm::SegStarts &st, int64_t b0, int rows) {
        return ntm::launch_segment_crop(bank, st, mean + b0, rows, L, out + b0 * L, (hipStream_t)stream);
    });
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_segment_crop");
}

int ntm_segment_decimate(const float *bank, int64_t bank_len, const int64_t *start, const float *mean, int64_t B, int64_t L,
                         const float *ker, int orig, int width, int taps, float *out, void *stream)
{
    const std::string w("ntm_segment_decimate");
    if (!mean || !ker || !out) return fail(NTM_EINVAL, w + ": null pointer");
    if (orig < 1) return fail(NTM_EINVAL, w + ": orig must be positive");
    if (width < 0 || (int64_t)taps != 2 * (int64_t)width + orig) return fail(NTM_EINVAL, w + ": taps must be 2 width + orig, width >= 0");
    if (int rc = segment_check(w, bank, bank_len, start, B, L)) return rc;
    const int64_t n_out = (L + orig - 1) / orig;
    if (n_out > 0x7fffffff) return fail(NTM_EINVAL, w + ": ceil(L / orig) must be below 2^31");
    hipError_t e = segment_walk(start, B, [&](const ntm::SegStarts &st, int64_t b0, int rows) {
        return ntm::launch_segment_decimate(bank, st, mean + b0, rows, L, ker, orig, width, taps, n_out, out + b0 * n_out,
                                            (hipStream_t)stream);
    });
    return e == hipSuccess ? NTM_OK : hip_fail(e, "ntm_segment_decimate");
}

}  // extern "C"
