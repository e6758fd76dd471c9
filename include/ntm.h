/*
 * ntm.h -- C ABI of libntm.so: the MI355X (gfx950) kernels for the neural tape-nonlinearity
 * forward path of 01tot10/neural-tape-modeling.
 *
 * The reference has no FFI for this path: it is a Python torch.nn.Module protocol
 * (code/model.py).  Each entry point below names the reference call it replaces; the Python
 * host layer (neural-tape-modeling_amd/model.py) rebuilds the reference's object protocol on top
 * of these and INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (fp32) unless an entry point says otherwise (small
 *     host-side parameter arrays, the host side of ntm_copy2d_async); nothing is
 *     allocated or freed inside; no global state (carried state lives in the caller's h_state /
 *     dl_state buffers), so calls are re-entrant;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = default);
 *   - audio tensors are [B, T] row-major views of the reference's (B,1,T) layout with explicit
 *     per-stream strides in ELEMENTS (>= T);
 *   - return value: 0 on success, negative NTM_E* on failure; ntm_last_error() gives the
 *     thread-local message.  There is NO CPU fallback: without a HIP device every call fails.
 */
#ifndef NTM_H
#define NTM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTM_OK 0
#define NTM_EINVAL (-1)  /* bad argument (null pointer, negative size, unsupported H)  */
#define NTM_EHIP (-2)    /* HIP runtime error (launch failed, no device)               */
#define NTM_EDELAY (-3)  /* reserved for host-side delay-range checks                  */

#define NTM_ABI_VERSION 9 /* 2: hidden sizes 8/16/32/64; the delay line is one pass, no scratch, sticky error flag.  3: the TCN scratch is padded (ntm_tcn_scratch_floats grew), dilation / length limits.  4: ntm_diffdel_gru_forward is ONE fused launch where the matrix-pipe kernel runs (+ ntm_diffdel_gru_forward_ex).  5: ntm_gru_forward_esr, ntm_diffdel_gru_forward_esr.  6: ntm_tcn_forward works through the batch in stream chunks, ntm_tcn_scratch_floats is bounded (<= 2.0e9 floats + padding for any B), ntm_tcn_chunk_streams; DiffDelGRU warm-up calls always take the two-pass form.  7: ntm_loss_scalars (+ include/ntm_rccl.h, libntm_rccl.so).  8: any hidden size in [1, NTM_MAX_HIDDEN]; ntm_gru_forward_losses / ntm_diffdel_gru_forward_losses (ESR + DCPreESR sums in the recurrent launch).  9: NTM_GRU_BF16X3, ntm_gru_forward_io (any input_size / output_size) */

#define NTM_HIDDEN 64 /* hidden size of every shipped checkpoint (HS[64]): matrix-pipe and low-latency kernels.
                         Every other H in [1, NTM_MAX_HIDDEN] (the reference's `--HIDDEN_SIZE` is a free integer,
                         code/train.py:50; its constructor default is 8, code/model.py:22, its training default 16)
                         runs on gru_small.hip, any variant among AUTO / LAT / VALU: H = 8, 16, 32 one wavefront per
                         64/H streams; other H < 64 the same kernel zero-padded to the next power of two; 64 < H <=
                         128 a workgroup per stream with the weights in registers; above that a plain kernel that
                         streams the weights from L2 (correct, not fast).                                          */
#define NTM_MAX_HIDDEN 1024

/* GRU kernel variants (the laboratory ones: docs/DESIGN_measurement_log_r1_r5.md).  ntm_gru_forward_ex of libntm.so (the product) accepts NTM_GRU_AUTO, _MFMA2,
 * _LAT and the opt-in _F16X3 / _BF16X3; the others are LABORATORY kernels -- older or experimental exact-fp32 implementations
 * kept as independent checks and as measured dead ends -- compiled into libntm_lab.so only (include/ntm_lab.h).  */
#define NTM_GRU_AUTO 0  /* NTM_GRU_MFMA2, or NTM_GRU_LAT when B <= NTM_GRU_LAT_MAX_B         */
#define NTM_GRU_MFMA 1  /* 16 streams / workgroup, 4 waves, v_mfma_f32_16x16x4_f32, h in LDS */
#define NTM_GRU_VALU 2  /* 2 streams / wavefront, W_hh in VGPRs, h broadcast through LDS     */
#define NTM_GRU_MFMA2 3 /* as MFMA, own-quarter-first step order: LDS exchange hidden by MFMAs */
#define NTM_GRU_MFMA3 5 /* retired in round 6 (a measured negative result; the number stays reserved)     */
#define NTM_GRU_LAT 6   /* exact fp32, ONE stream per workgroup (K split over 4 waves): low latency, small B */
#define NTM_GRU_MFMA4 7 /* retired in round 6 (a measured negative result; the number stays reserved)     */
#define NTM_GRU_LAT_MAX_B 1024
#define NTM_GRU_F16X3 4 /* OPT-IN: MFMA2 with W.h as three fp16 hi/lo products, fp32 accumulate  */
#define NTM_GRU_BF16X3 8 /* OPT-IN: MFMA2 with W and h each split into THREE bf16 pieces (24 bits: the fp32 operands exactly) and
                            W.h as their eight partial products W_p.h_q, p + q <= 3 (W_3.h_3 <= 2^-32 |W||h| is dropped), each exact
                            in fp32, on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; state, gates and head in fp32 as MFMA2 */

/* ABI version of this header; bumped on any signature change. */
int ntm_abi_version(void);

/* Thread-local message for the last failing call on this thread ("" if none). */
const char *ntm_last_error(void);

/*
 * Replaces  x, self.hidden = self.GRU(x, self.hidden); y = self.output(x)
 * at code/model.py:81-82 (RNN.forward) and :412-413 (DiffDelRNN.forward, where b_o == NULL
 * because the head is Linear(..., bias=False), code/model.py:365).
 *
 * Weights in the reference's state_dict layout, gate row order r,z,n:
 *   w_ih [3H]      GRU.weight_ih_l0 (3H,1)      w_hh [3H,H]   GRU.weight_hh_l0
 *   b_ih [3H]      GRU.bias_ih_l0               b_hh [3H]     GRU.bias_hh_l0
 *   w_o  [H]       output.weight (1,H)          b_o  [1] or NULL   output.bias
 * x [B,T] (stride x_stride_b) -> y [B,T] (stride y_stride_b).
 * 1 <= H <= NTM_MAX_HIDDEN.  h_state [B,H] is read as h_0 and overwritten with h_T (the reference's self.hidden);
 * NULL means h_0 = 0 and h_T is discarded.  B == 0 or T == 0 is a successful no-op.
 */
int ntm_gru_forward(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                    const float *w_o, const float *b_o, int H, const float *x, float *y,
                    int64_t B, int64_t T, int64_t x_stride_b, int64_t y_stride_b, float *h_state,
                    void *stream);

/*
 * The same reference call for ANY input_size / output_size: self.GRU = nn.GRU(input_size, hidden_size, batch_first=True),
 * self.output = nn.Linear(hidden_size, output_size) (code/model.py:22,44-45), forward code/model.py:67-88.  The reference moves
 * between (B, C, T) and (B, T, C) with `reshape` (:77, :87) -- a reinterpretation of the row, not a transpose -- so per stream the
 * input row of I T floats IS the [T][I] matrix the GRU reads and the output row of O T floats IS the [T][O] matrix the head
 * writes: x [B] rows of T*I floats (x_stride_b >= T*I), y [B] rows of T*O floats.  w_ih [3H, I], w_o [O, H], b_o [O] or NULL;
 * h_state [B, H] in/out or NULL (zeros).  H, I, O in [1, 1024].  No caller of the reference uses sizes other than 1
 * (code/test-model.py:124-125): a plain, correct kernel (a workgroup per stream, weights from L2), not a fast one; pinned by
 * golden g22 from the reference's own forward().  The skip connection (y += x, output_size == input_size) is the caller's.
 */
int ntm_gru_forward_io(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                       const float *w_o, const float *b_o, int H, int I, int O, const float *x, float *y,
                       int64_t B, int64_t T, int64_t x_stride_b, int64_t y_stride_b, float *h_state, void *stream);

/* Same, with an explicit kernel variant (NTM_GRU_*); used by bench.py / tests to A/B kernels. */
int ntm_gru_forward_ex(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                       const float *w_o, const float *b_o, int H, const float *x, float *y,
                       int64_t B, int64_t T, int64_t x_stride_b, int64_t y_stride_b,
                       float *h_state, int variant, void *stream);

/*
 * RNN.forward + the ESR sums of the loss loop in ONE call: replaces
 *     output = model(input)  ...  loss_fcn(output[..., INIT_LEN:], target[..., INIT_LEN:])      (code/test-model.py:346,386-388)
 * for the ESR entry of the loss dict.  Arguments as ntm_gru_forward (kernel choice = NTM_GRU_AUTO), then
 * target [B,T] contiguous, skip (= INIT_LEN), and esr_out [B,2] fp64 (device):
 *     esr_out[2b] = sum_{n >= skip} (target - y)^2,   esr_out[2b+1] = sum_{n >= skip} target^2      of stream b
 * -- the per-sample terms of ntm_esr_sums (fp32 difference, fp64 products and sums), added in a fixed order.  Where the
 * matrix-pipe kernel runs (H = 64, B > NTM_GRU_LAT_MAX_B, skip a multiple of 4) the sums are accumulated inside that launch,
 * in the y-tile flush where the outputs sit in registers (the separate 2 GB pass, overlapped with the next launch, cost
 * that launch 0.37 ms at 4096 x 65 536); elsewhere it is the forward launch followed by the streaming pass (then y must
 * be contiguous).  target must not alias y.
 */
int ntm_gru_forward_esr(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                        const float *w_o, const float *b_o, int H, const float *x, float *y,
                        int64_t B, int64_t T, int64_t x_stride_b, int64_t y_stride_b, float *h_state,
                        const float *target, int64_t skip, double *esr_out, void *stream);

/*
 * RNN.forward + BOTH time-domain entries of the loss dict in ONE call: replaces
 *     output = model(input)  ...  for key in loss_fcns: loss_fcns[key](output[..., INIT_LEN:], target[..., INIT_LEN:])
 * (code/test-model.py:250-252,346,386-388) for the ESR and the DCPreESR entries.  Arguments as ntm_gru_forward_esr, then the
 * pole dcpre_R of the DC blocker (0.995 upstream) and dcpre_out [B,2] fp64 (device), the sums of ntm_esr_dcpre_sums:
 *     dcpre_out[2b] = sum f(target - y)^2,   dcpre_out[2b+1] = sum f(target)^2,   f = (1 - z^-1)/(1 - R z^-1) from zero
 * state at sample `skip`.  Where the matrix-pipe kernel runs (H = 64, B > NTM_GRU_LAT_MAX_B, skip a multiple of 4) both pairs
 * of sums come out of that launch: the one-pole filter is a 16-lane scan inside the y-tile flush (the streaming pass reads
 * y and target again, 2 GB at 4096 x 65 536); elsewhere the forward launch is followed by the two streaming passes.  The fp32
 * filter is evaluated in scan order there and in the streaming kernel's order elsewhere: the two agree with each other and
 * with the sequential recursion to ~1e-6 relative in the sums (not bit for bit).
 */
int ntm_gru_forward_losses(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                           const float *w_o, const float *b_o, int H, const float *x, float *y,
                           int64_t B, int64_t T, int64_t x_stride_b, int64_t y_stride_b, float *h_state,
                           const float *target, int64_t skip, double *esr_out, float dcpre_R,
                           double *dcpre_out, void *stream);

/*
 * Replaces TimeVaryingDelayLine.forward(x, dt, warmup), code/model.py:269-320.
 * x, d, y: [B,T] contiguous (stride T); d in SAMPLES.  dl_state [B,D] is the reference's
 * `self.buffer` (oldest sample first) and is updated in place to cat(buffer[T:], x[-D:]).
 * warmup != 0: y = x, only the buffer is updated (code/model.py:288-292).
 * y must not alias x.  One pass over the audio: d is read once, there is no separate range check.
 * err_flag (device int32, caller-owned, may be NULL): raised to 1 if any d > D (or NaN) -- the reference raises
 * AssertionError there (code/model.py:284) before touching its state; here y of the violating call is
 * unspecified and dl_state is left untouched.  The flag is STICKY: while it is non-zero every later call that is
 * given the same flag is a no-op (the state stays frozen at the last good call), so a caller that streams many
 * chunks may look at it once at the end instead of synchronising per chunk, and clears it (hipMemsetAsync)
 * when it re-initialises the state.
 */
int ntm_delay_forward(const float *x, const float *d, float *y, int64_t B, int64_t T,
                      float *dl_state, int D, int warmup, int32_t *err_flag, void *stream);

/*
 * Replaces DiffDelRNN.forward(x, del_traj, warmup), code/model.py:393-424:
 * the GRU + bias-free head writes pre_d, the delay line writes y.  Returns (y, pre_d) through the two
 * output pointers (distinct buffers, neither aliasing x); x, d, y, pre_d [B,T] contiguous; h_state, dl_state,
 * err_flag as above (a violation leaves dl_state untouched; h_state is h_T either way -- the reference assigns
 * self.hidden at :412 before its delay line asserts).
 *
 * Where the matrix-pipe kernel runs (H = 64, B > NTM_GRU_LAT_MAX_B) the step is ONE fused launch: the delay line
 * interpolates the kernel's own pre_d output inside the y-tile housekeeping of the recurrence, one 64-sample tile
 * behind it (taps read back through L2; d is read once, pre_d is never re-read from HBM), bit-identical to the separate
 * pass on the same pre_d; a small launch moves the carried buffer on afterwards.  Small batches and H < 64 run the GRU
 * launch followed by the streaming delay pass (NTM_DIFFDEL_TWO_PASS).  ntm_diffdel_gru_forward = mode NTM_DIFFDEL_AUTO.
 */
#define NTM_DIFFDEL_AUTO 0     /* fused where the matrix-pipe kernel runs, two passes elsewhere          */
#define NTM_DIFFDEL_TWO_PASS 1 /* ntm_gru_forward then ntm_delay_forward                                 */
#define NTM_DIFFDEL_FUSED 2    /* the fused kernel for every stream (H = 64), whatever B is (tests, A/B) */
int ntm_diffdel_gru_forward(const float *w_ih, const float *w_hh, const float *b_ih,
                            const float *b_hh, const float *w_o, int H, const float *x,
                            const float *d, float *y, float *pre_d, int64_t B, int64_t T,
                            float *h_state, float *dl_state, int D, int warmup, int32_t *err_flag,
                            void *stream);
int ntm_diffdel_gru_forward_ex(const float *w_ih, const float *w_hh, const float *b_ih,
                               const float *b_hh, const float *w_o, int H, const float *x,
                               const float *d, float *y, float *pre_d, int64_t B, int64_t T,
                               float *h_state, float *dl_state, int D, int warmup, int32_t *err_flag,
                               int mode, void *stream);
/*
 * DiffDelRNN.forward + the ESR sums of the loss loop (code/test-model.py:353,386-388) in one call: as
 * ntm_diffdel_gru_forward (warmup = 0, mode NTM_DIFFDEL_AUTO), then target [B,T] contiguous, skip (= INIT_LEN) and
 * esr_out [B,2] fp64 = sum (target - y)^2 | sum target^2 over samples [skip, T) of each stream, y being the DELAYED output.
 * Inside the fused launch (in its delay stage, where a thread's 4 outputs are in registers) when that launch runs and skip is a
 * multiple of 4; by the streaming ESR pass otherwise.  After a delay-range violation (err_flag raised) the sums are unspecified,
 * like y.
 */
int ntm_diffdel_gru_forward_esr(const float *w_ih, const float *w_hh, const float *b_ih,
                                const float *b_hh, const float *w_o, int H, const float *x,
                                const float *d, float *y, float *pre_d, int64_t B, int64_t T,
                                float *h_state, float *dl_state, int D, int32_t *err_flag,
                                const float *target, int64_t skip, double *esr_out, void *stream);

/* DiffDelRNN.forward + BOTH time-domain entries of the loss dict (ESR and DCPreESR of the DELAYED output, code/test-model.py:250-252,
 * 353,386-388) in one call: as ntm_diffdel_gru_forward_esr, plus dcpre_R / dcpre_out [B,2] fp64 as in ntm_gru_forward_losses.  Where the
 * fused step runs both pairs of sums come out of that ONE launch (accumulated in its delay stage); elsewhere the streaming passes follow. */
int ntm_diffdel_gru_forward_losses(const float *w_ih, const float *w_hh, const float *b_ih,
                                   const float *b_hh, const float *w_o, int H, const float *x,
                                   const float *d, float *y, float *pre_d, int64_t B, int64_t T,
                                   float *h_state, float *dl_state, int D, int32_t *err_flag,
                                   const float *target, int64_t skip, double *esr_out, float dcpre_R,
                                   double *dcpre_out, void *stream);

/*
 * Per-stream sums for the ESR loss that follows the path in code/test-model.py:250-254,386-388
 * (CoreAudioML ESRLoss, un-vendored): over samples [skip, T) of stream b, split over `splits` workgroups p:
 *   out[(b*splits + p)*2 + 0] = partial sum (t - y)^2      out[(b*splits + p)*2 + 1] = partial sum t^2   (fp64, device)
 * The caller adds the `splits` rows of a stream in index order: no atomics anywhere, the sums are bit-reproducible
 * from run to run for every B.  ntm_esr_splits() gives the split count that fills the device (1 for B >= 2048).
 * y, t: [B,T] contiguous.
 */
int ntm_esr_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int splits, double *out,
                 void *stream);
int ntm_esr_splits(int64_t B, int64_t T, int64_t skip);

/*
 * This rank's four loss scalars from per-stream ESR rows (esr_out of ntm_gru_forward_esr / ntm_diffdel_gru_forward_esr, or the
 * summed partial rows of ntm_esr_sums): what the loss loop of code/test-model.py:386-398 aggregates over the segments --
 *     out4 = [ sum_b ESR_b,  B,  sum_b err2_b,  sum_b tgt2_b ],     ESR_b = (err2_b / n_samples) / (tgt2_b / n_samples + eps)
 * (eps = 1e-5: CoreAudioML's ESRLoss; n_samples = T - skip) -- fp64, device in, device out, one small launch, bit-reproducible.
 * A job sharded over ranks adds these four numbers over the ranks (ntm_rccl_allreduce_f64 in include/ntm_rccl.h, MPI, or
 * torch.distributed) and divides out4[0] by out4[1]: the mean over segments of the per-segment loss.  B == 0 gives zeros.
 */
int ntm_loss_scalars(const double *esr_rows, int64_t B, int64_t n_samples, double eps, double *out4, void *stream);

/*
 * As ntm_esr_sums, on the DC-blocked signals: both y and t pass H(z) = (1 - z^-1)/(1 - R z^-1) (zero state
 * at sample `skip`) before the sums are taken -- the `DCPreESR(dc_pre=True)` loss of code/test-model.py:252
 * and code/train.py:173-174 (GreyBoxDRC, un-vendored: parity unpinned; upstream truncates the impulse
 * response to 2000 taps, this is the untruncated recursion).  R = 0.995 upstream.
 */
int ntm_esr_dcpre_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, float R,
                       double *out, void *stream);

/*
 * "Next" row N1: per-stream sums of the multi-resolution STFT loss of code/test-model.py:25,253
 * (`MultiResolutionSTFTLoss()` of the un-vendored auraloss submodule: parity unpinned by the reference; the
 * arithmetic is pinned to torch.stft by tests/golden/g10).  For ONE resolution, over samples [skip, T) of each
 * stream:  X = stft(x, n_fft, hop, win_length, periodic Hann, centred, reflect padding),
 * mag = sqrt(max(re^2 + im^2, power_eps)), and with P = 4 * chunks partial rows per stream
 *   out[(b*P + p)*4 + 0..3] = sum (mag_t - mag_y)^2 | sum mag_t^2 | sum |ln mag_y - ln mag_t| | sum |mag_y - mag_t|
 * (fp64, device; the caller adds the P rows of a stream).  y = prediction, t = target, [B,T] contiguous.
 * n_fft in {64, 128, 256, 512, 1024, 2048}; 0 < win_length <= n_fft; T - skip > n_fft/2; power_eps > 0 (auraloss: 1e-8);
 * chunks >= 1 splits the frames of a stream over that many workgroups.  There are 1 + (T-skip)/hop frames
 * of n_fft/2 + 1 bins.
 */
int ntm_stft_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop,
                  int win_length, float power_eps, int chunks, double *out, void *stream);

/*
 * Same transform and layout as ntm_stft_sums, with the POWER-spectrogram terms of the reference's validation
 * metric bundle (code/evaluation.py:75-84: `TimeFreqConverter` = torchaudio Spectrogram(n_fft, hop = n_fft/4,
 * power = 2), un-vendored torchaudio semantics = torch.stft, parity pinned to torch.stft by golden g13):
 *   out[..0..3] = sum |P_y - P_t| | sum |log10 max(P_y, log_floor) - log10 max(P_t, log_floor)| | sum P_t | sum P_y
 * (log_floor = 1e-5 in the reference).
 */
int ntm_spec_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop,
                  int win_length, float log_floor, int chunks, double *out, void *stream);

/*
 * The two MEL entries of the same bundle (code/evaluation.py:86-92): the power spectrogram of
 * `TimeFreqConverter(n_fft = 2048, hop 512)` projected on the mel basis `librosa.filters.mel(sr, n_fft, 160)`
 * (code/utilities/utilities.py:639-646, :666) inside the transform kernel, then
 *   out[..0..3] = sum |mel_y - mel_t| | sum |log10 max(mel_y, log_floor) - log10 max(mel_t, log_floor)| | sum mel_t | sum mel_y
 * in the partial-row layout of ntm_stft_sums.  The filter bank comes in row-compressed form (device arrays): filter m
 * has weights mel_w[mel_start[m] .. mel_start[m+1]) on the bins mel_first[m], mel_first[m] + 1, ...  (host helper:
 * ntm_amd.utilities.mel_filterbank_sparse; librosa is un-vendored and absent: published algorithm, parity unpinned).
 * n_fft in {1024, 2048}; there are (1 + (T-skip)/hop) * n_mels cells per stream.
 */
int ntm_mel_sums(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop, int win_length,
                 float log_floor, int chunks, int n_mels, const int32_t *mel_first, const int32_t *mel_start,
                 const float *mel_w, double *out, void *stream);

/*
 * Adjoint of ntm_stft_sums for ONE resolution (the backward of MRSTFTLoss): with per-stream coefficients
 * coef[b] = (c_sc, c_log, c_lin) (device, [B,3] fp32),
 *   dy[b] = d/dy sum_cells ( 1/2 c_sc (my - mt)^2 + c_log |ln my - ln mt| + c_lin |my - mt| )
 * over the cells of stream b, my / mt the magnitudes of ntm_stft_sums (same frames, padding, window -- here each value
 * correctly rounded to fp32 -- and floor: where the
 * unclamped power of the prediction is at or below power_eps the cell contributes nothing; sgn(0) = 0).  Gradients go to
 * the prediction y only.  dy [B,T] fp32: samples before `skip` get 0.  accumulate != 0: dy[i] = dy[i] + gradient in
 * place of the store (samples before `skip` stay as they are) -- how the caller adds the resolutions, in its call order.
 * ws: ntm_stft_grad_workspace_floats(B, T, skip, n_fft, hop) floats of device scratch (the windowed frame gradients,
 * B * frames * n_fft; -1 for sizes ntm_stft_grad refuses).  No atomics: the overlap-add is a gather with a fixed order
 * of addition (csrc/stft_kernels.hip), so equal calls give equal bits, and a stream's result does not depend on the
 * batch it is in.  Same argument checks as ntm_stft_sums; B == 0 returns NTM_OK without looking at the pointers.
 */
int64_t ntm_stft_grad_workspace_floats(int64_t B, int64_t T, int64_t skip, int n_fft, int hop);
int ntm_stft_grad(const float *y, const float *t, int64_t B, int64_t T, int64_t skip, int n_fft, int hop, int win_length,
                  float power_eps, const float *coef, float *ws, float *dy, int accumulate, void *stream);

/*
 * The power spectrogram ITSELF, for a caller that reads its cells: the front end of the reference's spectral critics
 * (`TimeFreqConverter`, code/utilities/utilities.py:627-672 = torchaudio Spectrogram(power = 2) = |torch.stft|^2).
 *   P[b][k][f] = |stft(y_b, n_fft, hop, win_length, periodic Hann, centred, reflect padding)[k, f]|^2
 * y [B,T] fp32 contiguous; P [B][n_fft/2 + 1][1 + T/hop] fp32 contiguous (torch's layout: bins, then frames).  Frames,
 * padding and window placement are those of ntm_stft_sums without `skip`.  Window, transform and powers are computed in
 * fp64 and each cell is rounded to fp32 once (a network behind P divides by it: DESIGN.md 11.5).  Two frames (2j, 2j + 1) of a stream share one complex transform; a last frame without a
 * partner is paired with itself.  Every cell is written once: equal calls give equal bits; a stream's result does not
 * depend on its batch.  Argument checks as ntm_stft_sums (n_fft in {64, ..., 2048}; 0 < win_length <= n_fft; hop >= 1;
 * T > n_fft/2; T < 2^31 - 4096, B * frames < 2^31), made before anything touches a device; P must not be y.  B == 0
 * returns NTM_OK without looking at the pointers.
 */
int ntm_spectrogram(const float *y, int64_t B, int64_t T, int n_fft, int hop, int win_length, float *P, void *stream);

/*
 * Adjoint of ntm_spectrogram: with an upstream gradient gP in P's layout,
 *   dy[b] = d/dy sum_{k,f} gP[b][k][f] P[b][k][f]
 * -- per frame g_f[n] = w[n] Re sum_{k=0}^{n_fft/2} conj(c_k) e^{-2 pi i k n / n_fft}, c_k = 2 gP[b][k][f] Y_k (every bin once,
 * no 1/N, no doubling), Y recomputed from y in fp64 (nothing is saved by the forward), each frame gradient rounded to fp32, then the overlap-add back through the
 * reflect padding.  dy [B,T] fp32; accumulate != 0: dy[i] = dy[i] + gradient in place of the store.  ws:
 * ntm_stft_grad_workspace_floats(B, T, 0, n_fft, hop) floats of device scratch (the windowed frame gradients,
 * [B][frames][n_fft]).  No atomics: the overlap-add is ntm_stft_grad's gather with its fixed order of addition (direct
 * position, left mirror, right mirror; frames ascending -- csrc/stft_kernels.hip), so equal calls give equal bits, and a
 * stream's result does not depend on its batch.  Same argument checks as ntm_spectrogram; dy and ws must not be y, gP or
 * each other.  B == 0 returns NTM_OK without looking at the pointers.
 */
int ntm_spectrogram_grad(const float *y, const float *gP, int64_t B, int64_t T, int n_fft, int hop, int win_length,
                         float *ws, float *dy, int accumulate, void *stream);

/*
 * The conv stack of the reference's spectral critics behind the spectrogram (`SpecCrit`, code/critics.py:181-259), forward
 * and backward: n_layers weight-normed Conv1d(c_in, c_out, k, groups) with stride 1, dilation 1 and no padding, effective
 * weight w = g v / |v| (the norm over (c_in/groups, k) per output channel: torch.nn.utils.weight_norm, dim 0), LeakyReLU(0.2)
 * after every layer but the last.  fp32 in, fp32 accumulate on the matrix pipe (csrc/critic_kernels.hip).
 *   x    [B][C0][F0] fp32 contiguous: the layout of ntm_spectrogram's P, or of the mel product.  log_floor > 0: the first
 *        layer reads log10(max(x, log_floor)) as it loads x (SpecCrit(log=True)); log_floor == 0: x as it is.
 *   g, v, bias (and dg, dv, dbias): HOST arrays of n_layers DEVICE pointers -- g[l] [c_out], v[l] [c_out][c_in/groups][k],
 *        bias[l] [c_out], the separate tensors a module owns.
 *   out, gout  [B][c_out of the last layer][F_out], F_out = F0 - sum (k - 1).
 *   saved  ntm_speccrit_saved_floats(...) floats the forward fills and the backward of the SAME sizes and parameters reads:
 *        2 W + R + sum_{l < n-1} B c_out[l] F[l+1], with W = sum c_out (c_in/groups) k (the effective weights in the two
 *        layouts the kernels read), R = sum c_out (1/|v|), then the post-activation output of every layer but the last (it is
 *        the next layer's input; the LeakyReLU slope is recovered from its sign, y > 0 <=> pre > 0, and y == 0 takes 0.2).
 *   ws   ntm_speccrit_workspace_floats(...) floats of device scratch for the backward: 2 max_{l < n-1} B c_out[l] F[l+1]
 *        + min(B, 32)' (W + R), min(B, 32)' = ceil(B / ceil(B / min(B, 32))) the number of stream chunks of the weight gradient.
 *   gx   [B][C0][F0] or NULL: no input gradient (the first layer's data-gradient kernel is skipped).  With the log head
 *        gx = gX / (x ln 10) where x >= log_floor (it passes at equality: torch's clamp), else 0.
 *   dg   NULL: no parameter gradients (dv and dbias are then not looked at).  Gradients are stored, not accumulated.
 * No floating-point atomics: the weight gradient adds the streams of a chunk in order inside a workgroup and the chunks in order
 * afterwards, so equal calls give equal bits; a stream's out and gx do not depend on the batch it is in.  Refused (-1 from the
 * two size functions; NTM_EINVAL and a message starting with the function's name from the others) before anything touches a
 * device: null pointers, n_layers outside [1, 8], a channel count outside [1, 1024] (C0 alone may be
 * 1025, the bins of ntm_spectrogram's largest transform), k outside [1, 64], groups not dividing
 * both channel counts, c_in of a layer not c_out of the one before it (C0 for the first), a k larger than the frames that
 * reach it, B * C * F >= 2^31 for any tensor of the stack, a negative or NaN log_floor.  B == 0 returns NTM_OK without looking
 * at the device pointers (the size functions then count the weights alone).
 */
typedef struct { int32_t c_in, c_out, k, groups; } ntm_conv1d_layer;      /* stride 1, dilation 1, no padding */
int64_t ntm_speccrit_saved_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer *layers);
int64_t ntm_speccrit_workspace_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer *layers);
int ntm_speccrit_forward(const float *x, int64_t B, int64_t C0, int64_t F0, float log_floor, int n_layers,
                         const ntm_conv1d_layer *layers, const float *const *g, const float *const *v, const float *const *bias,
                         float *saved, float *out, void *stream);
int ntm_speccrit_backward(const float *x, int64_t B, int64_t C0, int64_t F0, float log_floor, int n_layers,
                          const ntm_conv1d_layer *layers, const float *const *g, const float *const *v,
                          const float *saved, const float *gout, float *gx, float *const *dg, float *const *dv,
                          float *const *dbias, float *ws, void *stream);

/*
 * The conv stack of the reference's time-domain critic (`DilatedConvDisc`, code/critics.py:262-331), forward and backward: the
 * ntm_speccrit family with a dilation per layer, up to 16 layers, a LeakyReLU slope passed by the caller and no log head.
 * n_layers weight-normed Conv1d(c_in, c_out, k, groups, dilation) with stride 1 and no padding, frames shrinking as
 * F[l+1] = F[l] - (k - 1) dilation; effective weight w = g v / |v| (the norm over (c_in/groups, k) per output channel);
 * LeakyReLU(slope) after every layer but the last.  fp32 in, fp32 accumulate on the matrix pipe (csrc/convstack_kernels.hip).
 *   x    [B][C0][F0] fp32 contiguous (the waveform: C0 = 1).
 *   g, v, bias (and dg, dv, dbias): HOST arrays of n_layers DEVICE pointers, as in the ntm_speccrit family.
 *   out, gout  [B][c_out of the last layer][F_out], F_out = F0 - sum (k - 1) dilation.
 *   saved  ntm_convstack_saved_floats(...) floats the forward fills and the backward of the SAME sizes, slope and parameters
 *        reads: 2 W + R + sum_{l < n-1} B c_out[l] F[l+1], with W = sum c_out (c_in/groups) k, R = sum c_out, as in the
 *        ntm_speccrit family (the slope's side is recovered from the sign of the saved output: y > 0 <=> pre > 0 because
 *        slope > 0, and y == 0 takes the slope).
 *   ws   ntm_convstack_workspace_floats(...) floats of device scratch for the backward:
 *        2 max_{l < n-1} B c_out[l] F[l+1] + sum_l min(B, 32)' ceil(F[l+1] / 1024) (W_l + c_out[l]),
 *        W_l = c_out (c_in/groups) k of layer l.  The chunk rule of the weight gradient: the streams are cut into
 *        min(B, 32)' = ceil(B / ceil(B / min(B, 32))) contiguous chunks (as in the ntm_speccrit family; none for B == 0) and the
 *        output frames of layer l into segments of 1024; one workgroup per (stream chunk, segment) adds its streams in
 *        order and its frames in order (256 frames from 0 at a time, then to its total) and stores one partial; the partials
 *        are added stream chunk major, segment minor.
 *   gx   [B][C0][F0] or NULL: no input gradient (the first layer's data-gradient kernel is skipped).
 *   dg   NULL: no parameter gradients (dv and dbias are then not looked at).  Gradients are stored, not accumulated.
 * No floating-point atomics: equal calls give equal bits; a stream's out and gx do not depend on the batch it is in.  Refused
 * (-1 from the two size functions; NTM_EINVAL and a message starting with the function's name from the others) before
 * anything touches a device: null pointers, n_layers outside [1, 16], a channel count outside [1, 1024], k outside [1, 64],
 * dilation outside [1, 2^20], groups not dividing both channel counts, c_in of a layer not c_out of the one before it (C0 for
 * the first), a layer whose (k - 1) dilation + 1 is larger than the frames that reach it, B * C * F >= 2^31 for any tensor of
 * the stack, a slope outside (0, 1) or NaN (forward and backward).  B == 0 returns NTM_OK without looking at the device
 * pointers (the size functions then count the weights alone).  Additions within ABI version 9: ntm_conv1d_layer and the
 * ntm_speccrit entry points are unchanged.
 */
typedef struct { int32_t c_in, c_out, k, groups, dilation; } ntm_conv1d_layer_d;   /* stride 1, no padding */
int64_t ntm_convstack_saved_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_d *layers);
int64_t ntm_convstack_workspace_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_d *layers);
int ntm_convstack_forward(const float *x, int64_t B, int64_t C0, int64_t F0, float slope, int n_layers,
                          const ntm_conv1d_layer_d *layers, const float *const *g, const float *const *v, const float *const *bias,
                          float *saved, float *out, void *stream);
int ntm_convstack_backward(const float *x, int64_t B, int64_t C0, int64_t F0, float slope, int n_layers,
                           const ntm_conv1d_layer_d *layers, const float *const *g, const float *const *v,
                           const float *saved, const float *gout, float *gx, float *const *dg, float *const *dv,
                           float *const *dbias, float *ws, void *stream);

/*
 * The conv stack of the reference's MelGAN critic (`MelGCrit` / `NLayerDiscriminator`, code/critics.py:18-122), forward and
 * backward: n_layers weight-normed Conv1d(c_in, c_out, k, groups, stride, pad) with dilation 1, frames following
 * F[l+1] = floor((F[l] + 2 pad - k) / stride) + 1; effective weight w = g v / |v| (the norm over (c_in/groups, k) per output
 * channel); LeakyReLU(slope) after every layer but the last.  pad_mode 0: frames outside the input read zero; pad_mode 1: they
 * read the mirrored sample (torch's ReflectionPad1d(pad) in front of the conv), on the FIRST layer only.  The output of EVERY
 * layer is returned, and a gradient may arrive at every one of them.  fp32 in, fp32 accumulate on the matrix pipe
 * (csrc/sconv_kernels.hip).
 *   x    [B][C0][F0] fp32 contiguous (the waveform: C0 = 1).
 *   g, v, bias (and dg, dv, dbias): HOST arrays of n_layers DEVICE pointers, as in the ntm_speccrit family.
 *   outs   HOST array of n_layers DEVICE pointers, outs[l] [B][c_out[l]][F[l+1]]: the post-activation output of layer l (the
 *        bare conv output for the last).  They are the activations the backward reads: hand it the same tensors, unchanged
 *        (the slope's side is recovered from the sign: y > 0 <=> pre > 0 because slope > 0, and y == 0 takes the slope).
 *   gouts  HOST array of n_layers DEVICE pointers in outs' shapes; an entry may be NULL (no gradient arrives at that output),
 *        at least one is not.  Layers above the highest non-NULL entry get exact zeros in dg, dv and dbias and no kernel.
 *   saved  ntm_sconvstack_saved_floats(...) floats the forward fills and the backward of the SAME sizes, slope and parameters
 *        reads: 2 W + R, W = sum c_out (c_in/groups) k (the effective weights in the two layouts the kernels read), R = sum
 *        c_out (1/|v|).  No activations.
 *   ws   ntm_sconvstack_workspace_floats(...) floats of device scratch for the backward:
 *        2 max_l B c_out[l] F[l+1]  +  (layer 0 reflected with pad > 0: B C0 (F0 + 2 pad), else 0)
 *        +  sum_l nchunk_l nseg_l (W_l + c_out[l]),   W_l = c_out (c_in/groups) k of layer l.
 *        The chunk rule of the weight gradient, a function of the sizes only, per layer (Fo = F[l+1]):
 *          seg    = 1024, doubled while ceil(Fo / seg) > 1 and ceil(Fo / seg) W_l > 2^24   (frames per segment)
 *          nseg   = ceil(Fo / seg)
 *          per    = max(ceil(B / 32), ceil(2048 / min(Fo, seg)), ceil(B / max(1, floor(2^24 / (nseg W_l))))), at most B
 *          nchunk = ceil(B / per)   (0 for B == 0)
 *        so a partial sums at least 2048 frames where the layer has them (a layer of 64 output frames at B = 16 is ONE partial,
 *        not 16), there are at most 32 stream chunks, and the partials of a layer stay within 2^24 floats (64 MiB) unless one
 *        partial alone is larger.  One workgroup per (stream chunk, segment) adds its streams in order and its frames in order
 *        (256 frames from 0 at a time, then to its total) and stores one partial; the partials are added stream chunk major,
 *        segment minor.
 *   gx   [B][C0][F0] or NULL: no input gradient (the first layer's data-gradient kernel is skipped).  Under a reflected first
 *        layer the border terms are added back in a fixed order: interior, left mirror, right mirror.
 *   dg   NULL: no parameter gradients (dv and dbias are then not looked at).  Gradients are stored, not accumulated.
 * No floating-point atomics: equal calls give equal bits; a stream's outputs and gx do not depend on the batch it is in.  Refused
 * (-1 from the two size functions; NTM_EINVAL and a message starting with the function's name from the others) before
 * anything touches a device: null pointers, n_layers outside [1, 16], a channel count outside [1, 1024], k outside [1, 64],
 * stride outside [1, 64], pad outside [0, k - 1], a pad_mode other than 0 or 1, pad_mode 1 on a layer other than the first or
 * with pad >= F0, groups not dividing both channel counts, c_in of a layer not c_out of the one before it (C0 for the first), a
 * layer with no output frame (F + 2 pad < k), B * C * F >= 2^31 for any tensor of the stack (the padded first input included),
 * B ceil(F[l+1] / 64) or B stride ceil(ceil((F[l] + pad) / stride) / 64) >= 2^24 for any layer (the workgroups of one launch; a
 * reflected first layer counts F0 + 2 pad), a
 * slope outside (0, 1) or NaN (forward and backward), gouts with every entry NULL.  B == 0 returns NTM_OK without looking at the
 * device pointers (the size functions then count the weights alone).  Additions within ABI version 9.
 */
typedef struct { int32_t c_in, c_out, k, groups, stride, pad, pad_mode; } ntm_conv1d_layer_s;   /* pad_mode 0 zeros, 1 reflect */
int64_t ntm_sconvstack_saved_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_s *layers);
int64_t ntm_sconvstack_workspace_floats(int64_t B, int64_t C0, int64_t F0, int n_layers, const ntm_conv1d_layer_s *layers);
int ntm_sconvstack_forward(const float *x, int64_t B, int64_t C0, int64_t F0, float slope, int n_layers,
                           const ntm_conv1d_layer_s *layers, const float *const *g, const float *const *v,
                           const float *const *bias, float *saved, float *const *outs, void *stream);
int ntm_sconvstack_backward(const float *x, int64_t B, int64_t C0, int64_t F0, float slope, int n_layers,
                            const ntm_conv1d_layer_s *layers, const float *const *g, const float *const *v,
                            const float *saved, const float *const *outs, const float *const *gouts, float *gx,
                            float *const *dg, float *const *dv, float *const *dbias, float *ws, void *stream);

/*
 * "Next" row N2 plumbing: pitched asynchronous copy between (pinned) host memory and the device, rows x
 * width_bytes with independent pitches -- what the segment feeder uses to send a TIME CHUNK of many segments
 * ([B, c0:c1] of a [B,T] batch) so that the copy of chunk c+1 overlaps the GRU launch on chunk c.
 * kind 0: host -> device, 1: device -> host.  Thin wrapper of hipMemcpy2DAsync on `stream`.
 */
int ntm_copy2d_async(void *dst, int64_t dst_pitch_bytes, const void *src, int64_t src_pitch_bytes,
                     int64_t width_bytes, int64_t rows, int kind, void *stream);

/*
 * "Next" row N3: DelayAnalyzer.demodulate, code/utilities/utilities.py:408-465 -- removes the time-varying
 * delay of a recording using the pulse indices of its pilot channel.  x, out: [C,N] fp32 device (out must not
 * alias x); y_idx [P] int64 device = output pulse indices (strictly increasing, P >= 2);
 * period = int(mean(diff(input pulse indices))) and shift = y_idx[0] - x_idx[0] are computed by the caller from
 * the INPUT pulse indices (:436, :458); scratch holds N doubles.  Interpolation runs in fp64 with scipy's
 * formulas, results are rounded to fp32 on store.
 */
int ntm_demodulate(const float *x, float *out, int C, int64_t N, const int64_t *y_idx, int P, int64_t period,
                   int64_t shift, double *scratch, void *stream);

/*
 * Record-head field of the reference's tape simulator, the stage in front of H_mag: I_rec = I + bias
 * (code/tape.py:476-510; bias [N] fp64 is shared by all streams, NULL = bias disabled) and
 * H = (gain * I_rec) / gap with gain = REC_N * REC_E, gap = REC_G (:512-514).  I, H: [B,N] fp64 device.
 */
int ntm_tape_record_field(const double *I, const double *bias, double *H, int64_t B, int64_t N, double gain,
                          double gap, void *stream);

/*
 * "Next" row N4: replaces Tape.H_mag, code/tape.py:516-551 (Jiles-Atherton hysteresis, RK4, fp64) of the
 * reference's white-box tape simulator.  H, M: [B,N] fp64 device, contiguous (oversampled rate);
 * state [B,3] fp64 device = (M_prev, H_prev, Hprime_prev), read and updated (zeros initially, :303-309);
 * Ts = 1/(fs*oversampling); params5 is a HOST array {Ms, A, alpha, K, c} (code/tape.py:251-256).
 */
int ntm_tape_hmag(const double *H, double *M, int64_t B, int64_t N, double *state, double Ts,
                  const double *params5, void *stream);

/*
 * The resamplers of Tape.__call__ (code/tape.py:330-332,471-474,553-558: torchaudio.transforms.Resample -- sinc
 * interpolation, Hann window, lowpass_filter_width 6, rolloff 0.99; torchaudio is un-vendored and absent here: the
 * published algorithm, parity unpinned).  Polyphase FIR in fp64 with a caller-supplied kernel table (device,
 * [up][2*width + down], built by ntm_amd.tape.sinc_resample_kernel):
 *   y[b][i*up + p] = sum_k kernel[p][k] * xpad[b][i*down + k],  xpad[j] = x[j - width] (zero outside [0, N)),  i*up + p < M.
 * x [B,N], y [B,M] fp64 device, contiguous.
 */
int ntm_resample_fir(const double *x, double *y, int64_t B, int64_t N, int64_t M, int up, int down, int width,
                     const double *kernel, void *stream);

/*
 * The playback-loss filter of Tape.H_play (code/tape.py:565-574: torchaudio.functional.lfilter with a = [1, 0, ...],
 * i.e. a FIR; clamp != 0 limits the output to [-1, 1] as lfilter's default does; zero initial state every call, as in the
 * reference):  y[b][n] = sum_{k < taps, k <= n} h[k] x[b][n-k].   x, y [B,N] fp64 device; h [taps] fp64 device.
 */
int ntm_fir_f64(const double *x, double *y, int64_t B, int64_t N, const double *h, int taps, int clamp, void *stream);

/*
 * Builder-defined causal dilated-Conv1d TCN (BASELINE.json config 4; the reference has no TCN:
 * code/micro_tcn is an empty submodule).  L causal blocks  out = PReLU(conv_dilated(in)) + conv1x1(in),
 * then a 1x1 conv to one channel.  params (device), block after block:
 *   W[C_in][K][C], b[C], alpha[C], R[C_in][C]   (C_in = 1 for block 0, C afterwards), then out_w[C], out_b[1].  x,y [B,T] contiguous; dil[L] host array; `scratch`
 * holds ntm_tcn_scratch_floats(B,T,C) floats (two activation buffers, each padded by one 16-row block: always ask this
 * function).  A batch whose activations exceed 8 GB is worked through in chunks of ntm_tcn_chunk_streams(B,T,C) streams
 * (streams are independent; same results bit for bit): the scratch never exceeds 2e9 floats (+ padding) whatever B is --
 * 8 GB for 32 768 x 65 536 instead of 2 x 275 GB.  Chunks alternate between two lanes, each with its own pair of
 * activation buffers inside `scratch` and its own HIP stream, forked from and joined to `stream` by events (the two side
 * streams and three events are created on the first chunked call on a device and kept -- the library's only state, it
 * holds no data): the call returns as soon as the work is enqueued, is ordered on `stream` like any other, and one
 * chunk's drain and HBM-bound first block run under the other chunk's matrix-pipe blocks.  A call made while `stream` is
 * being CAPTURED into a graph does not touch the shared lanes: its chunks are enqueued one after the other on `stream`
 * itself (same results; the lanes belong to every caller on the device, and a lane forked into one capture would pull
 * another thread's concurrent call into it).  Limits: T < 2^31 - 2^25,
 * 1 <= dil[l] <= 2^20 (NTM_EINVAL otherwise).
 */
int ntm_tcn_forward(const float *params, int L, int C, int K, const int *dil, const float *x,
                    float *y, int64_t B, int64_t T, float *scratch, void *stream);
int64_t ntm_tcn_scratch_floats(int64_t B, int64_t T, int C);
int64_t ntm_tcn_chunk_streams(int64_t B, int64_t T, int C);

/*
 * ---- Training of GRU-HS[64] (input_size = output_size = 1, no skip, exact fp32): what RNN.train_epoch of
 * code/model.py:90-161 needs, run by code/train.py:181-267 with --HIDDEN_SIZE 64 and --LOSS ESR | DCPreESR.  These entry
 * points were added without changing any existing one, so NTM_ABI_VERSION stays 9 (a caller of the version-9 ABI sees no
 * difference).  GRU as torch.nn.GRU defines it (code/model.py:44-45,80-82), with gh_n = W_hn h_{t-1} + b_hn.
 */
#define NTM_TRAIN_SAVED 5             /* saved floats per step and unit: h_{t-1}, r, z, n, gh_n                          */
#define NTM_TRAIN_GRAD_FLOATS 12929   /* w_ih 192 | w_hh 12288 | b_ih 192 | b_hh 192 | w_o 64 | b_o 1                    */

/* Floats of the workspace ntm_gru_train_forward fills for B streams of T samples: B * T * NTM_TRAIN_SAVED * 64. */
int64_t ntm_gru_train_workspace_floats(int64_t B, int64_t T);

/*
 * The forward of one TBPTT window with its activations saved (the `pred_mini = self.forward(input_mini)` of
 * code/model.py:133-134 and the warm-up forward of :122, both under autograd): ntm_gru_forward_ex with NTM_GRU_LAT for
 * H = 64, input / output size 1 -- y and h_state come out bit-identical to it -- plus, for every step t and unit u,
 * ws[((b*T + t)*5 + j)*64 + u] = h_{t-1}, r, z, n, gh_n (j = 0..4; contiguous, ntm_gru_train_workspace_floats(B, T)).
 * h_state [B,64] in / out (null: zero initial state, final state not written).  b_o may be null.
 */
int ntm_gru_train_forward(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                          const float *b_o, const float *x, float *y, int64_t B, int64_t T, int64_t x_stride_b,
                          int64_t y_stride_b, float *h_state, float *ws, void *stream);

/*
 * Backward through time of that window (the `loss.backward()` of code/model.py:140), one workgroup per stream, t = T-1 .. 0.
 * dy [B,T] (row stride dy_stride_b; null = zeros) is dL/dy, dh_T [B,64] the gradient of the final hidden state (null =
 * zeros; it chains a window to the one after it), ws the workspace of the forward.  Out: dh0 [B,64] (the gradient of the
 * initial state; may be null) and part [B, NTM_TRAIN_GRAD_FLOATS], every stream's own parameter gradients.
 */
int ntm_gru_train_backward(const float *w_hh, const float *w_o, const float *x, int64_t x_stride_b, const float *ws,
                           const float *dy, int64_t dy_stride_b, const float *dh_T, int64_t B, int64_t T, float *dh0,
                           float *part, void *stream);

/* grad[NTM_TRAIN_GRAD_FLOATS] = the B rows of part added in stream order (fp64 accumulation, no atomics: bit-reproducible). */
int ntm_gru_train_reduce(const float *part, int64_t B, float *grad, void *stream);

/*
 * Adjoint of the ESRLoss of code/train.py:176 on the whole [B,T] tensor (contiguous):
 *     dy = gout[0] * 2 (y - t) / (n (S_t / n + eps)),   n = B T,
 * sums2 = the whole-batch [S_e, S_t] (fp64, device: the stream rows of ntm_esr_sums added up), gout the upstream gradient
 * (one float, device), eps = 1e-5 (CoreAudioML).
 */
int ntm_esr_grad(const float *y, const float *t, int64_t B, int64_t T, const double *sums2, const float *gout, double eps,
                 float *dy, void *stream);

/*
 * Adjoint of the DCPreESR(dc_pre=True) loss of code/train.py:174 (the sums of ntm_esr_dcpre_sums with skip 0): with
 * e_f = H(y - t), H(z) = (1 - z^-1)/(1 - R z^-1) from zero state, and v = gout[0] * 2 e_f / (n (S_tf / n + eps)),
 * dy = H^T v -- the anti-causal one-pole q[t] = v[t] + R q[t+1] followed by dy[t] = q[t] - q[t+1].  sums2 = the whole-batch
 * [S_ef, S_tf] of ntm_esr_dcpre_sums.
 */
int ntm_esr_dcpre_grad(const float *y, const float *t, int64_t B, int64_t T, float R, const double *sums2, const float *gout,
                       double eps, float *dy, void *stream);

/*
 * ---- R replicas of that training configuration in one launch each (additions within ABI version 9): what an array of
 * independent runs of one configuration (scripts/sbatch-train-exp1a.sh:7-15, --array=0-2) needs on one device.  The streams
 * are stacked replica-major -- stream s of R * Bper belongs to replica s / Bper -- and the parameters arrive as contiguous
 * stacks: w_ih [R,192,1], w_hh [R,192,64], b_ih, b_hh [R,192], w_o [R,1,64], b_o [R,1] (may be null).  Everything is per
 * stream and free of atomics, so every replica's outputs are bit-identical to those of the single-model entry point above
 * called on that replica's slice with that replica's parameters.  R and Bper must be positive (R <= 65535).
 * The reduction and the two loss adjoints are the same kernels either way: ntm_gru_train_reduce, ntm_esr_grad and
 * ntm_esr_dcpre_grad run them with R = 1, Bper = B (and, unlike the calls below, accept B = 0).
 */

/* ntm_gru_train_forward for R replicas: x, y, h_state [R*Bper, .], ws = ntm_gru_train_workspace_floats(R * Bper, T). */
int ntm_gru_train_forward_replicas(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                                   const float *b_o, const float *x, float *y, int64_t R, int64_t Bper, int64_t T,
                                   int64_t x_stride_b, int64_t y_stride_b, float *h_state, float *ws, void *stream);

/* ntm_gru_train_backward for R replicas: dh0 [R*Bper,64] (may be null), part [R*Bper, NTM_TRAIN_GRAD_FLOATS]. */
int ntm_gru_train_backward_replicas(const float *w_hh, const float *w_o, const float *x, int64_t x_stride_b, const float *ws,
                                    const float *dy, int64_t dy_stride_b, const float *dh_T, int64_t R, int64_t Bper, int64_t T,
                                    float *dh0, float *part, void *stream);

/* grad[R, NTM_TRAIN_GRAD_FLOATS]: row r = the Bper rows of replica r added in stream order in fp64 (ntm_gru_train_reduce's order). */
int ntm_gru_train_reduce_replicas(const float *part, int64_t R, int64_t Bper, float *grad, void *stream);

/*
 * sums2[R,2] fp64 from the per-stream rows of ntm_esr_sums (rows [R*Bper, splits, 2]) or ntm_esr_dcpre_sums (splits = 1):
 * per replica the `splits` (<= 255) partial rows of each stream, then the Bper stream sums, both in the fixed order given in
 * csrc/gru_train.hip -- the order in which ESRLoss / DCPreESR add them for one model, so the same bits.
 */
int ntm_loss_sums_replicas(const double *rows, int64_t R, int64_t Bper, int splits, double *sums2, void *stream);

/* ntm_esr_grad for R losses: every element takes sums2[r], gout[r] and n = Bper T of its replica; y, t, dy [R*Bper, T] contiguous. */
int ntm_esr_grad_replicas(const float *y, const float *t, int64_t R, int64_t Bper, int64_t T, const double *sums2, const float *gout,
                          double eps, float *dy, void *stream);

/* ntm_esr_dcpre_grad for R losses (pole: the DC blocker's R). */
int ntm_esr_dcpre_grad_replicas(const float *y, const float *t, int64_t R, int64_t Bper, int64_t T, float pole, const double *sums2,
                                const float *gout, double eps, float *dy, void *stream);

/*
 * Inference for R replicas (the `validate` / `predict` half of the epoch loop, code/train.py:238-267, for models trained side by
 * side): ntm_gru_forward_ex with NTM_GRU_LAT for H = 64, input / output size 1, on R * Bper streams stacked replica-major with
 * the parameter stacks described above -- y [R*Bper, T] (row strides in elements, >= T) and h_state [R*Bper, 64] (in / out; null:
 * zero initial state, final state not written) of replica r are bit-identical to that call on r's slice with r's parameters,
 * and R = 1 IS that call.  b_o may be null.  One launch; always the low-latency kernel (a workgroup per stream), for any
 * R * Bper: NTM_GRU_AUTO's hand-over to the matrix-pipe kernel above NTM_GRU_LAT_MAX_B streams does not happen here.
 * NTM_EINVAL before anything is enqueued: R < 1, Bper < 1, T < 0, a null required pointer, a stride below T, y == x.
 */
int ntm_gru_forward_replicas(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                             const float *b_o, const float *x, float *y, int64_t R, int64_t Bper, int64_t T, int64_t x_stride_b,
                             int64_t y_stride_b, float *h_state, void *stream);

/*
 * Adjoint of the time-varying fractional delay line (ntm_delay_forward) over one call of B streams of L samples with a buffer of
 * D samples (the backward of DiffDelRNN.train_epoch's delay step, code/model.py:269-320,456-496).  With z = [buffer, x] the
 * forward is y[n] = sum_m w_m(n) z[D + n - m] over the taps m in {k+1, k}, k = floor(d[n]), that it counts, and the new buffer
 * is z[L : L + D]; warmup: y = x.  Writes gz = [gbuf (D), gpre (L)] per stream:
 *     gz[i] = g_newbuf[i - L] (i >= L) + the terms w_m(n) gy[n] with D + n - m = i, added in ascending n.
 * gy [B,L] (null: no gradient from y), d [B,L] in samples (read unless warmup; no gradient flows to it), g_newbuf [B,D] (null:
 * none), gpre [B,L], gbuf [B,D] (null: not computed).  All contiguous fp32.  Deterministic: repeated calls give the same bits.
 * flags: 0, or NTM_DELAY_BWD_SCAN to take the general path for every tile (it gives the same bits as the default one).
 */
#define NTM_DELAY_BWD_SCAN 1
int ntm_delay_backward(const float *gy, const float *d, const float *g_newbuf, float *gpre, float *gbuf, int64_t B, int64_t L,
                       int D, int warmup, int flags, void *stream);

/*
 * ---- DiffDelRNN block by block (additions within ABI version 9): what a real-time host needs to advance B streams of
 * DiffDelRNN(1, 64, 1, skip=False) by `block` samples per call with ONE launch and O(block) traffic of delay state per stream.
 * The delay line's history lives in a caller-owned ring per stream, ring [B, C] floats with C = ntm_diffdel_stream_ring_floats(D,
 * block) (a power of two >= D + block), beside a sample counter pos [B] (int64, device) that only the kernel reads and advances:
 * no host-side position, so the block call can be captured into a graph and replayed.  Sample i of a stream, counted from the
 * ring's origin, is ring[b][i mod C]; the reference's buffer (dl_state of ntm_delay_forward, oldest first) is samples
 * pos - D .. pos - 1.
 */

/* Floats per stream of the ring for a delay line of D samples advanced `block` samples per call; 0 for a negative argument. */
int64_t ntm_diffdel_stream_ring_floats(int D, int64_t block);

/* ring, pos <- the reference's buffer dl_state [B,D] (contiguous): samples 0 .. D-1, pos = D.  C as above for the block size
 * that will follow (any power of two >= D is accepted here).  B == 0 is a successful no-op. */
int ntm_diffdel_stream_seed(const float *dl_state, float *ring, int64_t *pos, int64_t B, int D, int64_t C, void *stream);

/* dl_state [B,D] <- the reference's buffer as the ring holds it now (what DiffDelRNN's delay line would carry after the same calls). */
int ntm_diffdel_stream_export(const float *ring, const int64_t *pos, float *dl_state, int64_t B, int D, int64_t C, void *stream);

/*
 * One block of DiffDelRNN.forward(x, del_traj, warmup) (code/model.py:393-424) in one launch, a workgroup per stream: the
 * low-latency GRU step with the bias-free head gives pre_d, the delay line reads its taps from the ring and writes y.
 * x [B,block] (row stride x_stride_b), d [B,block] in samples (d_stride_b), y and pre_d [B,block] (both y_stride_b; pre_d may
 * be NULL: not returned); h_state [B,64] in / out, ring / pos as above with C >= D + block, all required.
 * pre_d and h_state are the bits of ntm_gru_forward_ex with NTM_GRU_LAT on the same block, y the bits of ntm_delay_forward on
 * that pre_d and the exported buffer, for every block size and any split of a signal into blocks.  warmup != 0: y = pre_d,
 * the ring and pos move on (code/model.py:288-292).  err_flag (device int32, may be NULL) is raised to 1 by any d > D or NaN
 * d, as in ntm_delay_forward; unlike there nothing is frozen: from the violating call on y, pre_d and the streamer's own state
 * (h_state, ring, pos) are unspecified until the caller seeds them again -- nothing else is touched.
 * B == 0 or block == 0 is a successful no-op.  y, pre_d must not alias x, d or each other.
 */
int ntm_diffdel_stream_block(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *w_o,
                             const float *x, const float *d, float *y, float *pre_d, int64_t B, int64_t block,
                             int64_t x_stride_b, int64_t d_stride_b, int64_t y_stride_b, float *h_state, float *ring, int64_t C,
                             int64_t *pos, int D, int warmup, int32_t *err_flag, void *stream);

/*
 * ---- The hinge / mean heads of the adversarial losses (additions within ABI version 9): what code/critics.py's train_crit and
 * train_gen evaluate on the K outputs of a critic, as one node.  outs: host array of K device pointers, output k a contiguous
 * fp32 tensor of `rows` rows of elems[k] floats (elems: host array); K in [1, NTM_ADV_HEAD_MAX_K], rows and every elems[k] >= 1.
 *   NTM_ADV_HEAD_CRIT  rows [0, n_fake) are fake with the terms relu(fp32(1 + o)), rows [n_fake, rows) real with
 *                      relu(fp32(1 - o)); 0 < n_fake < rows; every half of every output has a mean of its own and
 *                          loss = sum_k mean(fake terms of k) + sum_k mean(real terms of k);
 *   NTM_ADV_HEAD_GEN   loss = sum_k -mean(o_k) over all rows (n_fake is not read).
 * The terms are formed in fp32 and summed in fp64 in a fixed order: chunks of NTM_ADV_HEAD_CHUNK terms over workgroups, then
 * the chunk sums in a second, single-workgroup launch.  No atomics: equal calls give equal bits.  Every mean is rounded to fp32
 * once and the means are added in fp32 in the order written above, as the reference adds them.
 * ws: device workspace of ws_doubles >= (K or, in the critic mode, 2 K) * ceil(longest half in floats / NTM_ADV_HEAD_CHUNK)
 * doubles; loss: one device float.  Two launches, nothing else.
 */
#define NTM_ADV_HEAD_CRIT 0
#define NTM_ADV_HEAD_GEN 1
#define NTM_ADV_HEAD_MAX_K 8
#define NTM_ADV_HEAD_CHUNK 4096
int ntm_adv_head_forward(const float *const *outs, const int64_t *elems, int K, int64_t rows, int64_t n_fake, int mode, double *ws,
                         int64_t ws_doubles, float *loss, void *stream);

/*
 * Its adjoint in one launch: grads[k] (host array of K device pointers, each of output k's size, all written) receives
 *     fake rows  +c_k [fp32(1 + o) > 0],   real rows  -c_k' [fp32(1 - o) > 0],   generator mode  -c_k,
 * with c = gout[0] * (1.0f / fp32(floats of that half)): the arithmetic of torch's autograd on the reference's expression (its
 * mean divides by a host scalar, which torch evaluates as a product with the fp32 reciprocal), so the gradients are its bits;
 * the mask is torch's relu mask, zero at a term of exactly 0 and one at a NaN.  gout: the upstream gradient, one device float.
 * grads[k] must not alias outs[k].
 */
int ntm_adv_head_backward(const float *const *outs, const int64_t *elems, int K, int64_t rows, int64_t n_fake, int mode,
                          const float *gout, float *const *grads, void *stream);

/*
 * ntm_delay_forward with the delays in float64 (an addition within ABI version 9): x, y [B,T] fp32, d [B,T] fp64 in samples,
 * dl_state [B,D] in / out, warmup and err_flag as there (a d > D or NaN raises the sticky flag and leaves y and dl_state of that
 * call unspecified / untouched respectively).  The weights 1 - |m - d| of the two taps and their products with the samples are
 * formed in float64, added in the reference's order and rounded to float32 once: what the reference's delay line returns, cast
 * to float32, when its data set hands float64 trajectories (code/train-adversarial.py with VADataset(double=True)).  A float32
 * delay of several hundred samples is 3e-5 to 6e-5 samples wide, which on a noise-like signal is 1e-5 at the output.
 * B <= 65535.  Two launches (the interpolation, one sample per thread; the buffer update of ntm_delay_forward).
 */
int ntm_delay_forward_f64(const float *x, const double *d, float *y, int64_t B, int64_t T, float *dl_state, int D, int warmup,
                          int32_t *err_flag, void *stream);

/*
 * The diffusion generators (`UNet1D`, code/networks/unet_1d.py, under `DiffusionGenerator`, code/model.py:656-891): the network's
 * fused blocks and the sampler's step, inference only (csrc/unet_kernels.hip).  Additions within ABI version 9.
 *
 * ntm_unet_resblock_forward: one ResnetBlock(bias=False, use_norm=False) in one launch (two in the tiled form):
 *     x = film * [src0 from frame off0 | src1 from frame off1]       the concatenation is never materialised; off0 is
 *                                                                    CropConcatBlock's centre crop
 *     y = W_first gelu(x);  n_layers times  y <- (y + Conv1d_{k = 5, dilation 2^l, "same", zeros}(gelu(y))) / sqrt 2
 *     out = (y + W_res x) / sqrt 2                                   W_res == NULL: the identity (c0 + c1 == c_out)
 *   src0 [B][c0][T0], src1 [B][c1][T1] (c1 == 0: NULL), out [B][c_out][T] fp32 contiguous; T frames are read from each source.
 *   init != 0: src0 is the waveform [B][1][T0] and its c0 channels are Conv1d(1, c0, 5, "same", zeros) of it with
 *     init_w [c0][5], computed on the fly (the network's init_conv).
 *   film [1 or B][c0 + c1] with film_stride floats between streams (0: one vector for all); w_first [c_out][c0 + c1];
 *   w_gated [n_layers][c_out][c_out][5]; w_res [c_out][c0 + c1] or NULL.  gelu is the exact (erf) one.
 *   form NTM_UNET_AUTO: the whole form for T <= NTM_UNET_WHOLE_MAX_T, else the tiled one; _WHOLE / _TILED force one.
 *     whole: one workgroup per stream holds the signal, no halo, one launch.
 *     tiled: windows of 1024 frames = a tile of NTM_UNET_TILE and a halo of 256 a side; a run of layers is one launch while
 *       2 sum(dilation) <= 256: layers 0-6 and layer 7 for the eight dilations 1 .. 128.  ws holds y between the runs:
 *       ntm_unet_resblock_workspace_floats(B, blk) floats (0 for one launch; -1 on arguments the forward refuses).
 *   Frames outside [0, T) are zero at every layer, as the reference's per-layer padding makes them.
 *   Contractions on v_mfma_f32_16x16x4_f32, fp32 accumulate.  Refused (NTM_EINVAL, a message starting with the function's
 *   name) before anything touches a device: null pointers, B outside [0, 65535], c0 < 1, c1 < 0, c0 + c1 > 32, c_out outside
 *   [1, 16], n_layers outside [1, 8], T < 1, a source shorter than off + T or a negative off, 32 T0 or 32 T1 >= 2^31, an unknown
 *   form, the whole form with T > NTM_UNET_WHOLE_MAX_T, film_stride neither 0 nor >= c0 + c1, W_res == NULL with
 *   c0 + c1 != c_out, out aliasing a source.  B == 0 returns NTM_OK.
 *
 * ntm_unet_down_combine: Downsample(S) of x [B][C][F] and pyr [B][1][F] by the polyphase FIR ker [taps], taps == 2 width + S
 *   (the module's `resample.kernel` buffer), then CombinerDown: x_out [B][C][Fo] = (wc[c] pyr_d + x_d) / sqrt 2, pyr_out
 *   [B][1][Fo] = pyr_d, Fo = ceil(F / S).
 * ntm_unet_up_combine: CombinerUp, p = sum_c wc[c] x[c] on [B][C][F], with a pyramid pyr [B][1][pyr_T >= F] p = (pyr[:F] + p) /
 *   sqrt 2; then Upsample(S) of x and p by the S phases ker [S][taps], taps == 2 width + 1: x_out [B][C][S F], pyr_out [B][1][S F].
 *   S == 1 (ker NULL, width == taps == 0, x_out NULL): the combiner alone, pyr_out [B][1][F].
 * ntm_unet_upsample: the upsampler alone on x [B][F] -> out [B][S F] (the sampler's 100 Hz -> 44.1 kHz resampler: S = 441).
 *   Refused: null pointers, B outside [0, 65535], C outside [1, 32], F < 1, S outside [1, 1024], width < 0, taps > 64 or not as
 *   stated, S F or C S F >= 2^31, pyr_T < F.  One launch each.
 *
 * ntm_edm_pre / ntm_edm_post: the sampler's step around the network on [B][T] fp32, every product and sum rounded on its own in
 *   the reference's order (code/model.py:797-837, 764-769):
 *     pre:  z' = z + eps_scale (eps snoise)            eps != NULL (the Schurn branch)
 *           z' = mask (x_out + n sigma0) + (1 - mask) z'     mask != NULL (outpainting; mask_stride 0: one row for all, else T)
 *           z_out = z', net_in = cin z'
 *     post: x0 = cskip z + cout F;  out = z - k ((x0 - z) / b2)        b2 = sigma^2, k = (sigma_next - sigma) sigma
 *   Refused: null z / z_out / net_in / F / out, mask without x_out and n, negative sizes, mask_stride neither 0 nor T.
 */
#define NTM_UNET_WHOLE_MAX_T 1024
#define NTM_UNET_TILE 512
#define NTM_UNET_AUTO 0
#define NTM_UNET_WHOLE 1
#define NTM_UNET_TILED 2
typedef struct {
    int32_t c0, c1, c_out, n_layers;
    int64_t T, T0, off0, T1, off1;
    int32_t init, form;
} ntm_unet_block;
int64_t ntm_unet_resblock_workspace_floats(int64_t B, const ntm_unet_block *blk);
int ntm_unet_resblock_forward(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                              const float *w_first, const float *w_gated, const float *w_res, int64_t B, const ntm_unet_block *blk,
                              float *ws, float *out, void *stream);
int ntm_unet_down_combine(const float *x, const float *pyr, const float *ker, const float *wc, int64_t B, int C, int64_t F, int S,
                          int width, int taps, float *x_out, float *pyr_out, void *stream);
int ntm_unet_up_combine(const float *x, const float *pyr, int64_t pyr_T, const float *ker, const float *wc, int64_t B, int C,
                        int64_t F, int S, int width, int taps, float *x_out, float *pyr_out, void *stream);
int ntm_unet_upsample(const float *x, const float *ker, int64_t B, int64_t F, int S, int width, int taps, float *out, void *stream);
int ntm_edm_pre(const float *z, const float *eps, float eps_scale, float snoise, const float *mask, int64_t mask_stride,
                const float *x_out, const float *n, float sigma0, float cin, int64_t B, int64_t T, float *z_out, float *net_in,
                void *stream);
int ntm_edm_post(const float *z, const float *F, float cskip, float cout, float b2, float k, int64_t N, float *out, void *stream);

/*
 * The whole sampler of a network whose every level fits the whole form, in ONE launch (csrc/unet_sampler.hip).  Additions
 * within ABI version 9.
 *
 * ntm_unet_sample_one_launch: n_steps times { ntm_edm_pre, the network's n_stages calls, ntm_edm_post } on B streams of T
 *   frames, one workgroup per stream (grid (1, B), 1024 threads) walking the steps and the stages with a workgroup barrier
 *   between them.  Every output is computed by the code of the step-by-step entry points above (one definition per output,
 *   csrc/unet_steps.h and csrc/unet_block.h), in their order of operations: z is bit-identical to running those entry points
 *   with the same operands.  Workgroups do not communicate and a workgroup touches only its own stream's rows.
 *   stages [n_stages] in HOST memory: the network's calls in launch order, read and checked by this entry point on every call;
 *   stages_dev: the same n_stages records in DEVICE memory, which the kernel walks (the caller copies them once).  A record:
 *     kind NTM_USTAGE_BLOCK  ntm_unet_resblock_forward(a = src0, b = src1, w3 = init_w, film, 0, w0 = w_first, w1 = w_gated,
 *                            w2 = w_res, B, &blk, NULL, o0 = out), blk of the whole form (form AUTO or WHOLE, T <= 1024), with
 *                            film = films + step film_len + film_off: c0 + c1 floats of the step's FiLM row, one vector for all
 *                            streams.  a == NULL: the network's input [B][1][T] (needs blk.init, blk.T0 == T)
 *          NTM_USTAGE_DOWN   ntm_unet_down_combine(a = x, b = pyr, w0 = ker, w1 = wc, B, C, F, S, width, taps, o0 = x_out,
 *                            o1 = pyr_out), F <= 1024.  b == NULL: the network's input (needs F == T)
 *          NTM_USTAGE_UP     ntm_unet_up_combine(a = x, b = pyr or NULL, pyr_T, w0 = ker, w1 = wc, B, C, F, S, width, taps,
 *                            o0 = x_out, o1 = pyr_out), S >= 2, F <= 1024, S F <= 2048
 *          NTM_USTAGE_FINAL  ntm_unet_up_combine with S == 1 (w0 == o0 == NULL, width == taps == 0): the last combiner.
 *                            o1 == NULL: the network's output [B][T] (needs F == T)
 *     Fields a kind does not name are ignored.  Every other pointer is a device pointer to a buffer of that entry point's
 *     layout for B streams; an intermediate is written by one stage and read by later ones, through vector loads.
 *   scal [n_steps][NTM_UNET_SAMPLE_SCALARS] fp32, per step: eps_scale, snoise, sigma0, cin (ntm_edm_pre's), cskip, cout, b2, k
 *     (ntm_edm_post's).  films [n_steps][film_len] fp32.  eps_steps: bit i set when step i has the eps draw.
 *   z0 [B][T]: the first latent.  draws [n_draws][B][T]: per step its eps draw (where eps_steps says so), then its outpainting
 *     noise n (with a mask, every step): n_draws == popcount(eps_steps below n_steps) + (mask ? n_steps : 0); NULL when 0.
 *   x_outpaint [B][T], mask [1 or B][T] with mask_stride 0 or T: ntm_edm_pre's, the same for every step; both NULL: no outpainting.
 *   ws: ntm_unet_sample_workspace_floats(B, T) = 3 B T floats (z after pre, the network's input, the network's output).
 *   z [B][T]: the sample; also the carry between steps, so it must not alias z0, the draws, x_outpaint, mask or ws.
 *   Refused (NTM_EINVAL) before anything touches a device, z untouched: null pointers, B outside [0, 65535], T outside [1, 1024],
 *   n_stages outside [1, NTM_UNET_SAMPLE_MAX_STAGES], n_steps outside [1, NTM_UNET_SAMPLE_MAX_STEPS], an unknown kind, a stage that
 *   its own entry point refuses or that breaks a bound stated above, film_off < 0 or film_off + c0 + c1 > film_len, n_draws not
 *   as stated, a mask without x_outpaint, mask_stride neither 0 nor T, z aliasing an input.  B == 0 returns NTM_OK.
 *   Dynamic LDS: the largest stage's (a block of 16 channels at 1024 frames: 143 360 bytes).  No scratch, no atomics.
 */
#define NTM_USTAGE_BLOCK 0
#define NTM_USTAGE_DOWN 1
#define NTM_USTAGE_UP 2
#define NTM_USTAGE_FINAL 3
#define NTM_UNET_SAMPLE_MAX_STAGES 64
#define NTM_UNET_SAMPLE_MAX_STEPS 64
#define NTM_UNET_SAMPLE_SCALARS 8
typedef struct {
    int32_t kind;                   /* NTM_USTAGE_* */
    int32_t C, S, width, taps;      /* the resample stages */
    int32_t film_off;               /* BLOCK: floats into the step's FiLM row */
    int64_t F, pyr_T;               /* the resample stages: input frames; UP / FINAL: the pyramid's row length */
    ntm_unet_block blk;             /* BLOCK */
    const float *a, *b, *w0, *w1, *w2, *w3;
    float *o0, *o1;
} ntm_unet_stage;                   /* 168 bytes */
int64_t ntm_unet_sample_workspace_floats(int64_t B, int64_t T);
int ntm_unet_sample_one_launch(const ntm_unet_stage *stages, const ntm_unet_stage *stages_dev, int n_stages, const float *scal,
                               const float *films, int64_t film_len, int n_steps, uint64_t eps_steps, const float *z0,
                               const float *draws, int n_draws, const float *x_outpaint, const float *mask, int64_t mask_stride,
                               int64_t B, int64_t T, float *ws, float *z, void *stream);

/*
 * Training of that network (code/train-diffusion.py): the ResnetBlock in its whole form (T <= NTM_UNET_WHOLE_MAX_T, form AUTO or
 * WHOLE) with its adjoint (csrc/unet_train.hip).  Additions within ABI version 9.  Operands and layouts are
 * ntm_unet_resblock_forward's; with y_0 = W_first gelu(x) and y_{l+1} = (y_l + conv_l(gelu(y_l))) / sqrt 2:
 *
 * ntm_unet_resblock_forward_save: the forward, which also writes y_0 .. y_{n_layers - 1} to ysave [B][n_layers][c_out][T],
 *   ntm_unet_resblock_save_floats(B, blk) floats.  out is bit-identical to ntm_unet_resblock_forward's whole form (one body).
 * ntm_unet_resblock_backward: from gout [B][c_out][T] and ysave, one workgroup per stream, two launches (the gated layers,
 *   last to first; then the 1x1s, FiLM and the sources) with gy_0 between them in ws [B][c_out][T] (B c_out T floats):
 *     g_src0 [B][c0][T0], g_src1 [B][c1][T1]   the sources' gradients, 0 at frames the block did not read; either may be NULL
 *                                              (not wanted); with init the waveform takes none and g_src0 must be NULL
 *     gfilm [B][c0 + c1]                       per stream (the caller sums the rows of a shared FiLM vector)
 *     partials [B][W][P]                       weight-gradient partials, one per stream and wave that owns frames:
 *                                              W = min(8, ceil(T / 16)), P = ntm_unet_resblock_wgrad_floats(blk) =
 *                                              n_layers c_out c_out 5 + 2 c_out (c0 + c1) + (init ? 5 c0 : 0), laid out as
 *                                              dW_gated | dW_first | dW_res (zeros without W_res) | dinit_w;
 *                                              ntm_unet_resblock_partial_floats(B, blk) = B W P floats
 * ntm_unet_wgrad_reduce: out[e] = sum_{p < count} partials[p n + e], e < n, added in index order in fp64, rounded once.
 *   No atomics anywhere: equal calls give equal bits, and a stream's g_src0, g_src1 and gfilm do not depend on its batch.
 *   The three size queries return -1 on arguments the entry points refuse.  Refused (NTM_EINVAL, before anything touches a
 *   device): what ntm_unet_resblock_forward refuses, T > NTM_UNET_WHOLE_MAX_T or the tiled form, null ysave / out / gout / ws /
 *   gfilm / partials, g_src0 with init, g_src1 with c1 == 0, negative count or n.  B == 0 returns NTM_OK.
 */
int64_t ntm_unet_resblock_save_floats(int64_t B, const ntm_unet_block *blk);
int64_t ntm_unet_resblock_wgrad_floats(const ntm_unet_block *blk);
int64_t ntm_unet_resblock_partial_floats(int64_t B, const ntm_unet_block *blk);
int ntm_unet_resblock_forward_save(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                                   const float *w_first, const float *w_gated, const float *w_res, int64_t B,
                                   const ntm_unet_block *blk, float *ysave, float *out, void *stream);
int ntm_unet_resblock_backward(const float *src0, const float *src1, const float *init_w, const float *film, int64_t film_stride,
                               const float *w_first, const float *w_gated, const float *w_res, int64_t B, const ntm_unet_block *blk,
                               const float *ysave, const float *gout, float *ws, float *g_src0, float *g_src1, float *gfilm,
                               float *partials, void *stream);
int ntm_unet_wgrad_reduce(const float *partials, int64_t count, int64_t n, float *out, void *stream);

/*
 * The same pair for the TILED form of the block, at any length (the upper levels of the noise net: 65 536 frames and more).
 * Additions within ABI version 9.  Operands, layouts and results are those of the whole-form namesakes; accepted are form
 * NTM_UNET_TILED at any T >= 1 and NTM_UNET_AUTO with T > NTM_UNET_WHOLE_MAX_T.  With tiles = ceil(T / NTM_UNET_TILE):
 *
 * ntm_unet_resblock_tiled_forward_save: the tiled forward in its runs of layers (ntm_unet_resblock_forward), which also writes
 *   y_0 .. y_{n_layers - 1} to ysave [B][n_layers][c_out][T] (ntm_unet_resblock_tiled_save_floats(B, blk) floats), every frame
 *   by the tile that owns it; y travels between the runs in the save itself, so there is no workspace.  out is bit-identical
 *   to ntm_unet_resblock_forward's tiled form (one body).
 * ntm_unet_resblock_tiled_backward: one workgroup per (tile, stream) on the forward's windows (the tile and 256 frames of halo a
 *   side: the gradient enters a run of layers over the window and leaves it exact on the tile).  The forward's runs last to
 *   first, then the 1x1s, FiLM and the sources per tile, then three fixed-order sums: 2 + 3 launches up to seven layers,
 *   3 + 3 for eight.
 *     ws        ntm_unet_resblock_tiled_workspace_floats(B, blk) floats: gy [B][c_out][T] between the launches (two such planes
 *               when the layers take two runs) and the gfilm partials [B][tiles][c0 + c1]
 *     gfilm     [B][c0 + c1], the partials of a stream's tiles added in tile order in fp64, rounded once
 *     partials  ntm_unet_resblock_tiled_partial_floats(B, blk) = B (1 + 9 tiles) P floats, P =
 *               ntm_unet_resblock_tiled_wgrad_floats(blk) = ntm_unet_resblock_wgrad_floats' formula: on return the FIRST B
 *               partials [B][P] are the per-stream sums (a tile's eight waves in wave order, then a stream's tiles in tile
 *               order, fp64 each, rounded once each), which ntm_unet_wgrad_reduce(partials, B, P, out) adds over the streams;
 *               behind them the per-tile and the per-(tile, wave) partials as the kernels wrote them
 *   No atomics anywhere: equal calls give equal bits, and a stream's g_src0, g_src1, gfilm and partial do not depend on its batch.
 *   The four size queries return -1 on arguments the entry points refuse.  Refused (NTM_EINVAL, a message starting with the
 *   function's name, before anything touches a device): what the whole-form pair refuses except the length -- and instead of
 *   the tiled form the whole one (NTM_UNET_WHOLE, NTM_UNET_AUTO with T <= NTM_UNET_WHOLE_MAX_T) -- and 8 B tiles >= 2^31.
 *   B == 0 returns NTM_OK.
 */
int64_t ntm_unet_resblock_tiled_save_floats(int64_t B, const ntm_unet_block *blk);
int64_t ntm_unet_resblock_tiled_workspace_floats(int64_t B, const ntm_unet_block *blk);
int64_t ntm_unet_resblock_tiled_wgrad_floats(const ntm_unet_block *blk);
int64_t ntm_unet_resblock_tiled_partial_floats(int64_t B, const ntm_unet_block *blk);
int ntm_unet_resblock_tiled_forward_save(const float *src0, const float *src1, const float *init_w, const float *film,
                                         int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res,
                                         int64_t B, const ntm_unet_block *blk, float *ysave, float *out, void *stream);
int ntm_unet_resblock_tiled_backward(const float *src0, const float *src1, const float *init_w, const float *film,
                                     int64_t film_stride, const float *w_first, const float *w_gated, const float *w_res, int64_t B,
                                     const ntm_unet_block *blk, const float *ysave, const float *gout, float *ws, float *g_src0,
                                     float *g_src1, float *gfilm, float *partials, void *stream);

/*
 * The adjoints of ntm_unet_down_combine and ntm_unet_up_combine (csrc/unet_resample_train.hip).  Additions within ABI version 9.
 * Sizes, layouts and limits are the forwards'; fp32 in and out, one launch each.  No atomics: every sum is a gather in a fixed
 * order, so equal calls give equal bits and a stream's results do not depend on its batch.  An upstream gradient that is NULL is
 * zero (not both), and an output that is NULL is not computed (not all).
 *
 * ntm_unet_down_combine_backward: from g_xo [B][C][Fo] and g_po [B][1][Fo], Fo = ceil(F / S), with w = width:
 *     g_pd[b][j]   = g_po[b][j] + (sum_c wc[c] g_xo[b][c][j]) / sqrt 2
 *     g_x[b][c][f] = (sum_j ker[f + w - j S] g_xo[b][c][j]) / sqrt 2       [B][C][F]; j ascending over the terms in range
 *     g_pyr[b][f]  = sum_j ker[f + w - j S] g_pd[b][j]                      [B][1][F]
 *     partials[b][c] = (sum_j g_xo[b][c][j] pyr_d[b][j]) / sqrt 2           [B][C]; pyr_d is the forward's pyr_out.  Added in fp64
 *                    in a fixed order, rounded once; ntm_unet_wgrad_reduce(partials, B, C, g_wc) gives the combiner's gradient.
 * ntm_unet_up_combine_backward: from g_xo [B][C][S F] (NULL with S == 1) and g_po [B][1][S F]; pyr_T == 0 says that the forward
 *   had no pyramid, else it is the forward's pyr_T >= F:
 *     g_p[b][f]    = sum_{ph, i} ker[ph][i] g_po[b][(f - i + w) S + ph]     (S == 1: g_po[b][f]); / sqrt 2 with a pyramid
 *     g_x[b][c][f] = the same gather of g_xo[b][c] + wc[c] g_p[b][f]        [B][C][F]
 *     g_pyr[b][f]  = g_p[b][f], 0 for F <= f < pyr_T                        [B][1][pyr_T]; only with a pyramid
 *     partials[b][t][c] = sum_{f in tile t} g_p[b][f] x[b][c][f]            [B][P][C], P = ntm_unet_up_combine_backward_partials(F)
 *                    = ceil(F / 256) tiles of 256 frames; fp64 in a fixed order, rounded once;
 *                    ntm_unet_wgrad_reduce(partials, B P, C, g_wc) gives the combiner's gradient.
 *   Refused (NTM_EINVAL, a message starting with the function's name, before anything touches a device): what the forwards refuse
 *   of the sizes (B outside [0, 65535], C outside [1, 32], taps > 64 or not 2 width + S (down) / 2 width + 1 (up), S == 1 with a
 *   filter, C frames >= 2^31), 0 < pyr_T < F, g_pyr with pyr_T == 0, both upstream gradients NULL, every output NULL, a NULL ker
 *   or wc, partials without pyr_d (down) or x (up).  B == 0 returns NTM_OK.
 */
int ntm_unet_down_combine_backward(const float *pyr_d, const float *ker, const float *wc, const float *g_xo, const float *g_po,
                                   int64_t B, int C, int64_t F, int S, int width, int taps, float *g_x, float *g_pyr, float *partials,
                                   void *stream);
int64_t ntm_unet_up_combine_backward_partials(int64_t F);
int ntm_unet_up_combine_backward(const float *x, const float *ker, const float *wc, const float *g_xo, const float *g_po, int64_t B,
                                 int C, int64_t F, int S, int width, int taps, int64_t pyr_T, float *g_x, float *g_pyr,
                                 float *partials, void *stream);

/*
 * The optimiser step over a list of tensors (csrc/multi_tensor.hip): the total gradient norm and clip coefficient of
 * torch.nn.utils.clip_grad_norm_, torch.optim.Adam's single-tensor step, and the EMA dst = dst s + src (1 - s) of the diffusion
 * trainer.  Additions within ABI version 9.  Every list (p, g, m, v, dst, src) is a HOST array of `count` device pointers to
 * contiguous fp32 tensors, n the host array of their element counts; a tensor of zero elements is skipped (its pointers are not
 * read).  A launch serves up to NTM_MULTI_MAX_TENSORS tensors -- their pointers, sizes and chunk map travel by value in the kernel
 * arguments, so nothing is copied to the device and the arrays may be freed on return -- and a longer list is cut into
 * ceil(tensors / NTM_MULTI_MAX_TENSORS) launches here (tensors: those with n > 0).  One 256-thread workgroup per chunk of
 * NTM_MULTI_CHUNK elements of one tensor; 16-byte accesses where all of a tensor's base pointers are 16-byte aligned, the same
 * elements one by one otherwise, with the same bits either way.  Nothing synchronises with the host.
 *
 * ntm_multi_partials(n, count) = sum_k ceil(n[k] / NTM_MULTI_CHUNK): the doubles ntm_multi_sqnorm writes; -1 on what it refuses.
 * ntm_multi_sqnorm: partials[c] = the sum of g^2 over chunk c, chunks numbered through the whole list in list order.  fp64 in a
 *     fixed order: thread i of 256 adds the elements 4 (i + 256 r) ... + 3, r ascending; then a halving tree over the 256 sums.
 *     *n_partials_out (may be NULL) = ntm_multi_partials(n, count).  Calls on several lists may fill one partials array side by
 *     side (offset the pointer); ntm_multi_clip_coef then takes the norm over all of them.
 * ntm_multi_clip_coef: one workgroup adds partials[0 .. n_partials) in index order in fp64 and writes
 *     norm_coef[0] = (float)sqrt(sum),  norm_coef[1] = (float)min(1, max_norm / (sqrt(sum) + 1e-6))
 *     -- clip_grad_norm_ with error_if_nonfinite=False: a non-finite norm goes into the coefficient (a NaN stays a NaN) and from
 *     there into the parameters; no host check.  n_partials == 0: the norm of nothing, 0.
 * ntm_multi_adam: per element, every operation rounded to fp32 on its own (no fused multiply-add, IEEE division and square root),
 *     in torch's order:
 *         g' = g coef                                     coef = norm_coef[1]; g' is written back to g.  norm_coef == NULL: g' = g,
 *                                                         g is not written
 *         m' = m + (1 - beta1) (g' - m)                   for 1 - beta1 < 0.5; else g' - (g' - m) (1 - (1 - beta1)): ATen's lerp
 *         v' = beta2 v + ((1 - beta2) g') g'
 *         p' = p + (-step_size) (m' / (sqrtf(v') / bc2_sqrt + eps))
 *     with step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) formed by the caller in double and rounded to fp32 at
 *     the call, like one_minus_beta1 and one_minus_beta2 -- what torch does with its Python scalars.
 * ntm_multi_ema: dst' = dst s + src one_minus_s: two rounded products, one rounded sum (dst == src is allowed).
 *   No atomics: equal calls give equal bits, and a tensor's results do not depend on the list it is in (the norm aside).
 *   Refused (NTM_EINVAL, a message starting with the function's name, before anything touches a device): count < 0, a NULL list or
 *   n with count > 0, n[k] < 0 or above 2^32, a NULL tensor pointer with n[k] > 0, p, m and v of one tensor not all distinct
 *   (ntm_multi_adam), NULL partials with chunks to write, a NULL norm_coef or n_partials < 0 (ntm_multi_clip_coef).  count == 0
 *   returns NTM_OK.
 */
#define NTM_MULTI_MAX_TENSORS 64
#define NTM_MULTI_CHUNK 2048
int64_t ntm_multi_partials(const int64_t *n, int64_t count);
int ntm_multi_sqnorm(const float *const *g, const int64_t *n, int64_t count, double *partials, int64_t *n_partials_out, void *stream);
int ntm_multi_clip_coef(const double *partials, int64_t n_partials, float max_norm, float *norm_coef, void *stream);
int ntm_multi_adam(float *const *p, float *const *g, float *const *m, float *const *v, const int64_t *n, int64_t count,
                   const float *norm_coef, float step_size, float bc2_sqrt, float one_minus_beta1, float beta2, float one_minus_beta2,
                   float eps, void *stream);
int ntm_multi_ema(float *const *dst, const float *const *src, const int64_t *n, int64_t count, float s, float one_minus_s, void *stream);

/*
 * The batch feeder of the diffusion trainers (csrc/segment_feed.hip): what the reference's datasets_diffusion.py and
 * Trainer.get_batch do per batch -- a random crop of a file, minus the crop's mean, resampled to the network's rate -- on a
 * "bank" that lives on the device: every training file mixed to mono in fp32, concatenated, bank_len floats.  Additions within
 * ABI version 9.  Row b is bank[start[b] .. start[b] + L); start is a HOST array of B first samples (offset of the file in the
 * bank + the crop's index).  A launch serves up to NTM_SEGMENT_MAX_ROWS rows, whose starts travel by value in the kernel
 * arguments: nothing is copied to the device, the array may be freed on return, and a larger B is cut into
 * ceil(B / NTM_SEGMENT_MAX_ROWS) launches here.  Nothing synchronises with the host.
 *
 * ntm_segment_mean: mean[b] = (float)(sum / L), the sum in fp64 in a fixed order (thread i of 1024 adds x[i], x[i + 1024], ...
 *     ascending; then lanes by shuffles and the 16 waves in wave order), rounded once.
 * ntm_segment_crop: out[b][i] = x[i] - mean[b], one rounded fp32 subtraction (equal rates: the noise net).
 * ntm_segment_decimate: torchaudio's polyphase rule for a reduced ratio orig : 1 with the filter ker[taps], taps == 2 width + orig:
 *         out[b][j] = sum_k ker[k] xz[b][j orig + k - width],   j < ceil(L / orig),
 *     xz = x - mean[b] inside [0, L) and exactly 0 outside (the padding is zeros, not -mean).  The crop, the subtraction and the
 *     filter are one pass over the bank: no [B][L] intermediate.  One 256-thread workgroup per output; thread i takes the taps
 *     i, i + 256, ... ascending, the difference and the product rounded to fp32 each, added in fp64; the same fixed tree joins them.
 *   No atomics: equal calls give equal bits, and a row's result does not depend on the rows beside it.
 *   Refused (NTM_EINVAL, a message starting with the function's name, before anything touches a device): a NULL pointer, B < 0,
 *   L < 1, orig < 1, width < 0, taps != 2 width + orig, ceil(L / orig) above 2^31 - 1, and a row outside the bank
 *   (start[b] < 0 or start[b] + L > bank_len).  B == 0 returns NTM_OK.
 */
#define NTM_SEGMENT_MAX_ROWS 64
int ntm_segment_mean(const float *bank, int64_t bank_len, const int64_t *start, int64_t B, int64_t L, float *mean, void *stream);
int ntm_segment_crop(const float *bank, int64_t bank_len, const int64_t *start, const float *mean, int64_t B, int64_t L, float *out,
                     void *stream);
int ntm_segment_decimate(const float *bank, int64_t bank_len, const int64_t *start, const float *mean, int64_t B, int64_t L,
                         const float *ker, int orig, int width, int taps, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NTM_H */
