// The batch feeder of the diffusion trainers (ntm_segment_* in include/ntm.h): what the reference's datasets_diffusion.py and
// Trainer.get_batch do per batch -- a random crop of a file, minus the crop's mean, resampled to the network's rate -- on a
// "bank" that lives on the device: every training file mixed to mono in fp32, concatenated.  A row is start[b] .. start[b] + L
// of the bank.  The starts of a launch travel BY VALUE in the kernel arguments (SegStarts, 512 bytes): no staging copy, nothing
// whose lifetime has to outlast the launch, no host synchronisation.  A launch serves up to NTM_SEGMENT_MAX_ROWS rows.
//
//   segment_mean_kernel      one 1024-thread workgroup per row: thread i adds x[i], x[i + 1024], ... ascending in fp64, then a
//                            fixed tree (lanes by shuffles, the 16 waves in wave order); mean = (float)(sum / L), one rounding;
//   segment_crop_kernel      out = x - mean, one rounded subtraction per element (the noise net: both rates equal);
//   segment_decimate_kernel  torchaudio's polyphase rule for a reduced ratio orig : 1 (diffusion.apply_resample_kernel, new == 1):
//                                out[b][j] = sum_k ker[k] xz[b][j orig + k - width],  xz = x - mean in [0, L), exactly 0 outside
//                            one 256-thread workgroup per (row, output).  The crop, the mean subtraction and the filter are one
//                            pass over the bank.  Thread i takes the taps i, i + 256, ... ascending: the difference and the
//                            product rounded to fp32 each, added in fp64; then the same fixed tree.  Taps whose sample lies in
//                            the padding are skipped (their term is an exact zero).
// No atomics, nothing crosses a workgroup: equal calls give equal bits, and a row's result does not depend on the rows beside it.
#include "ntm_common.h"

#pragma clang fp contract(off)

namespace ntm {

constexpr int kMeanThreads = 1024;
constexpr int kCropThreads = 256;
constexpr int kCropPerThread = 4;
constexpr int kDecThreads = 256;

// the workgroup's sum of `v`, valid in thread 0: lanes by shuffles (64 -> 1), then the waves in wave order
template <int THREADS>
__device__ __forceinline__ double block_sum_f64(double v, double *red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (tid == 0) {
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) s += red[w];
    }
    return s;
}

__global__ __launch_bounds__(kMeanThreads) void segment_mean_kernel(const float *bank, SegStarts st, int64_t L, float *mean)
{
    __shared__ double red[kMeanThreads / 64];
    const float *x = bank + st.s[blockIdx.x];
    double acc = 0.0;
#pragma unroll 8
    for (int64_t i = threadIdx.x; i < L; i += kMeanThreads) acc += (double)x[i];
    const double s = block_sum_f64<kMeanThreads>(acc, red);
    if (threadIdx.x == 0) mean[blockIdx.x] = (float)(s / (double)L);
}

__global__ __launch_bounds__(kCropThreads) void segment_crop_kernel(const float *bank, SegStarts st, const float *mean, int64_t L,
                                                                    float *out)
{
    const int b = blockIdx.y;
    const float *x = bank + st.s[b];
    float *o = out + (int64_t)b * L;
    const float m = mean[b];
    const int64_t i0 = (int64_t)blockIdx.x * (kCropThreads * kCropPerThread) + threadIdx.x;
#pragma unroll
    for (int r = 0; r < kCropPerThread; ++r) {
        const int64_t i = i0 + r * kCropThreads;
        if (i < L) o[i] = x[i] - m;
    }
}

__global__ __launch_bounds__(kDecThreads) void segment_decimate_kernel(const float *bank, SegStarts st, const float *mean, int64_t L,
                                                                       const float *ker, int orig, int width, int taps,
                                                                       int64_t n_out, float *out)
{
    __shared__ double red[kDecThreads / 64];
    const int b = blockIdx.y;
    const int64_t j = blockIdx.x;
    const float m = mean[b];
    // tap k reads sample j orig + k - width of the row: in [0, L) for k in [k_lo, k_hi)
    const int64_t first = j * orig - width;
    const int64_t lo = first < 0 ? -first : 0, hi = L - first < taps ? L - first : taps;
    const int k_lo = (int)lo, k_hi = (int)hi;              // 0 <= k_lo, k_hi <= taps; first < L, so k_hi >= 1
    const float *x = bank + st.s[b] + first;               // only x[k_lo .. k_hi) is read: inside the row
    double acc = 0.0;
#pragma unroll 4
    for (int k = (k_lo / kDecThreads) * kDecThreads + (int)threadIdx.x; k < k_hi; k += kDecThreads) {
        if (k >= k_lo) {
            const float xz = x[k] - m;
            const float p = ker[k] * xz;
            acc += (double)p;
        }
    }
    const double s = block_sum_f64<kDecThreads>(acc, red);
    if (threadIdx.x == 0) out[(int64_t)b * n_out + j] = (float)s;
}

hipError_t launch_segment_mean(const float *bank, const SegStarts &st, int rows, int64_t L, float *mean, hipStream_t stream)
{
    hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)rows), dim3(kMeanThreads), 0, stream, bank, st, L, mean);
    return hipGetLastError();
}

hipError_t launch_segment_crop(const float *bank, const SegStarts &st, const float *mean, int rows, int64_t L, float *out,
                               hipStream_t stream)
{
    const int64_t per = kCropThreads * kCropPerThread;
    hipLaunchKernelGGL(segment_crop_kernel, dim3((unsigned)((L + per - 1) / per), (unsigned)rows), dim3(kCropThreads), 0, stream, bank,
                       st, mean, L, out);
    return hipGetLastError();
}

hipError_t launch_segment_decimate(const float *bank, const SegStarts &st, const float *mean, int rows, int64_t L, const float *ker,
                                   int orig, int width, int taps, int64_t n_out, float *out, hipStream_t stream)
{
    hipLaunchKernelGGL(segment_decimate_kernel, dim3((unsigned)n_out, (unsigned)rows), dim3(kDecThreads), 0, stream, bank, st, mean, L,
                       ker, orig, width, taps, n_out, out);
    return hipGetLastError();
}

}  // namespace ntm
