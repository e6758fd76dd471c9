// The whole EDM sampler of a diffusion generator whose every level fits one workgroup (the WHOLE form of the block, T <= 1024:
// the trajectory nets) in ONE launch: what DiffusionGenerator._sample runs as n_steps x (edm_pre, the network's calls, edm_post).
//
// unet_sampler_kernel   grid (1, B), 1024 threads: the workgroup of stream b walks the steps, and within a step the stage table
//                       (ntm_unet_stage: block | down + combine | combine + up | final combiner), with that step's edm_pre in
//                       front and edm_post behind.  A stream never reads another stream's data, so a workgroup touches only its
//                       own stream's rows of every buffer and no workgroup ever waits for another: no grid sync, no spin, no
//                       atomics -- occupancy cannot hang it.
// One definition per output: the block stage IS unet_block_body<false> (unet_block.h; blockIdx.x == 0, blockIdx.y == stream:
// the geometry of its whole form), the other stages and the EDM arithmetic call unet_steps.h's per-output functions, which the
// step-by-step kernels (unet_kernels.hip) call too.  Only which thread computes an output changes: 1024 threads stride over a
// stream's outputs where 256 threads cover a grid.  Equal operations in equal order: the sample is bit-identical.
// Between stages: a stage reads from global memory what an earlier stage of the SAME workgroup wrote there.  stage_sync() is a
// workgroup-scope release (with every wave's own stores drained), the workgroup barrier, a workgroup-scope acquire: the waves
// of a workgroup share their CU's vector L1, which is write-through, so a vector load behind it sees the stores in front of it.
// The intermediates (z, the network's input and output, every stage's outputs) are therefore read through plain pointers with
// lane-dependent addresses -- vector loads -- and never through const __restrict__ or a non-temporal load, which would let
// the compiler take the scalar cache, which no vector store updates.  The stage table, the per-step scalars and FiLM rows, the
// weights, the filters and the draws are read-only for the whole launch; uniform reads of those may be scalar.
// A resample stage first copies its stream's rows of x (and the pyramid) into LDS, with such vector loads, and computes from there:
// every output reads `taps` frames tap by tap, and one workgroup has no other workgroups to hide that latency behind (measured:
// from global memory the sampler was 6 % slower than the step path, from LDS it ties).  Same values, same order of operations.
// Dynamic LDS is the largest stage's need (sampler_lds_bytes), with unet_block_kernel's opt-in above 64 KB.
// Every loop bound is a field ntm_unet_sample_one_launch (ntm_api.hip) has checked against a cap on the HOST copy of the table
// (stages, steps, channels, taps, frames); the kernel clamps the same bounds again on the device copy it walks, so that a
// device copy that differs from the checked one still ends.
#include "unet_steps.h"

namespace ntm {

struct USampleArgs {
    const ntm_unet_stage *stages;
    const float *scal, *films, *z0, *draws, *x_outpaint, *mask;
    float *zin, *net_in, *F, *z;
    int64_t film_len, mask_stride, B;
    uint64_t eps_steps;
    int n_stages, n_steps, T;
};

static_assert(sizeof(ntm_unet_stage) == 168, "ntm_unet_stage: the documented 168 bytes (diffusion's ctypes mirror)");
static_assert(sizeof(ntm_unet_block) == 64, "ntm_unet_block: 64 bytes");

constexpr int kSThreads = kUWaves * 64;
constexpr int kSMaxT = NTM_UNET_WHOLE_MAX_T, kSMaxUp = 2 * NTM_UNET_WHOLE_MAX_T, kSMaxC = 32, kSMaxTaps = 64;

__device__ __forceinline__ int clampi(int v, int hi) { return v < hi ? v : hi; }

// the stores of this stage become visible to the vector loads of the next one, in this workgroup
__device__ __forceinline__ void stage_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // the wave's own stores and LDS reads, whatever the fence kept
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// A record of the table or a row of scalars, which every lane reads from one address, into scalar registers: behind the
// fences of stage_sync() the compiler loads them per lane, and a block stage has no vector registers to spare for 42 copies.
template <class V>
__device__ __forceinline__ V load_uniform(const V *p)
{
    static_assert(sizeof(V) % 4 == 0, "dwords");
    union { V v; unsigned u[sizeof(V) / 4]; } r;
#pragma unroll
    for (unsigned i = 0; i < sizeof(V) / 4; ++i) r.u[i] = __builtin_amdgcn_readfirstlane(reinterpret_cast<const unsigned *>(p)[i]);
    return r.v;
}

// threadIdx.x as a value the compiler computes where it is used: what a light stage derives from it (addresses, indices) then
// stays inside that stage, and does not sit in vector registers through the block stages, which have none to spare
__device__ __forceinline__ int own_tid()
{
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

struct UStepScalars { float eps_scale, snoise, sigma0, cin, cskip, cout, b2, k; };
static_assert(sizeof(UStepScalars) == NTM_UNET_SAMPLE_SCALARS * sizeof(float), "a row of scal");

__global__ __launch_bounds__(kSThreads) void unet_sampler_kernel(USampleArgs s)
{
    extern __shared__ float lds[];
    const int64_t b = blockIdx.y, row = b * s.T, BT = s.B * s.T;
    const int n_steps = clampi(s.n_steps, NTM_UNET_SAMPLE_MAX_STEPS), n_stages = clampi(s.n_stages, NTM_UNET_SAMPLE_MAX_STAGES);
    const int T = clampi(s.T, kSMaxT);
    int draw = 0;
    for (int step = 0; step < n_steps; ++step) {
        const int tid = own_tid();
        const UStepScalars sc = load_uniform(reinterpret_cast<const UStepScalars *>(s.scal) + step);
        const float *films = s.films + step * s.film_len;
        {   // the stream's own rows: element t of them (pointers moved to the row, so that an address is a scalar base and t)
            EdmPreArgs p{};
            p.z = (step ? s.z : s.z0) + row;
            if ((s.eps_steps >> step) & 1) p.eps = s.draws + draw++ * BT + row;
            if (s.mask) p.mask = s.mask + b * s.mask_stride, p.x_out = s.x_outpaint + row, p.n = s.draws + draw++ * BT + row;
            p.z_out = s.zin + row, p.net_in = s.net_in + row;
            p.eps_scale = sc.eps_scale, p.snoise = sc.snoise, p.sigma0 = sc.sigma0, p.cin = sc.cin;
            p.mask_stride = 0, p.T = s.T, p.N = s.T;
            for (unsigned t = tid; t < (unsigned)T; t += kSThreads) edm_pre_one(p, t);
        }
        stage_sync();
        for (int q = 0; q < n_stages; ++q) {
            const ntm_unet_stage st = load_uniform(s.stages + q);
            const int tid = own_tid();
            if (st.kind == NTM_USTAGE_BLOCK) {
                UBlockArgs a = unet_block_args(st.a ? st.a : s.net_in, st.b, st.w3, films + st.film_off, 0, st.w0, st.w1, st.w2,
                                               st.blk, st.o0);
                a.l0 = 0, a.l1 = a.nl = clampi(a.nl, 8);
                unet_block_body<false>(a, nullptr);
            } else if (st.kind == NTM_USTAGE_DOWN) {
                // the stream's rows of x and the pyramid go through LDS once: every output reads `taps` frames of two rows, and
                // one workgroup has no other workgroups' loads to hide the latency of reading them from memory tap by tap
                const int F = clampi((int)st.F, kSMaxT), S = st.S > 0 ? st.S : 1, C = clampi(st.C, kSMaxC), Fo = (F + S - 1) / S;
                const float *x = st.a + b * C * F, *pyr = (st.b ? st.b : s.net_in) + b * F;
                float *lx = lds, *lp = lds + C * F;
                for (int e = tid; e < C * F; e += kSThreads) lx[e] = x[e];
                for (int e = tid; e < F; e += kSThreads) lp[e] = pyr[e];
                __syncthreads();
                const UDownArgs d{lx, lp, st.w0, st.w1, st.o0 + b * C * Fo, st.o1 + b * Fo, C, F, Fo, S, st.width, clampi(st.taps, kSMaxTaps)};
                for (int e = tid; e < C * Fo; e += kSThreads) udown_one(d, 0, e / Fo, e % Fo);
            } else if (st.kind == NTM_USTAGE_UP || st.kind == NTM_USTAGE_FINAL) {
                const int F = clampi((int)st.F, kSMaxT), S = st.S > 0 ? st.S : 1, C = clampi(st.C, kSMaxC);
                const int Fo = clampi(S * F, kSMaxUp);
                const float *x = st.a + b * C * F;
                float *lx = lds, *pn = lds + C * F;               // x through LDS as above, then the combined pyramid
                for (int e = tid; e < C * F; e += kSThreads) lx[e] = x[e];
                __syncthreads();
                const UUpArgs u{lx, st.b ? st.b + b * st.pyr_T : nullptr, st.w0, st.w1, st.o0 ? st.o0 + b * C * Fo : nullptr,
                                (st.o1 ? st.o1 : s.F) + b * Fo, C, F, S, st.width, clampi(st.taps, kSMaxTaps), (int)st.pyr_T, Fo};
                if (u.x_out)
                    for (int e = tid; e < C * Fo; e += kSThreads) {
                        const int c = e / Fo, n = e % Fo, j = n / S;
                        uup_x_one(u, 0, c, n, j, n - j * S);
                    }
                // the pyramid: the level's combined frames once, frame g at pn[g + width], then the filter
                const int cnt = F + (u.taps > 0 ? u.taps - 1 : 0);
                for (int t = tid; t < cnt; t += kSThreads) pn[t] = uup_combined(u, 0, t - u.width);
                __syncthreads();
                for (int n = tid; n < Fo; n += kSThreads) {
                    const int j = n / S;
                    uup_pyr_one(u, 0, n, n - j * S, pn + j);
                }
            }
            stage_sync();
        }
        for (unsigned t = own_tid(); t < (unsigned)T; t += kSThreads)
            edm_post_one(s.zin + row, s.F + row, sc.cskip, sc.cout, sc.b2, sc.k, t, s.z + row);
        stage_sync();
    }
}

// bytes of dynamic LDS: the largest stage's
static size_t sampler_lds_bytes(const ntm_unet_stage *stages, int n_stages)
{
    size_t lds = 0;
    for (int q = 0; q < n_stages; ++q) {
        const ntm_unet_stage &st = stages[q];
        size_t need = 0;
        if (st.kind == NTM_USTAGE_BLOCK)
            need = unet_block_lds_bytes(unet_block_args(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, st.blk, nullptr));
        else if (st.kind == NTM_USTAGE_DOWN)
            need = (size_t)(st.C + 1) * st.F * sizeof(float);                   // the rows of x and the pyramid
        else
            need = (size_t)(st.C * st.F + st.F + (st.taps > 0 ? st.taps - 1 : 0)) * sizeof(float);     // x, the combined pyramid
        lds = need > lds ? need : lds;
    }
    return lds;
}

hipError_t launch_unet_sampler(const ntm_unet_stage *stages, const ntm_unet_stage *stages_dev, int n_stages, const float *scal,
                               const float *films, int64_t film_len, int n_steps, uint64_t eps_steps, const float *z0,
                               const float *draws, const float *x_outpaint, const float *mask, int64_t mask_stride, int64_t B,
                               int64_t T, float *ws, float *z, hipStream_t stream)
{
    USampleArgs s{};
    s.stages = stages_dev, s.scal = scal, s.films = films, s.z0 = z0, s.draws = draws, s.x_outpaint = x_outpaint, s.mask = mask;
    s.zin = ws, s.net_in = ws + B * T, s.F = ws + 2 * B * T, s.z = z;
    s.film_len = film_len, s.mask_stride = mask_stride, s.B = B, s.eps_steps = eps_steps;
    s.n_stages = n_stages, s.n_steps = n_steps, s.T = (int)T;
    const size_t lds = sampler_lds_bytes(stages, n_stages);
    if (lds > 64 * 1024)      // above the default limit of a launch, as for unet_block_kernel: the CU has 160 KB
        if (hipError_t e = hipFuncSetAttribute((const void *)unet_sampler_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
            return e;
    hipLaunchKernelGGL(unet_sampler_kernel, dim3(1, (unsigned)B), dim3(kSThreads), lds, stream, s);
    return hipGetLastError();
}

}  // namespace ntm
