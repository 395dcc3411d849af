// Gradient-noise diagnostics (simple noise scale, McCandlish et al. 2018) on gfx950 - the device half of
// estimate_noise_scale (rl/sns.py:149-178) and of the norms it takes (rl/utils.py:146-161).
//
// The reference runs b_big / b_small backward passes of b_small rows; after each it takes the gradient's 2-norm
// (`optimizer_grad_norm`: one `.norm(2).item()` per parameter tensor, i.e. a device->host sync each) and adds the
// gradient into a running sum (`acc += p`, one launch per parameter tensor).  Here every backward pass overwrites ONE
// flat gradient buffer, so the per-pass work is two streaming operations over one contiguous array:
//
//  * ppo_grad_noise_pass_f32    one launch per pass: acc = grad (pass 0) or acc += grad (float32, element-wise: the
//                               rounding of ppo_accumulate_f32 and of the reference's `acc += p`), and from the same read
//                               the pass's sum of grad^2 in float64, left as per-workgroup partials in workspace[pass].
//                               A float32 square is exact in float64: summation is the only rounding.
//  * ppo_grad_noise_finish_f64  two launches: the partials of sum acc^2 into workspace[passes], then every row summed:
//                               out[0..passes) = each pass's sum g^2, out[passes] = sum acc^2.  The host reads `out`
//                               in one copy; nothing is read back during an estimate.
//
// Every sum has a fixed order: the workgroup count is a function of n alone, a thread's elements follow a fixed
// grid-stride map, then a 64-lane shuffle tree, the workgroup's 4 waves in order, and the partials in a fixed strided
// order + shuffle tree.  No atomics: two runs on the same input give the same bits.
//
// The kernels are bandwidth / launch-latency bound (1 - 2 M floats): 16-byte accesses over the part of the buffers
// where `acc` is 16-byte aligned, at most 3 + 3 scalar elements around it.  `grad` may sit at any other 4-byte offset:
// it is read with 4-byte-aligned 16-byte loads (global_load_dwordx4 needs dword alignment only).  Loads are never
// predicated: an unrolled slot past the end reads a clamped address and its value is dropped.
#include "common.h"

namespace ppo {
namespace {

constexpr int kGnBlocks = 256;   // most workgroups of a launch = partials per workspace row
constexpr int kGnThreads = 256;
constexpr int kGnUnroll = 4;     // 16-byte loads in flight per thread and operand

typedef float gn_f32x4 __attribute__((ext_vector_type(4)));
typedef gn_f32x4 gn_f32x4_a4 __attribute__((aligned(4)));  // a 16-byte access that is only known to be dword aligned

__device__ __forceinline__ double gn_sumsq(gn_f32x4 v, double s)
{
    s += (double)v.x * (double)v.x;
    s += (double)v.y * (double)v.y;
    s += (double)v.z * (double)v.z;
    s += (double)v.w * (double)v.w;
    return s;
}

// the workgroup's sum in a fixed order -> partials[blockIdx.x]
__device__ __forceinline__ void gn_block_reduce(double s, double *__restrict__ partials)
{
    __shared__ double wave_sum[kGnThreads / kWave];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_sum[threadIdx.x / kWave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = wave_sum[0];
#pragma unroll
        for (int w = 1; w < kGnThreads / kWave; ++w) t += wave_sum[w];
        partials[blockIdx.x] = t;
    }
}

// Elements [0, head) and [head + 4 * n4, n) are the scalar head and tail (at most 3 each), done by 8 threads of
// workgroup 0; [head, head + 4 * n4) are n4 vectors whose `acc` address is 16-byte aligned.
// FIRST: acc = grad (acc is not read).  ACCUMULATE false: sum of squares of `grad` alone, nothing is written.
template <bool FIRST, bool ACCUMULATE>
__global__ __launch_bounds__(kGnThreads) void grad_noise_pass_kernel(const float *__restrict__ grad, float *__restrict__ acc,
                                                                     int64_t n, int head, int64_t n4,
                                                                     double *__restrict__ partials)
{
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kGnThreads;
    const gn_f32x4_a4 *g4 = reinterpret_cast<const gn_f32x4_a4 *>(grad + head);
    gn_f32x4 *a4 = reinterpret_cast<gn_f32x4 *>(acc + head);
    for (int64_t i0 = (int64_t)blockIdx.x * kGnThreads + threadIdx.x; i0 < n4; i0 += stride * kGnUnroll) {
        gn_f32x4 g[kGnUnroll], a[kGnUnroll];
#pragma unroll
        for (int u = 0; u < kGnUnroll; ++u) {
            const int64_t i = i0 + stride * u;
            const int64_t ic = i < n4 ? i : i0;  // clamped address, unconditional load
            g[u] = g4[ic];
            if (ACCUMULATE && !FIRST) a[u] = a4[ic];
        }
#pragma unroll
        for (int u = 0; u < kGnUnroll; ++u) {
            const int64_t i = i0 + stride * u;
            if (i < n4) {
                if (ACCUMULATE) a4[i] = FIRST ? g[u] : a[u] + g[u];
                s = gn_sumsq(g[u], s);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const int t = threadIdx.x;
        const int64_t e = t < 4 ? t : (int64_t)head + 4 * n4 + (t - 4);
        const bool mine = t < 4 ? t < head : e < n;
        const int64_t ec = mine ? e : 0;  // n >= 1: element 0 exists
        const float g = grad[ec];
        const float a = (ACCUMULATE && !FIRST) ? acc[ec] : 0.0f;
        if (mine) {
            if (ACCUMULATE) acc[e] = FIRST ? g : a + g;
            s += (double)g * (double)g;
        }
    }
    gn_block_reduce(s, partials);
}

// one wave per output: out[r] = sum of the n_partials partials of workspace row r
__global__ __launch_bounds__(kWave) void grad_noise_final_kernel(const double *__restrict__ workspace, int n_partials,
                                                                 double *__restrict__ out)
{
    const double *row = workspace + (int64_t)blockIdx.x * kGnBlocks;
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += kWave) s += row[i];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

struct GnShape {
    int head;
    int64_t n4;
    int blocks;
};

// a function of n and of acc's address modulo 16 alone
GnShape gn_shape(const float *acc, int64_t n)
{
    GnShape s;
    const int mis = (int)((reinterpret_cast<uintptr_t>(acc) >> 2) & 3);
    s.head = (4 - mis) & 3;
    if (s.head > n) s.head = (int)n;
    s.n4 = (n - s.head) / 4;
    const int64_t per_block = (int64_t)kGnThreads * kGnUnroll;
    int64_t b = (s.n4 + per_block - 1) / per_block;
    s.blocks = b < 1 ? 1 : (b > kGnBlocks ? kGnBlocks : (int)b);
    return s;
}

}  // namespace
}  // namespace ppo

extern "C" size_t ppo_grad_noise_workspace_bytes(int max_passes)
{
    if (max_passes < 1) return 0;
    return ((size_t)max_passes + 1) * ppo::kGnBlocks * sizeof(double);
}

extern "C" int ppo_grad_noise_pass_f32(const float *grad, float *acc, int64_t n, int pass, int max_passes, void *workspace,
                                       void *stream)
{
    using namespace ppo;
    if (n < 1) return fail(PPO_E_INVALID, "ppo_grad_noise_pass_f32: n < 1");
    if (max_passes < 1 || pass < 0 || pass >= max_passes)
        return fail(PPO_E_INVALID, "ppo_grad_noise_pass_f32: pass %d outside [0, %d)", pass, max_passes);
    if (!grad || !acc || !workspace) return fail(PPO_E_INVALID, "ppo_grad_noise_pass_f32: null pointer");
    if (!aligned(grad, 4) || !aligned(acc, 4) || !aligned(workspace, 8))
        return fail(PPO_E_ALIGN, "ppo_grad_noise_pass_f32: grad / acc need 4-byte, workspace 8-byte alignment");
    const GnShape s = gn_shape(acc, n);
    double *partials = static_cast<double *>(workspace) + (int64_t)pass * kGnBlocks;
    if (pass == 0)
        hipLaunchKernelGGL((grad_noise_pass_kernel<true, true>), dim3(s.blocks), dim3(kGnThreads), 0, as_stream(stream), grad,
                           acc, n, s.head, s.n4, partials);
    else
        hipLaunchKernelGGL((grad_noise_pass_kernel<false, true>), dim3(s.blocks), dim3(kGnThreads), 0, as_stream(stream), grad,
                           acc, n, s.head, s.n4, partials);
    return check_launch("grad_noise_pass_kernel");
}

extern "C" int ppo_grad_noise_finish_f64(const float *acc, int64_t n, int passes, int max_passes, void *workspace, double *out,
                                         void *stream)
{
    using namespace ppo;
    if (n < 1) return fail(PPO_E_INVALID, "ppo_grad_noise_finish_f64: n < 1");
    if (max_passes < 1 || passes < 1 || passes > max_passes)
        return fail(PPO_E_INVALID, "ppo_grad_noise_finish_f64: passes %d outside [1, %d]", passes, max_passes);
    if (!acc || !workspace || !out) return fail(PPO_E_INVALID, "ppo_grad_noise_finish_f64: null pointer");
    if (!aligned(acc, 4) || !aligned(workspace, 8) || !aligned(out, 8))
        return fail(PPO_E_ALIGN, "ppo_grad_noise_finish_f64: acc needs 4-byte, workspace / out 8-byte alignment");
    const GnShape s = gn_shape(acc, n);  // the shape the passes ran with: every row holds s.blocks partials
    double *ws = static_cast<double *>(workspace);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL((grad_noise_pass_kernel<false, false>), dim3(s.blocks), dim3(kGnThreads), 0, st, acc,
                       const_cast<float *>(acc), n, s.head, s.n4, ws + (int64_t)passes * kGnBlocks);
    int rc = check_launch("grad_noise_pass_kernel (sum acc^2)");
    if (rc) return rc;
    hipLaunchKernelGGL(grad_noise_final_kernel, dim3(passes + 1), dim3(kWave), 0, st, ws, s.blocks, out);
    return check_launch("grad_noise_final_kernel");
}
