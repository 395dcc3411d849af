// nn.BatchNorm2d for the IMPALA residual blocks (reference: rl/impala.py:63-76, bn0 / bn1 of CnnBasicBlock), NCHW
// float32, eps / momentum / affine / running statistics as torch's defaults.  Three operations, all HBM-bound:
//
//   batch form     (model.train(), the rollout's forwards)   2 launches: per-(channel, slice) partial sums, then apply
//   running form   (model.eval(), everything else)           1 launch
//   backward of the running form                             2 launches: dx + partial sums, then the (c)-sized finish
//
// Every sum over n*h*w runs in float64 in an order fixed by the shape alone: a lane adds its own elements in index
// order, a wave is reduced by a shuffle tree, the waves of a workgroup are added in wave order, and the workgroups of a
// channel ("slices" of whole planes, at most PPO_BATCHNORM_MAX_SLICES) meet in the workspace and are added by a second
// launch - a shuffle tree over slice index in the prologue of the apply kernel, a serial loop in the backward finish.
// There are no float atomics and no hand-off between the workgroups of one launch, so nothing depends on scheduling and
// two runs give the same bits.
//
// Walking a channel: a wave takes whole (image, channel) planes.  Planes start at element (n*C + c)*h*w, which is a
// multiple of four only by luck (21x21 and 11x11 planes are odd), so each plane is read as a scalar head up to the next
// 16-byte boundary, a float4 body and a scalar tail; every tensor of a call shares the element offset, so one split
// serves them all.  When a base pointer is not 16-byte aligned the whole plane is the scalar head.
#include "common.h"

namespace ppo {
namespace {

constexpr int kBnThreads = 256;
constexpr int kBnWaves = kBnThreads / kWave;

struct BnSlicing {
    int slices;            // workgroups per channel
    int planes_per_slice;  // images each of them walks
};

// A function of the shape alone: the summation order, and with it every bit of the result, follows from it.
inline BnSlicing bn_slicing(int n, int c)
{
    int s = (n + kBnWaves - 1) / kBnWaves;  // one plane per wave where the batch is large enough
    if (s > PPO_BATCHNORM_MAX_SLICES) s = PPO_BATCHNORM_MAX_SLICES;
    const int cap = 4096 / c;  // no more workgroups than keep the chip busy
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    BnSlicing r;
    r.planes_per_slice = (n + s - 1) / s;
    r.slices = (n + r.planes_per_slice - 1) / r.planes_per_slice;  // no empty slice
    return r;
}

// Calls f4(e) for the 16-byte aligned groups of four and f1(e) for the remaining elements (e = element offset from the
// tensors' bases) of this wave's planes of channel `ch` among images [n0, n1).
template <class F4, class F1>
__device__ __forceinline__ void bn_walk(int n0, int n1, int ch, int C, int hw, bool vec, F4 f4, F1 f1)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    for (int img = n0 + wave; img < n1; img += kBnWaves) {
        const int64_t e0 = ((int64_t)img * C + ch) * hw;
        int head = vec ? (int)((-e0) & 3) : hw;
        if (head > hw) head = hw;
        const int nvec = (hw - head) >> 2;
        const int edge = hw - 4 * nvec;  // head + tail
        for (int i = lane; i < nvec; i += kWave) f4(e0 + head + 4 * i);
        for (int i = lane; i < edge; i += kWave) f1(e0 + (i < head ? i : i + 4 * nvec));
    }
}

// (a, b) summed over the workgroup in a fixed order; the totals are valid in thread 0.
__device__ __forceinline__ void bn_block_sum(double &a, double &b)
{
    __shared__ double part[kBnWaves][2];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        a += __shfl_down(a, off, kWave);
        b += __shfl_down(b, off, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        part[threadIdx.x / kWave][0] = a;
        part[threadIdx.x / kWave][1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = part[0][0];
        b = part[0][1];
#pragma unroll
        for (int k = 1; k < kBnWaves; ++k) {
            a += part[k][0];
            b += part[k][1];
        }
    }
}

// The slices of one channel added by a butterfly over slice index: a + b == b + a bit for bit, so every lane of every
// wave ends with the same total and no barrier is needed.
__device__ __forceinline__ void bn_combine(const double *__restrict__ ws, int ch, int slices, double &a, double &b)
{
    const int lane = threadIdx.x & (kWave - 1);
    static_assert(PPO_BATCHNORM_MAX_SLICES <= kWave, "one lane per slice");
    const double *row = ws + ((int64_t)ch * slices) * 2;
    a = lane < slices ? row[2 * lane] : 0.0;
    b = lane < slices ? row[2 * lane + 1] : 0.0;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, kWave);
        b += __shfl_xor(b, off, kWave);
    }
}

// grid (slices, c): ws[c][slice] = (sum x, sum x^2)
__global__ __launch_bounds__(kBnThreads) void bn_moments_kernel(const float *__restrict__ x, double *__restrict__ ws, int n,
                                                                int C, int hw, int planes_per_slice, int vec)
{
    const int ch = blockIdx.y;
    const int n0 = blockIdx.x * planes_per_slice;
    const int n1 = min(n, n0 + planes_per_slice);
    double s = 0.0, q = 0.0;
    auto add = [&](float v) {
        const double d = (double)v;
        s += d;
        q += d * d;
    };
    bn_walk(
        n0, n1, ch, C, hw, vec != 0,
        [&](int64_t e) {
            const float4 v = *reinterpret_cast<const float4 *>(x + e);
            add(v.x);
            add(v.y);
            add(v.z);
            add(v.w);
        },
        [&](int64_t e) { add(x[e]); });
    bn_block_sum(s, q);
    if (threadIdx.x == 0) {
        double *dst = ws + ((int64_t)ch * gridDim.x + blockIdx.x) * 2;
        dst[0] = s;
        dst[1] = q;
    }
}

// z = s*x + t over this workgroup's planes
__device__ __forceinline__ void bn_apply(const float *__restrict__ x, float *__restrict__ z, float s, float t, int n0, int n1,
                                         int ch, int C, int hw, bool vec)
{
    bn_walk(
        n0, n1, ch, C, hw, vec,
        [&](int64_t e) {
            const float4 v = *reinterpret_cast<const float4 *>(x + e);
            *reinterpret_cast<float4 *>(z + e) =
                make_float4(fmaf(s, v.x, t), fmaf(s, v.y, t), fmaf(s, v.z, t), fmaf(s, v.w, t));
        },
        [&](int64_t e) { z[e] = fmaf(s, x[e], t); });
}

// grid (slices, c), the slicing of bn_moments_kernel.  Slice 0 of a channel owns its running statistics.
__global__ __launch_bounds__(kBnThreads) void bn_batch_apply_kernel(
    const float *__restrict__ x, const double *__restrict__ ws, const float *__restrict__ gamma,
    const float *__restrict__ beta, float *__restrict__ running_mean, float *__restrict__ running_var,
    long long *__restrict__ num_batches_tracked, float *__restrict__ z, float *__restrict__ batch_mean,
    float *__restrict__ batch_var, int n, int C, int hw, int planes_per_slice, int vec, double eps, double momentum)
{
    const int ch = blockIdx.y;
    double sum, sq;
    bn_combine(ws, ch, gridDim.x, sum, sq);
    const double m = (double)n * (double)hw;
    const double mean = sum / m;
    double var = sq / m - mean * mean;  // biased, as the normalisation uses it
    if (var < 0.0) var = 0.0;
    const double sd = (double)gamma[ch] / sqrt(var + eps);
    const float s = (float)sd;
    const float t = (float)((double)beta[ch] - mean * sd);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (running_mean) running_mean[ch] = (float)((1.0 - momentum) * (double)running_mean[ch] + momentum * mean);
        if (running_var)  // the unbiased estimate goes into the running variance
            running_var[ch] = (float)((1.0 - momentum) * (double)running_var[ch] + momentum * (var * (m / (m - 1.0))));
        if (batch_mean) batch_mean[ch] = (float)mean;
        if (batch_var) batch_var[ch] = (float)var;
        if (num_batches_tracked && ch == 0) *num_batches_tracked += 1;
    }
    const int n0 = blockIdx.x * planes_per_slice;
    bn_apply(x, z, s, t, n0, min(n, n0 + planes_per_slice), ch, C, hw, vec != 0);
}

__global__ __launch_bounds__(kBnThreads) void bn_running_apply_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float *__restrict__ running_mean, const float *__restrict__ running_var, float *__restrict__ z, int n, int C, int hw,
    int planes_per_slice, int vec, double eps)
{
    const int ch = blockIdx.y;
    const double sd = (double)gamma[ch] / sqrt((double)running_var[ch] + eps);
    const float s = (float)sd;
    const float t = (float)((double)beta[ch] - (double)running_mean[ch] * sd);
    const int n0 = blockIdx.x * planes_per_slice;
    bn_apply(x, z, s, t, n0, min(n, n0 + planes_per_slice), ch, C, hw, vec != 0);
}

// grid (slices, c): dx = s*dz (+ residual); ws[c][slice] = (sum dz, sum dz*(x - running_mean))
__global__ __launch_bounds__(kBnThreads) void bn_running_backward_kernel(
    const float *__restrict__ dz, const float *__restrict__ x, const float *__restrict__ residual,
    const float *__restrict__ gamma, const float *__restrict__ running_mean, const float *__restrict__ running_var,
    float *__restrict__ dx, double *__restrict__ ws, int n, int C, int hw, int planes_per_slice, int vec, double eps)
{
    const int ch = blockIdx.y;
    const float s = (float)((double)gamma[ch] / sqrt((double)running_var[ch] + eps));
    const double mu = (double)running_mean[ch];
    const int n0 = blockIdx.x * planes_per_slice;
    const int n1 = min(n, n0 + planes_per_slice);
    double sb = 0.0, sg = 0.0;
    auto add = [&](float g, float v) {
        const double d = (double)g;
        sb += d;
        sg += d * ((double)v - mu);
    };
    if (residual) {
        bn_walk(
            n0, n1, ch, C, hw, vec != 0,
            [&](int64_t e) {
                const float4 g = *reinterpret_cast<const float4 *>(dz + e);
                const float4 v = *reinterpret_cast<const float4 *>(x + e);
                const float4 r = *reinterpret_cast<const float4 *>(residual + e);
                *reinterpret_cast<float4 *>(dx + e) =
                    make_float4(fmaf(s, g.x, r.x), fmaf(s, g.y, r.y), fmaf(s, g.z, r.z), fmaf(s, g.w, r.w));
                add(g.x, v.x);
                add(g.y, v.y);
                add(g.z, v.z);
                add(g.w, v.w);
            },
            [&](int64_t e) {
                const float g = dz[e];
                dx[e] = fmaf(s, g, residual[e]);
                add(g, x[e]);
            });
    } else {
        bn_walk(
            n0, n1, ch, C, hw, vec != 0,
            [&](int64_t e) {
                const float4 g = *reinterpret_cast<const float4 *>(dz + e);
                const float4 v = *reinterpret_cast<const float4 *>(x + e);
                *reinterpret_cast<float4 *>(dx + e) = make_float4(s * g.x, s * g.y, s * g.z, s * g.w);
                add(g.x, v.x);
                add(g.y, v.y);
                add(g.z, v.z);
                add(g.w, v.w);
            },
            [&](int64_t e) {
                const float g = dz[e];
                dx[e] = s * g;
                add(g, x[e]);
            });
    }
    bn_block_sum(sb, sg);
    if (threadIdx.x == 0) {
        double *dst = ws + ((int64_t)ch * gridDim.x + blockIdx.x) * 2;
        dst[0] = sb;
        dst[1] = sg;
    }
}

// one thread per channel: the slices in index order
__global__ __launch_bounds__(kWave) void bn_backward_finish_kernel(const double *__restrict__ ws,
                                                                   const float *__restrict__ running_var,
                                                                   float *__restrict__ dgamma, float *__restrict__ dbeta, int C,
                                                                   int slices, double eps, int accumulate)
{
    const int ch = blockIdx.x * kWave + threadIdx.x;
    if (ch >= C) return;
    const double *row = ws + ((int64_t)ch * slices) * 2;
    double sb = 0.0, sg = 0.0;
    for (int k = 0; k < slices; ++k) {
        sb += row[2 * k];
        sg += row[2 * k + 1];
    }
    sg /= sqrt((double)running_var[ch] + eps);
    if (accumulate) {
        sg += (double)dgamma[ch];
        sb += (double)dbeta[ch];
    }
    dgamma[ch] = (float)sg;
    dbeta[ch] = (float)sb;
}

int bn_check(const char *who, int n, int c, int h, int w, double eps)
{
    if (n < 0 || c <= 0 || h <= 0 || w <= 0) return fail(PPO_E_INVALID, "%s: bad shape", who);
    if (c > 65535) return fail(PPO_E_INVALID, "%s: more than 65535 channels", who);
    if ((int64_t)h * w > (1 << 30)) return fail(PPO_E_INVALID, "%s: plane too large", who);
    if (!(eps >= 0.0)) return fail(PPO_E_INVALID, "%s: bad eps", who);
    return PPO_OK;
}

}  // namespace
}  // namespace ppo

extern "C" size_t ppo_batchnorm_workspace_bytes(int c)
{
    return c > 0 ? (size_t)c * PPO_BATCHNORM_MAX_SLICES * 2 * sizeof(double) : 0;
}

extern "C" int ppo_batchnorm_batch_forward_f32(const float *x, const float *gamma, const float *beta, float *running_mean,
                                               float *running_var, int64_t *num_batches_tracked, float *z, float *batch_mean,
                                               float *batch_var, void *workspace, size_t workspace_bytes, int n, int c, int h,
                                               int w, double eps, double momentum, void *stream)
{
    using namespace ppo;
    const char *who = "ppo_batchnorm_batch_forward_f32";
    if (int rc = bn_check(who, n, c, h, w, eps)) return rc;
    if ((int64_t)n * h * w < 2) return fail(PPO_E_INVALID, "%s: bad shape (batch statistics need n*h*w >= 2)", who);
    if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(PPO_E_INVALID, "%s: bad momentum", who);
    if (!x || !gamma || !beta || !z || !workspace) return fail(PPO_E_INVALID, "%s: null pointer", who);
    if (!aligned(workspace, 8)) return fail(PPO_E_ALIGN, "%s: workspace not 8-byte aligned", who);
    if (workspace_bytes < ppo_batchnorm_workspace_bytes(c)) return fail(PPO_E_INVALID, "%s: workspace too small", who);
    const BnSlicing sl = bn_slicing(n, c);
    const int vec = aligned(x, 16) && aligned(z, 16);
    double *ws = static_cast<double *>(workspace);
    const dim3 grid(sl.slices, c);
    hipLaunchKernelGGL(bn_moments_kernel, grid, dim3(kBnThreads), 0, as_stream(stream), x, ws, n, c, h * w,
                       sl.planes_per_slice, vec);
    if (int rc = check_launch("bn_moments_kernel")) return rc;
    hipLaunchKernelGGL(bn_batch_apply_kernel, grid, dim3(kBnThreads), 0, as_stream(stream), x, (const double *)ws, gamma, beta,
                       running_mean, running_var, reinterpret_cast<long long *>(num_batches_tracked), z, batch_mean, batch_var,
                       n, c, h * w, sl.planes_per_slice, vec, eps, momentum);
    return check_launch("bn_batch_apply_kernel");
}

extern "C" int ppo_batchnorm_running_forward_f32(const float *x, const float *gamma, const float *beta,
                                                 const float *running_mean, const float *running_var, float *z, int n, int c,
                                                 int h, int w, double eps, void *stream)
{
    using namespace ppo;
    const char *who = "ppo_batchnorm_running_forward_f32";
    if (int rc = bn_check(who, n, c, h, w, eps)) return rc;
    if (n == 0) return PPO_OK;
    if (!x || !gamma || !beta || !running_mean || !running_var || !z) return fail(PPO_E_INVALID, "%s: null pointer", who);
    const BnSlicing sl = bn_slicing(n, c);
    const int vec = aligned(x, 16) && aligned(z, 16);
    hipLaunchKernelGGL(bn_running_apply_kernel, dim3(sl.slices, c), dim3(kBnThreads), 0, as_stream(stream), x, gamma, beta,
                       running_mean, running_var, z, n, c, h * w, sl.planes_per_slice, vec, eps);
    return check_launch("bn_running_apply_kernel");
}

extern "C" int ppo_batchnorm_running_backward_f32(const float *dz, const float *x, const float *residual, const float *gamma,
                                                  const float *running_mean, const float *running_var, float *dx, float *dgamma,
                                                  float *dbeta, void *workspace, size_t workspace_bytes, int n, int c, int h,
                                                  int w, double eps, int accumulate, void *stream)
{
    using namespace ppo;
    const char *who = "ppo_batchnorm_running_backward_f32";
    if (int rc = bn_check(who, n, c, h, w, eps)) return rc;
    if (n == 0) return PPO_OK;
    if (!dz || !x || !gamma || !running_mean || !running_var || !dx || !dgamma || !dbeta || !workspace)
        return fail(PPO_E_INVALID, "%s: null pointer", who);
    if (!aligned(workspace, 8)) return fail(PPO_E_ALIGN, "%s: workspace not 8-byte aligned", who);
    if (workspace_bytes < ppo_batchnorm_workspace_bytes(c)) return fail(PPO_E_INVALID, "%s: workspace too small", who);
    const BnSlicing sl = bn_slicing(n, c);
    const int vec = aligned(dz, 16) && aligned(x, 16) && aligned(dx, 16) && (!residual || aligned(residual, 16));
    double *ws = static_cast<double *>(workspace);
    hipLaunchKernelGGL(bn_running_backward_kernel, dim3(sl.slices, c), dim3(kBnThreads), 0, as_stream(stream), dz, x, residual,
                       gamma, running_mean, running_var, dx, ws, n, c, h * w, sl.planes_per_slice, vec, eps);
    if (int rc = check_launch("bn_running_backward_kernel")) return rc;
    hipLaunchKernelGGL(bn_backward_finish_kernel, dim3((c + kWave - 1) / kWave), dim3(kWave), 0, as_stream(stream),
                       (const double *)ws, running_var, dgamma, dbeta, c, sl.slices, eps, accumulate);
    return check_launch("bn_backward_finish_kernel");
}
