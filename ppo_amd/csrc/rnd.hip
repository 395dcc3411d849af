// Random Network Distillation (gfx950): the prediction error that is the intrinsic reward, its gradient w.r.t. the
// predictor's output, and the feature statistics the reference logs (rl/models.py:712-738, rl/rollout.py:1804-1822).
// HBM-bound: [B, F] with F = 512, a few hundred KB.
//
//  * rows kernel   one wave per row b: err[b] = mean_j (target - pred)^2, each lane summing j = lane, lane + 64, ...
//                  in ascending order and the 64 partial sums combined by a butterfly - a fixed order, the same bits on
//                  every launch - and dpred[b, j] = grad_scale * 2 (pred - target) / F, the gradient of
//                  grad_scale * sum_b err[b].
//  * stats kernel  (only when `stats` is given: the training minibatches, never the rollout) one workgroup; thread j
//                  walks the batch for features j, j + 256, ... (coalesced across threads) in float64, then a fixed
//                  tree over the workgroup.  The launches of a stream are ordered, so the row is updated by plain
//                  loads and stores of one thread: no atomics.
#include "common.h"

namespace ppo {
namespace {

constexpr int kRowsPerBlock = 4;  // waves of a 256-thread workgroup

__global__ __launch_bounds__(256) void rnd_error_rows_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                             int B, int F, float *__restrict__ err, long long err_stride,
                                                             float *__restrict__ dpred, float grad_scale)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int b = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (b >= B) return;  // whole waves leave: the shuffles below see full waves
    const float *p = pred + (size_t)b * F, *t = target + (size_t)b * F;
    const float g = grad_scale * 2.0f / (float)F;
    float acc = 0.0f;
    for (int j = lane; j < F; j += kWave) {
        const float d = t[j] - p[j];
        acc += d * d;
        if (dpred != nullptr) dpred[(size_t)b * F + j] = -g * d;
    }
#pragma unroll
    for (int w = kWave / 2; w > 0; w >>= 1) acc += __shfl_xor(acc, w, kWave);
    if (lane == 0 && err != nullptr) err[(long long)b * err_stride] = acc / (float)F;
}

// stats[0] += sum_b err[b], stats[1] += mean(target), stats[2] += mean_j var_b(target[:, j]) (unbiased, as torch.var),
// stats[3] = max(stats[3], max |target|), stats[4] += 1
__global__ __launch_bounds__(256) void rnd_stats_kernel(const float *__restrict__ pred, const float *__restrict__ target, int B,
                                                        int F, float *__restrict__ stats)
{
    __shared__ double s_e[256], s_s[256], s_v[256];
    __shared__ float s_m[256];
    double e = 0.0, sum = 0.0, var = 0.0;
    float mx = 0.0f;
    for (int j = threadIdx.x; j < F; j += 256) {
        double s = 0.0, q = 0.0;
#pragma unroll 8  // the loads of eight rows in flight together; the sums keep their order
        for (int b = 0; b < B; ++b) {
            const float tv = target[(size_t)b * F + j], d = tv - pred[(size_t)b * F + j];
            s += (double)tv;
            q += (double)tv * (double)tv;
            e += (double)d * (double)d;
            mx = fmaxf(mx, fabsf(tv));
        }
        sum += s;
        var += (q - s * s / (double)B) / (double)(B - 1);  // B = 1: 0 / 0, NaN as torch.var gives
    }
    s_e[threadIdx.x] = e, s_s[threadIdx.x] = sum, s_v[threadIdx.x] = var, s_m[threadIdx.x] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            s_e[threadIdx.x] += s_e[threadIdx.x + w];
            s_s[threadIdx.x] += s_s[threadIdx.x + w];
            s_v[threadIdx.x] += s_v[threadIdx.x + w];
            s_m[threadIdx.x] = fmaxf(s_m[threadIdx.x], s_m[threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] += (float)(s_e[0] / (double)F);
        stats[1] += (float)(s_s[0] / ((double)B * (double)F));
        stats[2] += (float)(s_v[0] / (double)F);
        stats[3] = fmaxf(stats[3], s_m[0]);
        stats[4] += 1.0f;
    }
}

}  // namespace
}  // namespace ppo

extern "C" int ppo_rnd_error_f32(const float *pred, const float *target, int B, int F, float *err, int64_t err_stride,
                                 float *dpred, float grad_scale, float *stats, void *stream)
{
    using namespace ppo;
    if (B <= 0 || F <= 0 || (long long)B * F >= (1ll << 31))
        return fail(PPO_E_INVALID, "ppo_rnd_error_f32: bad shape [%d, %d]", B, F);
    if (err != nullptr && err_stride < 1) return fail(PPO_E_INVALID, "ppo_rnd_error_f32: err_stride %lld < 1", (long long)err_stride);
    if (!pred || !target) return fail(PPO_E_INVALID, "ppo_rnd_error_f32: null pointer");
    if (!err && !dpred && !stats) return fail(PPO_E_INVALID, "ppo_rnd_error_f32: no output");
    hipStream_t st = as_stream(stream);
    if (err != nullptr || dpred != nullptr) {
        hipLaunchKernelGGL(rnd_error_rows_kernel, dim3((B + kRowsPerBlock - 1) / kRowsPerBlock), dim3(256), 0, st, pred, target,
                           B, F, err, (long long)err_stride, dpred, grad_scale);
        if (int rc = check_launch("rnd_error_rows_kernel")) return rc;
    }
    if (stats != nullptr) {
        hipLaunchKernelGGL(rnd_stats_kernel, dim3(1), dim3(256), 0, st, pred, target, B, F, stats);
        return check_launch("rnd_stats_kernel");
    }
    return PPO_OK;
}
