// State hashing (gfx950): exploration counts and the count-based novelty bonus of the reference
// (rl/hash.py LinearStateHasher, rl/rollout.py:652-699 generate_hashes, :755-762 the per-step counts, :895-924 the bonus,
// :1243-1250 the log lines).  The reference hashes on the host, in a Python loop over envs at every env step; here the
// observations never leave HBM and neither do the hashes.
//
//  * hash kernel    one workgroup of 1024 threads per observation row.  Thread j owns elements 4 (j + 1024 k) + 0..3,
//                   k = 0, 1, ...: it forms each x in float32 (quantise, then raw / raw - 128 / the normaliser's
//                   clamp((o / 255 - mu) / (std + eps), -5, 5) [+ 3]), promotes x and w to float64 and keeps the `bits`
//                   partial sums of w * x in registers - a float32 x float32 product is exact in float64, so the only
//                   rounding is that of the float64 sum.  The 1024 partial sums are combined by a butterfly inside each
//                   wave and by ((w0 + w1) + w2) + ... + w15 across the sixteen waves; the bias is added last.  The order
//                   depends on D alone - not on B, on the launch shape or on whether the 4-wide loads apply (the scalar
//                   path walks the same elements in the same order) - so a row's hash is the same bits wherever and
//                   however often it is computed.  Each observation byte is read once, x is never materialised, and with
//                   one plane of a frame stack only that plane's bytes are read (the row stride is C * H * W).
//                   The launch is bound by latency: 128 rows x 7056 bytes, the [bits, D] weights come out of L2.
//  * counts kernel  the reference's sequence - for t: recent *= decay; for a: global[h] += 1, recent[h] += 1 - is a
//                   sequence per bin: what happens to one bin depends on that bin's hits alone.  One thread per bin, 1024
//                   bins per workgroup; per chunk of 8 steps the workgroup counts the hits of ITS bins into LDS
//                   (integer LDS atomics: any order gives the same count), then every thread walks the 8 steps of its
//                   bin: one rounded multiplication per step and one rounded `+ 1.0` per hit.  Every addend is 1.0, so the
//                   result does not depend on the order of a step's hits and equals the reference's float64 loop bit
//                   for bit.  One launch per rollout, no grid-wide barrier, no float atomics.  An entry outside
//                   [0, n_bins) belongs to no workgroup's range and is never written through.
//  * bonus kernel   int_rewards[i] = float32(float64(int_rewards[i]) + bonus * g(recent[hashes[i]])), product and sum
//                   rounded separately (__dmul_rn / __dadd_rn: the build allows contraction).
//  * stats kernel   count_nonzero(global) and the number of recent bins >= 1 (count_nonzero(recent.astype(int)), the
//                   counts being non-negative), block sums added with integer atomics into a zeroed pair.
#include "common.h"

namespace ppo {
namespace {

constexpr int kHashThreads = 1024;  // 16 waves on one CU: the loop over D is 2 trips at D = 7056, the launch is latency
constexpr int kHashWaves = kHashThreads / kWave;
constexpr int kMaxBits = 24;

__device__ __forceinline__ float normalise(float v, float m, float s, float eps)
{
    return fminf(fmaxf((v - m) / (s + eps), -5.0f), 5.0f);  // csrc/obs_norm.hip: IEEE subtract / add / divide
}

// the normed modes come in three preparations of the byte (--observation_scaling): o/255, o/255 - 0.5, (o/255 - 0.5) * 6
constexpr bool hash_mode_normed(int mode)
{
    return mode == PPO_HASH_NORMED || mode == PPO_HASH_NORMED_OFFSET || (mode >= PPO_HASH_NORMED_CENTERED && mode <= PPO_HASH_NORMED_OFFSET_UNIT);
}
constexpr bool hash_mode_known(int mode) { return (mode >= PPO_HASH_RAW && mode <= PPO_HASH_NORMED_OFFSET) || hash_mode_normed(mode); }
constexpr bool hash_mode_offset(int mode)
{
    return mode == PPO_HASH_NORMED_OFFSET || mode == PPO_HASH_NORMED_OFFSET_CENTERED || mode == PPO_HASH_NORMED_OFFSET_UNIT;
}

// prep_for_model (rl/models.py:846-855) of one byte, each operation rounded on its own (no contraction: fused with
// normalise()'s `- m` the product would skip a rounding)
template <int MODE>
__device__ __forceinline__ float prepared(unsigned o)
{
#pragma clang fp contract(off)
    float p = (float)o / 255.0f;
    if constexpr (MODE >= PPO_HASH_NORMED_CENTERED) p = p - 0.5f;
    if constexpr (MODE >= PPO_HASH_NORMED_UNIT) p = p * 6.0f;
    return p;
}

// one element of the hash input from one observation byte (rl/rollout.py:670-684)
template <int MODE>
__device__ __forceinline__ float hash_input(unsigned o, unsigned q, float m, float s, float eps)
{
    if (q > 1u) o = (o / q) * q;
    if constexpr (MODE == PPO_HASH_RAW) return (float)o;
    if constexpr (MODE == PPO_HASH_RAW_CENTERED) return (float)o - 128.0f;
    const float v = normalise(prepared<MODE>(o), m, s, eps);
    if constexpr (!hash_mode_offset(MODE)) return v;
    return v + 3.0f;
}

// NB: `bits` rounded up to 8 / 16 / 24, the number of partial sums a thread keeps; VEC: D, the row stride and every pointer
// allow 4-wide loads.  Same elements per thread and same order in both forms.
template <int NB, int MODE, bool VEC>
__global__ __launch_bounds__(kHashThreads) void state_hash_kernel(const uint8_t *__restrict__ obs, size_t row_stride, int D,
                                                                  unsigned q, const float *__restrict__ mu,
                                                                  const float *__restrict__ std, float eps,
                                                                  const float *__restrict__ w, const float *__restrict__ bias,
                                                                  int bits, int32_t *__restrict__ out)
{
    constexpr bool kNormed = hash_mode_normed(MODE);
    __shared__ double s_part[kHashWaves][NB];
    const uint8_t *row = obs + (size_t)blockIdx.x * row_stride;
    double acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i] = 0.0;

    for (int e = threadIdx.x * 4; e < D; e += kHashThreads * 4) {
        float x[4];
        if constexpr (VEC) {
            const uchar4 o = *reinterpret_cast<const uchar4 *>(row + e);
            float4 m = make_float4(0.f, 0.f, 0.f, 0.f), s = m;
            if constexpr (kNormed) {
                m = *reinterpret_cast<const float4 *>(mu + e);
                s = *reinterpret_cast<const float4 *>(std + e);
            }
            x[0] = hash_input<MODE>(o.x, q, m.x, s.x, eps);
            x[1] = hash_input<MODE>(o.y, q, m.y, s.y, eps);
            x[2] = hash_input<MODE>(o.z, q, m.z, s.z, eps);
            x[3] = hash_input<MODE>(o.w, q, m.w, s.w, eps);
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                if (i < bits) {  // uniform
                    const float4 wv = *reinterpret_cast<const float4 *>(w + (size_t)i * D + e);
                    acc[i] += (double)wv.x * (double)x[0];
                    acc[i] += (double)wv.y * (double)x[1];
                    acc[i] += (double)wv.z * (double)x[2];
                    acc[i] += (double)wv.w * (double)x[3];
                }
            }
        } else {
            const int n = D - e < 4 ? D - e : 4;
            for (int k = 0; k < n; ++k) {
                float m = 0.f, s = 0.f;
                if constexpr (kNormed) m = mu[e + k], s = std[e + k];
                x[k] = hash_input<MODE>(row[e + k], q, m, s, eps);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                if (i < bits) {
                    for (int k = 0; k < n; ++k) acc[i] += (double)w[(size_t)i * D + e + k] * (double)x[k];
                }
            }
        }
    }

    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
#pragma unroll
        for (int s = kWave / 2; s > 0; s >>= 1) acc[i] += __shfl_xor(acc[i], s, kWave);
        if (lane == 0) s_part[wave][i] = acc[i];
    }
    __syncthreads();
    if (wave == 0) {
        bool bit = false;
        if (lane < bits) {
            double p = s_part[0][lane];
#pragma unroll
            for (int k = 1; k < kHashWaves; ++k) p += s_part[k][lane];
            bit = p + (double)bias[lane] > 0.0;
        }
        const unsigned long long mask = __ballot(bit);
        if (lane == 0) out[blockIdx.x] = (int32_t)(mask & ((1ull << bits) - 1ull));
    }
}

constexpr int kBinsPerBlock = 1024;  // one thread per bin
constexpr int kStepChunk = 8;        // steps whose hit counts are held in LDS together: 8 x 1024 x 4 bytes

__global__ __launch_bounds__(kBinsPerBlock) void hash_counts_kernel(const int32_t *__restrict__ hashes, int N, int A,
                                                                    double decay, double *__restrict__ global_counts,
                                                                    double *__restrict__ recent_counts, long long n_bins)
{
    __shared__ unsigned s_hits[kStepChunk][kBinsPerBlock];
    const long long base = (long long)blockIdx.x * kBinsPerBlock;
    const long long bin = base + threadIdx.x;
    const bool live = bin < n_bins;
    double g = 0.0, r = 0.0;
    bool touched = false;
    if (live) r = recent_counts[bin];
    for (int t0 = 0; t0 < N; t0 += kStepChunk) {
        const int steps = N - t0 < kStepChunk ? N - t0 : kStepChunk;
        for (int k = 0; k < steps; ++k) s_hits[k][threadIdx.x] = 0u;
        __syncthreads();
        const int entries = steps * A;
        for (int j = threadIdx.x; j < entries; j += kBinsPerBlock) {
            const long long off = (long long)hashes[(size_t)t0 * A + j] - base;
            // a range check in the block's own coordinates: entries of other blocks, negative entries and entries
            // >= n_bins (base + off >= n_bins) all fall outside
            if (off >= 0 && off < kBinsPerBlock && base + off < n_bins) atomicAdd(&s_hits[j / A][off], 1u);
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k < steps; ++k) {
                r = __dmul_rn(r, decay);
                const unsigned hits = s_hits[k][threadIdx.x];
                if (hits != 0u && !touched) {
                    touched = true;
                    g = global_counts[bin];
                }
                for (unsigned h = 0; h < hits; ++h) {
                    g = __dadd_rn(g, 1.0);
                    r = __dadd_rn(r, 1.0);
                }
            }
        }
        __syncthreads();
    }
    if (live) {
        recent_counts[bin] = r;
        if (touched) global_counts[bin] = g;
    }
}

__global__ __launch_bounds__(256) void hash_bonus_kernel(const int32_t *__restrict__ hashes, const double *__restrict__ recent,
                                                         long long n_bins, int method, double threshold, double bonus,
                                                         float *__restrict__ rewards, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long h = hashes[i];
    if (h < 0 || h >= n_bins) return;
    const double c = recent[h];
    double g;
    if (method == PPO_HASH_BONUS_HYPERBOLIC) g = 1.0 / c;
    else if (method == PPO_HASH_BONUS_QUADRATIC) g = 1.0 / __dmul_rn(c, c);
    else g = c < threshold ? 1.0 : -1.0;
    rewards[i] = (float)__dadd_rn((double)rewards[i], __dmul_rn(bonus, g));
}

__global__ __launch_bounds__(256) void hash_count_stats_kernel(const double *__restrict__ global_counts,
                                                               const double *__restrict__ recent_counts, long long n_bins,
                                                               unsigned long long *__restrict__ out)
{
    __shared__ unsigned s_g[256 / kWave], s_r[256 / kWave];
    unsigned g = 0u, r = 0u;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_bins; i += (long long)gridDim.x * blockDim.x) {
        g += global_counts[i] != 0.0 ? 1u : 0u;
        r += recent_counts[i] >= 1.0 ? 1u : 0u;
    }
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) {
        g += __shfl_xor(g, s, kWave);
        r += __shfl_xor(r, s, kWave);
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (lane == 0) s_g[wave] = g, s_r[wave] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned tg = 0u, tr = 0u;
        for (int k = 0; k < 256 / kWave; ++k) tg += s_g[k], tr += s_r[k];
        if (tg) atomicAdd(&out[0], (unsigned long long)tg);
        if (tr) atomicAdd(&out[1], (unsigned long long)tr);
    }
}

template <int NB, int MODE>
void launch_hash(bool vec, int B, hipStream_t st, const uint8_t *obs, size_t row_stride, int D, unsigned q, const float *mu,
                 const float *std, float eps, const float *w, const float *bias, int bits, int32_t *out)
{
    if (vec)
        hipLaunchKernelGGL((state_hash_kernel<NB, MODE, true>), dim3(B), dim3(kHashThreads), 0, st, obs, row_stride, D, q, mu,
                           std, eps, w, bias, bits, out);
    else
        hipLaunchKernelGGL((state_hash_kernel<NB, MODE, false>), dim3(B), dim3(kHashThreads), 0, st, obs, row_stride, D, q, mu,
                           std, eps, w, bias, bits, out);
}

template <int NB, typename... Args>
void launch_hash_mode(int mode, Args... a)
{
    switch (mode) {
    case PPO_HASH_RAW: launch_hash<NB, PPO_HASH_RAW>(a...); break;
    case PPO_HASH_RAW_CENTERED: launch_hash<NB, PPO_HASH_RAW_CENTERED>(a...); break;
    case PPO_HASH_NORMED: launch_hash<NB, PPO_HASH_NORMED>(a...); break;
    case PPO_HASH_NORMED_OFFSET: launch_hash<NB, PPO_HASH_NORMED_OFFSET>(a...); break;
    case PPO_HASH_NORMED_CENTERED: launch_hash<NB, PPO_HASH_NORMED_CENTERED>(a...); break;
    case PPO_HASH_NORMED_OFFSET_CENTERED: launch_hash<NB, PPO_HASH_NORMED_OFFSET_CENTERED>(a...); break;
    case PPO_HASH_NORMED_UNIT: launch_hash<NB, PPO_HASH_NORMED_UNIT>(a...); break;
    default: launch_hash<NB, PPO_HASH_NORMED_OFFSET_UNIT>(a...); break;
    }
}

}  // namespace
}  // namespace ppo

extern "C" int ppo_state_hash_i32(const uint8_t *obs, int B, int C, int H, int W, int planes, int quantize, int mode,
                                  const float *mu, const float *std, float eps, const float *weight, const float *bias,
                                  int bits, int32_t *out, void *stream)
{
    using namespace ppo;
    if (B < 0 || C <= 0 || H <= 0 || W <= 0 || (long long)C * H * W >= (1ll << 31))
        return fail(PPO_E_INVALID, "ppo_state_hash_i32: bad shape [%d, %d, %d, %d]", B, C, H, W);
    if (planes != 1 && planes != C)
        return fail(PPO_E_INVALID, "ppo_state_hash_i32: planes %d is neither 1 nor C = %d", planes, C);
    if (bits < 1 || bits > kMaxBits) return fail(PPO_E_INVALID, "ppo_state_hash_i32: bits %d outside [1, %d]", bits, kMaxBits);
    if (quantize < 0 || quantize > 255) return fail(PPO_E_INVALID, "ppo_state_hash_i32: quantize %d outside [0, 255]", quantize);
    if (!hash_mode_known(mode)) return fail(PPO_E_INVALID, "ppo_state_hash_i32: bad mode %d", mode);
    const bool normed = hash_mode_normed(mode);
    if (!obs || !weight || !bias || !out || (normed && (!mu || !std)))
        return fail(PPO_E_INVALID, "ppo_state_hash_i32: null pointer");
    if (B == 0) return PPO_OK;
    const size_t row_stride = (size_t)C * H * W;
    const int D = planes * H * W;
    const bool vec = D % 4 == 0 && row_stride % 4 == 0 && aligned(obs, 4) && aligned(weight, 16) &&
                     (!normed || (aligned(mu, 16) && aligned(std, 16)));
    hipStream_t st = as_stream(stream);
    const unsigned q = (unsigned)quantize;
    if (bits <= 8) launch_hash_mode<8>(mode, vec, B, st, obs, row_stride, D, q, mu, std, eps, weight, bias, bits, out);
    else if (bits <= 16) launch_hash_mode<16>(mode, vec, B, st, obs, row_stride, D, q, mu, std, eps, weight, bias, bits, out);
    else launch_hash_mode<24>(mode, vec, B, st, obs, row_stride, D, q, mu, std, eps, weight, bias, bits, out);
    return check_launch("state_hash_kernel");
}

extern "C" int ppo_hash_counts_update_f64(const int32_t *hashes, int N, int A, double decay, double *global_counts,
                                          double *recent_counts, int64_t n_bins, void *stream)
{
    using namespace ppo;
    if (N < 0 || A <= 0 || n_bins <= 0 || n_bins > (1ll << kMaxBits) || (long long)N * A >= (1ll << 31))
        return fail(PPO_E_INVALID, "ppo_hash_counts_update_f64: bad shape [%d, %d] / n_bins %lld", N, A, (long long)n_bins);
    if (!hashes || !global_counts || !recent_counts) return fail(PPO_E_INVALID, "ppo_hash_counts_update_f64: null pointer");
    if (N == 0) return PPO_OK;
    const int blocks = (int)((n_bins + kBinsPerBlock - 1) / kBinsPerBlock);
    hipLaunchKernelGGL(hash_counts_kernel, dim3(blocks), dim3(kBinsPerBlock), 0, as_stream(stream), hashes, N, A, decay,
                       global_counts, recent_counts, (long long)n_bins);
    return check_launch("hash_counts_kernel");
}

extern "C" int ppo_hash_bonus_f32(const int32_t *hashes, int64_t n, const double *recent_counts, int64_t n_bins, int method,
                                  double threshold, double bonus, float *int_rewards, void *stream)
{
    using namespace ppo;
    if (n < 0 || n >= (1ll << 31) || n_bins <= 0 || n_bins > (1ll << kMaxBits))
        return fail(PPO_E_INVALID, "ppo_hash_bonus_f32: bad size %lld / n_bins %lld", (long long)n, (long long)n_bins);
    if (method < PPO_HASH_BONUS_HYPERBOLIC || method > PPO_HASH_BONUS_BINARY)
        return fail(PPO_E_INVALID, "ppo_hash_bonus_f32: bad method %d", method);
    if (!hashes || !recent_counts || !int_rewards) return fail(PPO_E_INVALID, "ppo_hash_bonus_f32: null pointer");
    if (n == 0) return PPO_OK;
    hipLaunchKernelGGL(hash_bonus_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), hashes,
                       recent_counts, (long long)n_bins, method, threshold, bonus, int_rewards, (long long)n);
    return check_launch("hash_bonus_kernel");
}

extern "C" int ppo_hash_count_stats(const double *global_counts, const double *recent_counts, int64_t n_bins, int64_t *out,
                                    void *stream)
{
    using namespace ppo;
    if (n_bins <= 0 || n_bins > (1ll << kMaxBits)) return fail(PPO_E_INVALID, "ppo_hash_count_stats: bad n_bins %lld", (long long)n_bins);
    if (!global_counts || !recent_counts || !out) return fail(PPO_E_INVALID, "ppo_hash_count_stats: null pointer");
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(out, 0, 2 * sizeof(int64_t), st);
    if (e != hipSuccess) return fail(PPO_E_HIP, "ppo_hash_count_stats: memset: %s", hipGetErrorString(e));
    const long long want = (n_bins + 255) / 256;
    hipLaunchKernelGGL(hash_count_stats_kernel, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, st, global_counts,
                       recent_counts, (long long)n_bins, reinterpret_cast<unsigned long long *>(out));
    return check_launch("hash_count_stats_kernel");
}
