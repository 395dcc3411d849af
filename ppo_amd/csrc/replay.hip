// Experience replay on the device (gfx950) - the reference keeps its buffer in host NumPy (rl/replay.py) and moves rows
// one by one in Python; here the buffer lies in HBM next to the rollout and
//
//  * ppo_replay_scatter_rows        dst[spot[i]] = src[id[i]]: an add (rl/replay.py:255-256 the grow, :270-273 the
//                                   per-row loop), observation row and 16-float aux record in one launch
//  * ppo_replay_gather_rows2        dst[i] = sample[i] < n_a ? a[sample[i]] : b[sample[i] - n_a]: a sample of the buffer,
//                                   or of buffer + rollout with --replay_mixing (rl/rollout.py:2016-2048, the
//                                   np.concatenate and the fancy index), one launch for the whole distil batch
//  * ppo_replay_pairwise_sqdist_u8  all M x M squared L2 distances of M <= 128 picked uint8 rows as exact int64 (the
//                                   float32 torch.cdist of rl/replay.py:99-111, which the host turns into sqrt(d2) / 255)
//
// Rows are opaque bytes.  No atomics; every launch gives the same bits.  An index outside its buffer is clamped into it:
// nothing is read or written outside either buffer whatever the index vectors hold.
#include "common.h"

namespace ppo {
namespace {

constexpr int kAux = PPO_REPLAY_AUX_FLOATS;

// one row of row_bytes bytes, by the 256 threads of a workgroup; `vec`: both rows 16-byte aligned, row_bytes % 16 == 0
__device__ __forceinline__ void copy_row(const uint8_t *__restrict__ sp, uint8_t *__restrict__ dp, int64_t row_bytes, bool vec)
{
    if (vec) {
        const int64_t n16 = row_bytes >> 4;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(sp);
        uint4 *d4 = reinterpret_cast<uint4 *>(dp);
        // eight 16-byte loads in flight per thread before the first store (the form measured for gather_rows_kernel,
        // batch_ops.hip)
        for (int64_t i0 = threadIdx.x; i0 < n16; i0 += 256 * 8) {
            uint4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t i = i0 + 256 * u;
                v[u] = s4[i < n16 ? i : i0];  // clamped address, unconditional load
            }
            // pins the eight loads above the stores: left alone, the compiler sinks each load into its store's branch and
            // the copy pays one memory round trip after the other
#pragma unroll
            for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(v[u].x), "+v"(v[u].y), "+v"(v[u].z), "+v"(v[u].w));
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t i = i0 + 256 * u;
                if (i < n16) d4[i] = v[u];
            }
        }
    } else {
        for (int64_t i = threadIdx.x; i < row_bytes; i += 256) dp[i] = sp[i];
    }
}

__device__ __forceinline__ int64_t clamp_row(int64_t r, int64_t n) { return r < 0 ? 0 : (r >= n ? n - 1 : r); }

// one workgroup per moved row; the caller guarantees distinct destinations
__global__ __launch_bounds__(256) void scatter_rows_kernel(const uint8_t *__restrict__ src, const float *__restrict__ src_aux,
                                                           int64_t n_src_rows, int64_t row_bytes,
                                                           const int32_t *__restrict__ id, const int32_t *__restrict__ spot,
                                                           int n, uint8_t *__restrict__ dst, float *__restrict__ dst_aux,
                                                           int64_t n_dst_rows, int vec)
{
    const int r = blockIdx.x;
    if (r >= n) return;
    const int64_t s = clamp_row(id[r], n_src_rows);
    const int64_t d = clamp_row(spot[r], n_dst_rows);
    copy_row(src + s * row_bytes, dst + d * row_bytes, row_bytes, vec != 0);
    if (src_aux != nullptr && threadIdx.x < kAux) dst_aux[d * kAux + threadIdx.x] = src_aux[s * kAux + threadIdx.x];
}

// one workgroup per sampled row
__global__ __launch_bounds__(256) void gather_rows2_kernel(const uint8_t *__restrict__ a, const float *__restrict__ a_aux,
                                                           int64_t n_a, const uint8_t *__restrict__ b,
                                                           const float *__restrict__ b_aux, int64_t n_b, int64_t row_bytes,
                                                           const int32_t *__restrict__ sample, int n,
                                                           uint8_t *__restrict__ dst, float *__restrict__ dst_aux, int vec)
{
    const int r = blockIdx.x;
    if (r >= n) return;
    const int64_t s = clamp_row(sample[r], n_a + n_b);
    const bool from_b = s >= n_a;  // (n_b == 0: never)
    const int64_t row = from_b ? s - n_a : s;
    copy_row((from_b ? b : a) + row * row_bytes, dst + (int64_t)r * row_bytes, row_bytes, vec != 0);
    if (dst_aux != nullptr && threadIdx.x < kAux)
        dst_aux[(int64_t)r * kAux + threadIdx.x] = (from_b ? b_aux : a_aux)[row * kAux + threadIdx.x];
}

// sum of the four byte products of two packed words, added to acc (wraps mod 2^32; the callers widen before it can)
__device__ __forceinline__ uint32_t dot4(uint32_t x, uint32_t y, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(x, y, acc, false);
#else
    for (int k = 0; k < 4; ++k) acc += ((x >> (8 * k)) & 255u) * ((y >> (8 * k)) & 255u);
    return acc;
#endif
}

constexpr int kTile = 4;  // a workgroup forms the kTile x kTile pairs of two groups of kTile rows
// a thread's 32-bit partial sums are widened to 64 bits after this many 16-byte steps: each step adds at most
// 4 * 4 * 255^2 = 1040400 to a sum, and 2048 * 1040400 < 2^32
constexpr int kWiden = 2048;

// d2(i, j) = |x_i|^2 + |x_j|^2 - 2 x_i . x_j, all three as exact integer sums of byte products (64-bit once a thread's
// 32-bit partial could wrap); the workgroups on and above the diagonal write both (i, j) and (j, i)
__global__ __launch_bounds__(256) void pairwise_sqdist_kernel(const uint8_t *__restrict__ data, int64_t n_rows, int64_t D,
                                                              const int32_t *__restrict__ index, int M,
                                                              int64_t *__restrict__ out, int vec)
{
    if (blockIdx.y < blockIdx.x) return;
    __shared__ unsigned long long part[4][kTile * kTile + 2 * kTile];
    const uint8_t *ri[kTile], *rj[kTile];
#pragma unroll
    for (int k = 0; k < kTile; ++k) {
        const int i = min((int)blockIdx.x * kTile + k, M - 1), j = min((int)blockIdx.y * kTile + k, M - 1);
        ri[k] = data + clamp_row(index[i], n_rows) * D;
        rj[k] = data + clamp_row(index[j], n_rows) * D;
    }
    unsigned long long xy[kTile][kTile] = {}, ni[kTile] = {}, nj[kTile] = {};
    if (vec) {
        const int64_t n16 = D >> 4;
        for (int64_t base = 0; base < n16; base += (int64_t)256 * kWiden) {
            uint32_t xy32[kTile][kTile] = {}, ni32[kTile] = {}, nj32[kTile] = {};
            const int64_t end = base + (int64_t)256 * kWiden < n16 ? base + (int64_t)256 * kWiden : n16;
            for (int64_t v = base + threadIdx.x; v < end; v += 256) {
                uint4 a[kTile], b[kTile];
#pragma unroll
                for (int k = 0; k < kTile; ++k) {
                    a[k] = reinterpret_cast<const uint4 *>(ri[k])[v];
                    b[k] = reinterpret_cast<const uint4 *>(rj[k])[v];
                }
#pragma unroll
                for (int k = 0; k < kTile; ++k) {
                    const uint32_t aw[4] = {a[k].x, a[k].y, a[k].z, a[k].w};
                    const uint32_t bw[4] = {b[k].x, b[k].y, b[k].z, b[k].w};
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        ni32[k] = dot4(aw[w], aw[w], ni32[k]);
                        nj32[k] = dot4(bw[w], bw[w], nj32[k]);
                    }
#pragma unroll
                    for (int l = 0; l < kTile; ++l) {
                        const uint32_t lw[4] = {b[l].x, b[l].y, b[l].z, b[l].w};
#pragma unroll
                        for (int w = 0; w < 4; ++w) xy32[k][l] = dot4(aw[w], lw[w], xy32[k][l]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kTile; ++k) {
                ni[k] += ni32[k];
                nj[k] += nj32[k];
#pragma unroll
                for (int l = 0; l < kTile; ++l) xy[k][l] += xy32[k][l];
            }
        }
    } else {
        // rows that are not 16-byte aligned (D % 16 != 0 or an offset base): a byte at a time, 64-bit sums
        for (int64_t e = threadIdx.x; e < D; e += 256) {
            uint32_t a[kTile], b[kTile];
#pragma unroll
            for (int k = 0; k < kTile; ++k) {
                a[k] = ri[k][e];
                b[k] = rj[k][e];
            }
#pragma unroll
            for (int k = 0; k < kTile; ++k) {
                ni[k] += a[k] * a[k];
                nj[k] += b[k] * b[k];
#pragma unroll
                for (int l = 0; l < kTile; ++l) xy[k][l] += a[k] * b[l];
            }
        }
    }
    // integer sums: any order of the reduction gives the same value
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int q = 0; q < kTile * kTile + 2 * kTile; ++q) {
        unsigned long long v = q < kTile * kTile ? xy[q / kTile][q % kTile]
                                                 : (q < kTile * kTile + kTile ? ni[q - kTile * kTile] : nj[q - kTile * kTile - kTile]);
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
        if (lane == 0) part[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < kTile * kTile) {
        const int k = threadIdx.x / kTile, l = threadIdx.x % kTile;
        const int i = blockIdx.x * kTile + k, j = blockIdx.y * kTile + l;
        if (i < M && j < M) {
            unsigned long long dot = 0, a2 = 0, b2 = 0;
            for (int w = 0; w < 4; ++w) {
                dot += part[w][k * kTile + l];
                a2 += part[w][kTile * kTile + k];
                b2 += part[w][kTile * kTile + kTile + l];
            }
            const int64_t d2 = (int64_t)(a2 + b2) - 2 * (int64_t)dot;
            out[(int64_t)i * M + j] = d2;
            out[(int64_t)j * M + i] = d2;
        }
    }
}

}  // namespace
}  // namespace ppo

extern "C" int ppo_replay_scatter_rows(const void *src, const float *src_aux, int64_t n_src_rows, int64_t row_bytes,
                                       const int32_t *id, const int32_t *spot, int n, void *dst, float *dst_aux,
                                       int64_t n_dst_rows, void *stream)
{
    using namespace ppo;
    if (row_bytes <= 0 || n < 0 || n_src_rows <= 0 || n_dst_rows <= 0)
        return fail(PPO_E_INVALID, "ppo_replay_scatter_rows: bad shape");
    if (n == 0) return PPO_OK;
    if (!src || !id || !spot || !dst || (src_aux == nullptr) != (dst_aux == nullptr))
        return fail(PPO_E_INVALID, "ppo_replay_scatter_rows: null pointer");
    if (!aligned(src_aux, 4) || !aligned(dst_aux, 4)) return fail(PPO_E_ALIGN, "ppo_replay_scatter_rows: aux not 4-byte aligned");
    const int vec = (row_bytes & 15) == 0 && aligned(src, 16) && aligned(dst, 16);
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(n), dim3(256), 0, as_stream(stream), static_cast<const uint8_t *>(src), src_aux,
                       n_src_rows, row_bytes, id, spot, n, static_cast<uint8_t *>(dst), dst_aux, n_dst_rows, vec);
    return check_launch("scatter_rows_kernel");
}

extern "C" int ppo_replay_gather_rows2(const void *a, const float *a_aux, int64_t n_a, const void *b, const float *b_aux,
                                       int64_t n_b, int64_t row_bytes, const int32_t *sample, int n, void *dst,
                                       float *dst_aux, void *stream)
{
    using namespace ppo;
    if (row_bytes <= 0 || n < 0 || n_a < 0 || n_b < 0 || n_a + n_b <= 0)
        return fail(PPO_E_INVALID, "ppo_replay_gather_rows2: bad shape");
    if (n == 0) return PPO_OK;
    if ((n_a > 0 && !a) || (n_b > 0 && !b) || !sample || !dst)
        return fail(PPO_E_INVALID, "ppo_replay_gather_rows2: null pointer");
    if (dst_aux && ((n_a > 0 && !a_aux) || (n_b > 0 && !b_aux)))
        return fail(PPO_E_INVALID, "ppo_replay_gather_rows2: null pointer (aux)");
    if (!aligned(a_aux, 4) || !aligned(b_aux, 4) || !aligned(dst_aux, 4))
        return fail(PPO_E_ALIGN, "ppo_replay_gather_rows2: aux not 4-byte aligned");
    const int vec = (row_bytes & 15) == 0 && (n_a == 0 || aligned(a, 16)) && (n_b == 0 || aligned(b, 16)) && aligned(dst, 16);
    hipLaunchKernelGGL(gather_rows2_kernel, dim3(n), dim3(256), 0, as_stream(stream), static_cast<const uint8_t *>(a), a_aux, n_a,
                       static_cast<const uint8_t *>(b), b_aux, n_b, row_bytes, sample, n, static_cast<uint8_t *>(dst), dst_aux,
                       vec);
    return check_launch("gather_rows2_kernel");
}

extern "C" int ppo_replay_pairwise_sqdist_u8(const uint8_t *data, int64_t n_rows, int64_t D, const int32_t *index, int M,
                                             int64_t *out, void *stream)
{
    using namespace ppo;
    if (n_rows <= 0 || D <= 0 || M < 0 || M > PPO_REPLAY_MAX_PAIRWISE_ROWS)
        return fail(PPO_E_INVALID, "ppo_replay_pairwise_sqdist_u8: bad shape (1 <= M <= %d rows)", PPO_REPLAY_MAX_PAIRWISE_ROWS);
    if (M == 0) return PPO_OK;
    if (!data || !index || !out) return fail(PPO_E_INVALID, "ppo_replay_pairwise_sqdist_u8: null pointer");
    if (!aligned(out, 8)) return fail(PPO_E_ALIGN, "ppo_replay_pairwise_sqdist_u8: out not 8-byte aligned");
    const int vec = (D & 15) == 0 && aligned(data, 16);
    const unsigned tiles = (unsigned)((M + kTile - 1) / kTile);
    hipLaunchKernelGGL(pairwise_sqdist_kernel, dim3(tiles, tiles), dim3(256), 0, as_stream(stream), data, n_rows, D, index, M, out,
                       vec);
    return check_launch("pairwise_sqdist_kernel");
}
