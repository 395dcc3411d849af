// The tile loop of the generic implicit-GEMM convolution kernels (conv_strided.hip: strided "valid" convolutions;
// conv3x3_any.hip: 3x3 / stride 1 / padding 1), on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32).  A kernel is this
// loop and an operand description `Op` (the row / column / K decomposition of its GEMM view, its loads and its store).
//
// Tile: a workgroup of four waves forms 64 x 32 of C; wave v owns rows 16 v .. 16 v + 15 as two 16 x 16 accumulators
// (two independent MFMA chains per wave).  K goes through LDS 16 at a time: thread t gathers column t & 15 of the K
// tile for rows (t >> 4) + 16 j of A (j < 4) and of B^T (j < 2) - global loads of a tile are issued before the barrier
// that retires the previous tile's reads - into [row][17] images: rows 17 floats apart put the 16 rows x 2 columns of
// one 32-lane half of a ds_read_b32 operand fetch on 32 different banks (one pair aside), and the writes likewise.
// Every global access is predicated on its own bounds: rows past M, columns past N and the K tail read as zeros and
// are never stored.  A sum over K is formed in blocks - the 16 products of a K tile in one MFMA chain, eight tiles, then
// the groups of eight - which keeps the rounding error of a K = 1024 sum near that of a K = 100 chain; the order is
// fixed (tiles and slabs ascending): no atomics, the same bits on every launch.
#pragma once
#include <hip/hip_runtime.h>

#include "mfma.h"

namespace ppo {
namespace tile {

constexpr int kTM = 64, kTN = 32, kTK = 16, kLd = kTK + 1, kThreads = 256;
constexpr int kMaxSlabs = 64;
constexpr int kFold = 8;  // K tiles per level of the blocked summation

// Op: M, N (extents of C); k_range(z, kb, ke) (the K range of grid slice z); a_row(m) / b_col(n) / k_ctx(k) (each index
// decomposed once); load_a(row, kctx) / load_b(col, kctx); store(m, n, value, z).
template <class Op>
__global__ __launch_bounds__(kThreads) void conv_gemm_kernel(const Op op)
{
    __shared__ float s_a[kTM][kLd];
    __shared__ float s_b[kTN][kLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * kTM, n0 = blockIdx.y * kTN;
    int k_begin, k_end;
    op.k_range(blockIdx.z, k_begin, k_end);
    const int kk = tid & 15, r0 = tid >> 4;

    typename Op::ARow a_row[4];
    bool a_ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + r0 + 16 * j;
        a_ok[j] = m < op.M;
        a_row[j] = op.a_row(a_ok[j] ? m : 0);
    }
    typename Op::BCol b_col[2];
    bool b_ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + r0 + 16 * j;
        b_ok[j] = n < op.N;
        b_col[j] = op.b_col(b_ok[j] ? n : 0);
    }

    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 sum0 = zero, sum1 = zero, mid0 = zero, mid1 = zero;
    int tiles = 0;
    for (int k0 = k_begin; k0 < k_end; k0 += kTK) {
        const int k = k0 + kk;
        const bool k_ok = k < k_end;
        const typename Op::KCtx kc = op.k_ctx(k_ok ? k : k_begin);
        float a[4], b[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = (k_ok && a_ok[j]) ? op.load_a(a_row[j], kc) : 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = (k_ok && b_ok[j]) ? op.load_b(b_col[j], kc) : 0.0f;
        __syncthreads();  // the previous tile has been read
#pragma unroll
        for (int j = 0; j < 4; ++j) s_a[r0 + 16 * j][kk] = a[j];
#pragma unroll
        for (int j = 0; j < 2; ++j) s_b[r0 + 16 * j][kk] = b[j];
        __syncthreads();
        f32x4 acc0 = zero, acc1 = zero;
#pragma unroll
        for (int s = 0; s < kTK / 4; ++s) {
            const float av = s_a[wave * 16 + (lane & 15)][s * 4 + (lane >> 4)];
            const float b0 = s_b[lane & 15][s * 4 + (lane >> 4)];
            const float b1 = s_b[16 + (lane & 15)][s * 4 + (lane >> 4)];
            acc0 = mfma16(av, b0, acc0);
            acc1 = mfma16(av, b1, acc1);
        }
        // blocked summation: a K tile's 16 products, then kFold tiles, then the folds
        mid0 += acc0, mid1 += acc1;
        if (++tiles == kFold) {
            sum0 += mid0, sum1 += mid1;
            mid0 = zero, mid1 = zero;
            tiles = 0;
        }
    }
    sum0 += mid0, sum1 += mid1;
    // lane l holds C[(l >> 4) * 4 + r][l & 15] of each 16 x 16 block in element r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + wave * 16 + (lane >> 4) * 4 + r;
        const int n = n0 + (lane & 15);
        if (m < op.M && n < op.N) op.store(m, n, sum0[r], blockIdx.z);
        if (m < op.M && n + 16 < op.N) op.store(m, n + 16, sum1[r], blockIdx.z);
    }
}

inline dim3 gemm_grid(int M, int N, int Z) { return dim3((M + kTM - 1) / kTM, (N + kTN - 1) / kTN, Z); }

}  // namespace tile
}  // namespace ppo
