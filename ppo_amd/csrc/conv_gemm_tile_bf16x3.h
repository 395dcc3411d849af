// The split-bf16 form of the generic implicit-GEMM tile loop (csrc/conv_gemm_tile.h): the same `Op` contract, the
// same 64 x 32 tile of C per workgroup of four waves, every product as THREE v_mfma_f32_16x16x32_bf16 on (hi, lo) splits
// of both operands with float32 accumulation - the arithmetic in the header of stack_bf16x3.hip:
//
//   x = hi + lo + r,  hi = bf16(x),  lo = bf16(x - hi),  |r| <= 2^-17 |x|
//   a * b  ~=  a_hi * b_hi  +  a_hi * b_lo  +  a_lo * b_hi        (dropped: a_lo * b_lo ~ 2^-16, the r terms ~ 2^-17)
//
// Operands are gathered as float32 through op.load_a / op.load_b exactly as in the exact loop (so the uint8 x / 255,
// the ReLU / leaky gates and the row of ones of a weight gradient come with them) and split on their way into LDS; no
// packed weights, no second copy of any index arithmetic.  Every global access is predicated on its own bounds: rows
// past M, columns past N and the K tail are staged as zeros (whose split is 0, 0) and never stored.  Non-finite inputs
// are outside the contract: for x = +-inf the split forms inf - inf and the result is NaN where the exact loop gives
// inf.
//
// K tile: 32.  Thread t gathers the two adjacent k of pair t & 15 for rows (t >> 4) + 16 j of A (j < 4) and of B^T
// (j < 2); the global loads of a tile are issued before the barrier that retires the previous tile's reads.  A pair
// goes to LDS as one packed 4-byte store per image (hi, lo).
//
// LDS layout.  Lane l of v_mfma_f32_16x16x32_bf16 supplies A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) +
// j][col l & 15], j < 8: with the eight k of a group contiguous that is ONE 16-byte read per fragment.  An image (A hi,
// A lo, B hi, B lo) is therefore k-group major, four planes [rows][8 bf16] (16 bytes a row):
//     byte(row, q) = (q & 1) * rows * 16 + (q >> 1) * (2 * rows * 16 + 32) + 16 * row        q = k group, 0 .. 3
//  - Reads (ds_read_b128: four groups of 16 lanes, e.g. lanes 0-3, 12-15 with 20-27; a lane covers 4 of 64 banks): a
//    group holds rows {0-3, 12-15} of plane q and rows {4-11} of plane q ^ 1.  Planes q and q ^ 1 lie rows * 16 bytes
//    = a multiple of 256 bytes apart (rows = 64, 32), i.e. on the same banks, so the 16 lanes read 16 consecutive
//    16-byte slots: all 64 banks once, conflict-free.  A wave's row offset (16 rows = 256 bytes) changes nothing.
//  - Staging writes (ds_write_b32: two groups of 32 lanes, banks = dword mod 32): a group is the 16 pairs of two
//    adjacent rows, 8 dwords per plane.  Planes 0 and 1 share banks, planes 2 and 3 sit 32 bytes = 8 banks further
//    (the + 32 above), so each of 16 banks takes two addresses.  That 2-way conflict remains; it is inside the
//    transfer time of a ds_write_b32 (4 cycles for 2 array cycles) and costs nothing.  (hipcc pairs the stores of rows
//    16 apart into ds_write2st64_b32, which is banked as the two ds_write_b32 it stands for.)
//
// C/D has the lane map of v_mfma_f32_16x16x4_f32, so the epilogue is the exact loop's.  Order: per K tile and
// accumulator lo * hi, hi * lo, hi * hi into a zeroed register, then the blocked sum of the exact loop (kFold tiles, then
// the folds); tiles and slabs ascending, no atomics: the same bits on every launch.  gemm_grid and the slab partition
// of a weight gradient (csi::slab_rows / slab_count with kMaxSlabs, aligned to the exact loop's kTK) are the exact
// loop's - a slab may begin in the middle of a 32-wide tile, which the k bounds cover - so
// ppo_conv2d_strided_wgrad_workspace_bytes serves both precisions.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_gemm_tile.h"
#include "mfma.h"

namespace ppo {
namespace tile {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

constexpr int kTK3 = 32;    // K tile of the split loop
constexpr int kSkew3 = 32;  // bytes between the plane pairs (0, 1) and (2, 3) beyond their size

constexpr int image_bytes(int rows) { return 4 * rows * 16 + kSkew3; }
__device__ __forceinline__ int image_off(int rows, int row, int q)
{
    return (q & 1) * rows * 16 + (q >> 1) * (2 * rows * 16 + kSkew3) + row * 16;
}

// the split of store_split4c (conv_bf16x3.hip), two adjacent k at a time
__device__ __forceinline__ void store_split_pair(unsigned char *hi_p, unsigned char *lo_p, float x0, float x1)
{
    bf16x2 hi, lo;
    hi[0] = (__bf16)x0, hi[1] = (__bf16)x1;
    lo[0] = (__bf16)(x0 - (float)hi[0]), lo[1] = (__bf16)(x1 - (float)hi[1]);
    *reinterpret_cast<bf16x2 *>(hi_p) = hi;
    *reinterpret_cast<bf16x2 *>(lo_p) = lo;
}

__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 a, bf16x8 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

template <class Op>
__global__ __launch_bounds__(kThreads) void conv_gemm_bf16x3_kernel(const Op op)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_a[2][image_bytes(kTM)];  // [hi, lo]
    __shared__ __attribute__((aligned(16))) unsigned char s_b[2][image_bytes(kTN)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * kTM, n0 = blockIdx.y * kTN;
    int k_begin, k_end;
    op.k_range(blockIdx.z, k_begin, k_end);
    const int kp = tid & 15, r0 = tid >> 4;  // k pair of the tile, first row

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
    // staging: pair kp is bytes 4 (kp & 3) .. + 3 of k group kp >> 2; fragments: k group lane >> 4
    const int a_wr = image_off(kTM, r0, kp >> 2) + 4 * (kp & 3), b_wr = image_off(kTN, r0, kp >> 2) + 4 * (kp & 3);
    const int a_rd = image_off(kTM, wave * 16 + (lane & 15), lane >> 4), b_rd = image_off(kTN, lane & 15, lane >> 4);

    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 sum0 = zero, sum1 = zero, mid0 = zero, mid1 = zero;
    int tiles = 0;
    for (int k0 = k_begin; k0 < k_end; k0 += kTK3) {
        float a[4][2], b[2][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int k = k0 + 2 * kp + e;
            const bool k_ok = k < k_end;
            const typename Op::KCtx kc = op.k_ctx(k_ok ? k : k_begin);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j][e] = (k_ok && a_ok[j]) ? op.load_a(a_row[j], kc) : 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j][e] = (k_ok && b_ok[j]) ? op.load_b(b_col[j], kc) : 0.0f;
        }
        __syncthreads();  // the previous tile has been read
#pragma unroll
        for (int j = 0; j < 4; ++j) store_split_pair(s_a[0] + a_wr + 256 * j, s_a[1] + a_wr + 256 * j, a[j][0], a[j][1]);
#pragma unroll
        for (int j = 0; j < 2; ++j) store_split_pair(s_b[0] + b_wr + 256 * j, s_b[1] + b_wr + 256 * j, b[j][0], b[j][1]);
        __syncthreads();
        const bf16x8 a_hi = *reinterpret_cast<const bf16x8 *>(s_a[0] + a_rd);
        const bf16x8 a_lo = *reinterpret_cast<const bf16x8 *>(s_a[1] + a_rd);
        const bf16x8 b0_hi = *reinterpret_cast<const bf16x8 *>(s_b[0] + b_rd);
        const bf16x8 b0_lo = *reinterpret_cast<const bf16x8 *>(s_b[1] + b_rd);
        const bf16x8 b1_hi = *reinterpret_cast<const bf16x8 *>(s_b[0] + b_rd + 256);
        const bf16x8 b1_lo = *reinterpret_cast<const bf16x8 *>(s_b[1] + b_rd + 256);
        // the small terms first; two independent chains
        f32x4 acc0 = mfma_bf16(a_lo, b0_hi, zero), acc1 = mfma_bf16(a_lo, b1_hi, zero);
        acc0 = mfma_bf16(a_hi, b0_lo, acc0), acc1 = mfma_bf16(a_hi, b1_lo, acc1);
        acc0 = mfma_bf16(a_hi, b0_hi, acc0), acc1 = mfma_bf16(a_hi, b1_hi, acc1);
        // blocked summation: a K tile's 32 products, then kFold tiles, then the folds
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

}  // namespace tile
}  // namespace ppo
