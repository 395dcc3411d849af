// 2x2 / stride 2 max pooling with the ReLU behind it, NCHW float32 (reference: F.relu(torch.max_pool2d(., 2, 2)) at
// rl/models.py:203-205, the RTG encoder) and its gradient.  HBM-bound elementwise-class kernels.
//
// The pool floors: [n,c,h,w] -> [n,c,h/2,w/2], a trailing odd row or column belongs to no window.  Windows do not
// overlap, so the backward pass has one term per input element at most: no atomics, no summation order, and it writes
// every element of din itself (the trailing row / column as zeros).
//
// Forward optionally records one byte per window: the winning tap ky*2+kx (first maximum in row-major order - a strict
// '>' scan - with a NaN taking the window, as in PyTorch's kernel), or 4 where the pooled value is not > 0, i.e. where the
// ReLU is closed.  The byte is all the backward pass needs besides dout: it never reads an activation.
//
// Indexing: one thread per cell, flat over (plane, cell row, cell column) in 64 bits - never the plane in blockIdx.y,
// which ends at 65535 (1024 environments x 64 channels is one more).  Forward cells are the windows.  Backward cells are
// the 2x2 input blocks, ceil(h/2) x ceil(w/2) per plane: those of a trailing odd row or column hold no window and store
// zeros.  Where w is even and the base 8-byte aligned a cell's rows are 8-byte accesses (every row then starts on an
// even element); odd w - rows start at 4-byte offsets only - takes the scalar form.
#include "common.h"

namespace ppo {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxElements = (int64_t)1 << 30;
constexpr int kClosed = 4;  // gate value of a window whose pooled value is not > 0

template <bool PAIR>
__global__ __launch_bounds__(kThreads) void maxpool2x2_relu_fwd_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                       uint8_t *__restrict__ gate, int H, int W, int Ho,
                                                                       int Wo, int64_t n_windows)
{
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_windows) return;
    // n_windows < 2^30 (the host checks): 32-bit divisions
    const uint32_t per_plane = (uint32_t)(Ho * Wo);
    const uint32_t pl = (uint32_t)idx / per_plane;
    const uint32_t t = (uint32_t)idx - pl * per_plane;
    const uint32_t j = t / (uint32_t)Wo;
    const uint32_t k = t - j * (uint32_t)Wo;
    const float *src = in + ((int64_t)pl * H + 2 * j) * W + 2 * k;
    float v00, v01, v10, v11;
    if (PAIR) {
        const float2 r0 = *reinterpret_cast<const float2 *>(src);
        const float2 r1 = *reinterpret_cast<const float2 *>(src + W);
        v00 = r0.x, v01 = r0.y, v10 = r1.x, v11 = r1.y;
    } else {
        v00 = src[0], v01 = src[1], v10 = src[W], v11 = src[W + 1];
    }
    float best = v00;
    int tap = 0;
    if (v01 > best || v01 != v01) best = v01, tap = 1;
    if (v10 > best || v10 != v10) best = v10, tap = 2;
    if (v11 > best || v11 != v11) best = v11, tap = 3;
    const bool open = best > 0.f;
    out[idx] = (open || best != best) ? best : 0.f;  // relu keeps a NaN
    if (gate) gate[idx] = (uint8_t)(open ? tap : kClosed);
}

template <bool PAIR>
__global__ __launch_bounds__(kThreads) void maxpool2x2_relu_bwd_kernel(const float *__restrict__ dout,
                                                                       const uint8_t *__restrict__ gate,
                                                                       float *__restrict__ din, int H, int W, int Ho, int Wo,
                                                                       int Hc, int Wc, int64_t n_cells)
{
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_cells) return;
    // n_cells <= the elements of din < 2^30 (the host checks): 32-bit divisions
    const uint32_t per_plane = (uint32_t)(Hc * Wc);
    const uint32_t pl = (uint32_t)idx / per_plane;
    const uint32_t t = (uint32_t)idx - pl * per_plane;
    const uint32_t j = t / (uint32_t)Wc;
    const uint32_t k = t - j * (uint32_t)Wc;
    int tap = kClosed;
    float g = 0.f;
    if (j < (uint32_t)Ho && k < (uint32_t)Wo) {
        const int64_t o = ((int64_t)pl * Ho + j) * Wo + k;
        tap = gate[o];
        g = dout[o];
    }
    const float r00 = tap == 0 ? g : 0.f, r01 = tap == 1 ? g : 0.f, r10 = tap == 2 ? g : 0.f, r11 = tap == 3 ? g : 0.f;
    float *dst = din + ((int64_t)pl * H + 2 * j) * W + 2 * k;
    const bool row1 = 2 * j + 1 < (uint32_t)H;
    if (PAIR) {  // W even: every cell has both columns
        *reinterpret_cast<float2 *>(dst) = make_float2(r00, r01);
        if (row1) *reinterpret_cast<float2 *>(dst + W) = make_float2(r10, r11);
    } else {
        const bool col1 = 2 * k + 1 < (uint32_t)W;
        dst[0] = r00;
        if (col1) dst[1] = r01;
        if (row1) {
            dst[W] = r10;
            if (col1) dst[W + 1] = r11;
        }
    }
}

int check_shape(const char *what, int n, int c, int h, int w)
{
    if (n < 1 || c < 1 || h < 2 || w < 2)
        return fail(PPO_E_INVALID, "%s: bad shape n=%d c=%d on %dx%d (n, c >= 1; h, w >= 2)", what, n, c, h, w);
    if ((int64_t)n * c >= kMaxElements || (int64_t)n * c * h >= kMaxElements || (int64_t)n * c * h * w >= kMaxElements)
        return fail(PPO_E_INVALID, "%s: a tensor of 2^30 elements or more", what);
    return PPO_OK;
}

}  // namespace
}  // namespace ppo

extern "C" int ppo_maxpool2x2_relu_forward_f32(const float *in, float *out, uint8_t *gate, int n, int c, int h, int w,
                                               void *stream)
{
    using namespace ppo;
    const char *what = "ppo_maxpool2x2_relu_forward_f32";
    if (int rc = check_shape(what, n, c, h, w)) return rc;
    if (in == nullptr || out == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    const int ho = h / 2, wo = w / 2;
    const int64_t n_windows = (int64_t)n * c * ho * wo;
    const dim3 grid((unsigned)((n_windows + kThreads - 1) / kThreads));
    if (w % 2 == 0 && aligned(in, 8))
        hipLaunchKernelGGL(maxpool2x2_relu_fwd_kernel<true>, grid, dim3(kThreads), 0, as_stream(stream), in, out, gate, h, w,
                           ho, wo, n_windows);
    else
        hipLaunchKernelGGL(maxpool2x2_relu_fwd_kernel<false>, grid, dim3(kThreads), 0, as_stream(stream), in, out, gate, h, w,
                           ho, wo, n_windows);
    return check_launch(what);
}

extern "C" int ppo_maxpool2x2_relu_backward_f32(const float *dout, const uint8_t *gate, float *din, int n, int c, int h, int w,
                                                void *stream)
{
    using namespace ppo;
    const char *what = "ppo_maxpool2x2_relu_backward_f32";
    if (int rc = check_shape(what, n, c, h, w)) return rc;
    if (dout == nullptr || gate == nullptr || din == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    const int ho = h / 2, wo = w / 2, hc = (h + 1) / 2, wc = (w + 1) / 2;
    const int64_t n_cells = (int64_t)n * c * hc * wc;
    const dim3 grid((unsigned)((n_cells + kThreads - 1) / kThreads));
    if (w % 2 == 0 && aligned(din, 8))
        hipLaunchKernelGGL(maxpool2x2_relu_bwd_kernel<true>, grid, dim3(kThreads), 0, as_stream(stream), dout, gate, din, h, w,
                           ho, wo, hc, wc, n_cells);
    else
        hipLaunchKernelGGL(maxpool2x2_relu_bwd_kernel<false>, grid, dim3(kThreads), 0, as_stream(stream), dout, gate, din, h, w,
                           ho, wo, hc, wc, n_cells);
    return check_launch(what);
}
