// Strided "valid" convolutions of any geometry as implicit GEMMs on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32):
// the layers of the reference's NatureCNN (rl/models.py:101-145: 8x8 stride 4, 4x4 stride 2, 3x3 stride 1, no
// padding), forward, backward-data and backward-weight.  One kernel, three operand descriptions (csrc/
// conv_strided_index.h holds the offset arithmetic and the GEMM views).
//
// The tile loop (64 x 32 of C per workgroup, K through LDS 16 at a time, every access predicated on its own bounds, a
// blocked fixed-order sum over K: no atomics, the same bits on every launch) is csrc/conv_gemm_tile.h, shared with the
// 3x3 / padding 1 family of conv3x3_any.hip; the operand descriptions, the validation and the launchers are csrc/
// conv_strided_ops.h, shared with the split-bf16 entry points of conv_strided_bf16x3.hip.
#include "conv_strided_ops.h"

namespace ppo {
namespace {

struct ExactLoop {
    template <class Op>
    static void launch(const Op &op, dim3 grid, hipStream_t stream)
    {
        hipLaunchKernelGGL(tile::conv_gemm_kernel<Op>, grid, dim3(tile::kThreads), 0, stream, op);
    }
};

bool slope_ok(const char *what, float slope)
{
    if (slope > 0.0f && slope <= 1.0f) return true;
    fail(PPO_E_INVALID, "%s: negative_slope %g outside (0, 1]", what, (double)slope);
    return false;
}

}  // namespace
}  // namespace ppo

using namespace ppo;

extern "C" int ppo_conv2d_strided_supported(int cin, int cout, int kh, int kw, int stride, int h, int w)
{
    return csi::geometry_ok(cin, cout, kh, kw, stride, h, w) ? 1 : 0;
}

extern "C" int ppo_conv2d_strided_forward_f32(const void *in, int in_mode, const float *weight, const float *bias, float *out,
                                              int relu_out, int n, int cin, int h, int w, int cout, int kh, int kw, int stride,
                                              void *stream)
{
    return launch_forward<ExactLoop>("ppo_conv2d_strided_forward_f32", Relu{}, in, in_mode, weight, bias, out, relu_out, n,
                                     cin, h, w, cout, kh, kw, stride, stream);
}

extern "C" int ppo_conv2d_strided_backward_data_f32(const float *dy, const float *gate, const float *weight, float *dx, int n,
                                                    int cin, int h, int w, int cout, int kh, int kw, int stride, void *stream)
{
    return launch_backward_data<ExactLoop>("ppo_conv2d_strided_backward_data_f32", Relu{}, dy, gate, weight, dx, n, cin, h, w,
                                           cout, kh, kw, stride, stream);
}

extern "C" size_t ppo_conv2d_strided_wgrad_workspace_bytes(int n, int cin, int h, int w, int cout, int kh, int kw, int stride)
{
    if (!csi::geometry_ok(cin, cout, kh, kw, stride, h, w)) return 0;
    const csi::Geom g = csi::make_geom(n, cin, h, w, cout, kh, kw, stride);
    if (!csi::sizes_ok(g)) return 0;
    int rows;
    const int slabs = wgrad_slabs(g, &rows);
    return (size_t)slabs * cout * (csi::fwd_k(g) + 1) * sizeof(float);
}

extern "C" int ppo_conv2d_strided_backward_weight_f32(const void *in, int in_mode, const float *dy, const float *gate,
                                                      float *dweight, float *dbias, void *workspace, size_t workspace_bytes,
                                                      int n, int cin, int h, int w, int cout, int kh, int kw, int stride,
                                                      void *stream)
{
    return launch_backward_weight<ExactLoop>("ppo_conv2d_strided_backward_weight_f32", Relu{}, in, in_mode, dy, gate, dweight,
                                             dbias, workspace, workspace_bytes, n, cin, h, w, cout, kh, kw, stride, stream);
}

// The same three launches with F.leaky_relu(., negative_slope) behind the convolution instead of F.relu: the layers of
// the reference's RNDTarget / RNDPredictor (rl/models.py:228-230, 250-252, 270-272, 291-293).
extern "C" int ppo_conv2d_strided_forward_leaky_f32(const void *in, int in_mode, const float *weight, const float *bias,
                                                    float *out, float negative_slope, int n, int cin, int h, int w, int cout,
                                                    int kh, int kw, int stride, void *stream)
{
    const char *what = "ppo_conv2d_strided_forward_leaky_f32";
    if (!slope_ok(what, negative_slope)) return PPO_E_INVALID;
    return launch_forward<ExactLoop>(what, Leaky{negative_slope}, in, in_mode, weight, bias, out, 1, n, cin, h, w, cout, kh,
                                     kw, stride, stream);
}

extern "C" int ppo_conv2d_strided_backward_data_leaky_f32(const float *dy, const float *gate, const float *weight, float *dx,
                                                          float negative_slope, int n, int cin, int h, int w, int cout, int kh,
                                                          int kw, int stride, void *stream)
{
    const char *what = "ppo_conv2d_strided_backward_data_leaky_f32";
    if (!slope_ok(what, negative_slope)) return PPO_E_INVALID;
    return launch_backward_data<ExactLoop>(what, Leaky{negative_slope}, dy, gate, weight, dx, n, cin, h, w, cout, kh, kw,
                                           stride, stream);
}

extern "C" int ppo_conv2d_strided_backward_weight_leaky_f32(const void *in, int in_mode, const float *dy, const float *gate,
                                                            float *dweight, float *dbias, void *workspace,
                                                            size_t workspace_bytes, float negative_slope, int n, int cin, int h,
                                                            int w, int cout, int kh, int kw, int stride, void *stream)
{
    const char *what = "ppo_conv2d_strided_backward_weight_leaky_f32";
    if (!slope_ok(what, negative_slope)) return PPO_E_INVALID;
    return launch_backward_weight<ExactLoop>(what, Leaky{negative_slope}, in, in_mode, dy, gate, dweight, dbias, workspace,
                                             workspace_bytes, n, cin, h, w, cout, kh, kw, stride, stream);
}
