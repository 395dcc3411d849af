// OPT-IN reduced-precision form of the strided "valid" convolutions of conv_strided.hip (the layers of the reference's
// NatureCNN, rl/models.py:101-145): every product as three bf16 MFMAs on (hi, lo) splits of both operands, float32
// accumulation - ~16-bit products, more than the TF32 (10-bit) products the reference's default `--precision=medium`
// lets cuDNN use on its own GPUs (the reference's train.py:166-178).
//
// The tile loop is csrc/conv_gemm_tile_bf16x3.h; the operand descriptions, the validation (codes and messages), the
// slab partition and the float32 ascending-order slab reduction are those of the exact entry points, from csrc/
// conv_strided_ops.h.  Nothing is packed ahead of a launch: the operands are the float32 (or uint8) tensors themselves.
#include "conv_gemm_tile_bf16x3.h"
#include "conv_strided_ops.h"

namespace ppo {
namespace {

struct SplitLoop {
    template <class Op>
    static void launch(const Op &op, dim3 grid, hipStream_t stream)
    {
        hipLaunchKernelGGL(tile::conv_gemm_bf16x3_kernel<Op>, grid, dim3(tile::kThreads), 0, stream, op);
    }
};

}  // namespace
}  // namespace ppo

using namespace ppo;

extern "C" int ppo_conv2d_strided_forward_bf16x3(const void *in, int in_mode, const float *weight, const float *bias,
                                                 float *out, int relu_out, int n, int cin, int h, int w, int cout, int kh,
                                                 int kw, int stride, void *stream)
{
    return launch_forward<SplitLoop>("ppo_conv2d_strided_forward_bf16x3", Relu{}, in, in_mode, weight, bias, out, relu_out, n,
                                     cin, h, w, cout, kh, kw, stride, stream);
}

extern "C" int ppo_conv2d_strided_backward_data_bf16x3(const float *dy, const float *gate, const float *weight, float *dx,
                                                       int n, int cin, int h, int w, int cout, int kh, int kw, int stride,
                                                       void *stream)
{
    return launch_backward_data<SplitLoop>("ppo_conv2d_strided_backward_data_bf16x3", Relu{}, dy, gate, weight, dx, n, cin, h,
                                           w, cout, kh, kw, stride, stream);
}

extern "C" int ppo_conv2d_strided_backward_weight_bf16x3(const void *in, int in_mode, const float *dy, const float *gate,
                                                         float *dweight, float *dbias, void *workspace,
                                                         size_t workspace_bytes, int n, int cin, int h, int w, int cout, int kh,
                                                         int kw, int stride, void *stream)
{
    return launch_backward_weight<SplitLoop>("ppo_conv2d_strided_backward_weight_bf16x3", Relu{}, in, in_mode, dy, gate,
                                             dweight, dbias, workspace, workspace_bytes, n, cin, h, w, cout, kh, kw, stride,
                                             stream);
}
