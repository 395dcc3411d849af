// Strided "valid" convolutions of any geometry as implicit GEMMs on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32):
// the layers of the reference's NatureCNN (rl/models.py:101-145: 8x8 stride 4, 4x4 stride 2, 3x3 stride 1, no
// padding), forward, backward-data and backward-weight.  One kernel, three operand descriptions (csrc/
// conv_strided_index.h holds the offset arithmetic and the GEMM views).
//
// The tile loop (64 x 32 of C per workgroup, K through LDS 16 at a time, every access predicated on its own bounds, a
// blocked fixed-order sum over K: no atomics, the same bits on every launch) is csrc/conv_gemm_tile.h, shared with the
// 3x3 / padding 1 family of conv3x3_any.hip.
#include "common.h"
#include "conv_gemm_tile.h"
#include "conv_stage.h"
#include "conv_strided_index.h"
#include "mfma.h"

namespace ppo {
namespace {

using tile::conv_gemm_kernel;
using tile::gemm_grid;
using tile::kMaxSlabs;
using tile::kThreads;
using tile::kTK;

__device__ __forceinline__ float load_in(const void *in, int in_mode, long long off)
{
    return in_mode == PPO_IN_U8 ? u8_unit((float)static_cast<const uint8_t *>(in)[off])
                                : static_cast<const float *>(in)[off];
}
__device__ __forceinline__ float load_gated(const float *dy, const float *gate, long long off)
{
    const float v = dy[off];
    return (gate == nullptr || gate[off] > 0.0f) ? v : 0.0f;  // the reference's ReLU has derivative 0 at 0
}

// The activation behind a convolution, as a type the Op structs take: what a forward store applies and how a backward
// load scales dy by the stored activation (the gate).  Relu keeps the arithmetic the three original entry points had.
struct Relu {
    __device__ float act(float v) const { return fmaxf(v, 0.0f); }
    __device__ float gated(const float *dy, const float *gate, long long off) const { return load_gated(dy, gate, off); }
};
// F.leaky_relu(., slope) (the RND networks, rl/models.py:250-252, 291-293).  slope > 0, so the stored activation has the
// sign of the pre-activation and serves as the gate; torch's leaky_relu backward takes the slope branch at 0.
struct Leaky {
    float slope;
    __device__ float act(float v) const { return v > 0.0f ? v : slope * v; }
    __device__ float gated(const float *dy, const float *gate, long long off) const
    {
        const float v = dy[off];
        return (gate == nullptr || gate[off] > 0.0f) ? v : slope * v;
    }
};

// out[m, co] = sum_k im2col(in)[m, k] * weight[co, k] + bias[co]
template <class Act>
struct ForwardOp {
    csi::Geom g;
    Act act;
    const void *in;
    int in_mode;
    const float *weight, *bias;
    float *out;
    int relu_out;
    int M, N, K;
    struct KCtx {
        long long a_off;
        int k;
    };
    typedef long long ARow;
    typedef long long BCol;
    __device__ void k_range(int, int &kb, int &ke) const { kb = 0, ke = K; }
    __device__ ARow a_row(int m) const { return csi::in_row_base(g, m); }
    __device__ BCol b_col(int n) const { return csi::weight_off(g, n, 0); }
    __device__ KCtx k_ctx(int k) const { return KCtx{csi::in_col_off(g, k), k}; }
    __device__ float load_a(ARow r, const KCtx &kc) const { return load_in(in, in_mode, r + kc.a_off); }
    __device__ float load_b(BCol c, const KCtx &kc) const { return weight[c + kc.k]; }
    __device__ void store(int m, int n, float v, int) const
    {
        if (bias != nullptr) v += bias[n];
        if (relu_out) v = act.act(v);
        out[csi::out_row_base(g, m) + csi::out_col_off(g, n)] = v;
    }
};

// dx[m, ci] = sum_{k = (co, ky, kx)} [tap k reaches m] (gate > 0 ? dy : 0)[img, co, oy, ox] * weight[co, ci, ky, kx]
template <class Act>
struct BackwardDataOp {
    csi::Geom g;
    Act act;
    const float *dy, *gate, *weight;
    float *dx;
    int M, N, K;
    typedef csi::DxTap KCtx;
    typedef csi::DxRow ARow;
    typedef long long BCol;
    __device__ void k_range(int, int &kb, int &ke) const { kb = 0, ke = K; }
    __device__ ARow a_row(int m) const { return csi::dx_row(g, m); }
    __device__ BCol b_col(int n) const { return csi::dx_weight_col_off(g, n); }
    __device__ KCtx k_ctx(int k) const { return csi::dx_tap(g, k); }
    __device__ float load_a(const ARow &r, const KCtx &t) const
    {
        long long off;
        return csi::dx_tap_hits(g, r, t, &off) ? act.gated(dy, gate, off) : 0.0f;
    }
    __device__ float load_b(BCol c, const KCtx &t) const { return weight[t.w_base + c]; }
    __device__ void store(int m, int n, float v, int) const
    {
        const int img = m / (g.h * g.w), pix = m % (g.h * g.w);
        dx[(long long)img * g.cin * g.h * g.w + pix + csi::dx_col_off(g, n)] = v;
    }
};

// slab z: ws[z, co, kf] = sum_{m in slab z} (gate > 0 ? dy : 0)[m, co] * im2col(in)[m, kf];  kf == K_fwd: the row of
// ones, i.e. the slab's share of dbias
template <class Act>
struct BackwardWeightOp {
    csi::Geom g;
    Act act;
    const void *in;
    int in_mode;
    const float *dy, *gate;
    float *ws;
    int rows;      // per slab
    int M_fwd;     // reduction length
    int M, N;      // K_fwd + 1, cout
    struct KCtx {
        long long in_base, out_base;
    };
    typedef long long ARow;  // < 0: the row of ones
    typedef long long BCol;
    __device__ void k_range(int z, int &kb, int &ke) const { kb = csi::slab_begin(z, rows), ke = csi::slab_end(M_fwd, z, rows); }
    __device__ ARow a_row(int m) const { return m < M - 1 ? csi::in_col_off(g, m) : -1; }
    __device__ BCol b_col(int n) const { return csi::out_col_off(g, n); }
    __device__ KCtx k_ctx(int k) const { return KCtx{csi::in_row_base(g, k), csi::out_row_base(g, k)}; }
    __device__ float load_a(ARow r, const KCtx &kc) const { return r < 0 ? 1.0f : load_in(in, in_mode, kc.in_base + r); }
    __device__ float load_b(BCol c, const KCtx &kc) const { return act.gated(dy, gate, kc.out_base + c); }
    __device__ void store(int m, int n, float v, int z) const { ws[csi::slab_off(g, z, n, m)] = v; }
};

// dweight[co, k] = sum_s ws[s, co, k] (k < K), dbias[co] = sum_s ws[s, co, K], slabs in ascending order
__global__ __launch_bounds__(256) void strided_wgrad_reduce_kernel(const float *__restrict__ ws, float *__restrict__ dweight,
                                                                   float *__restrict__ dbias, int n_slabs, int cout, int K)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per_slab = (long long)cout * (K + 1);
    if (i >= per_slab) return;
    float sum = 0.0f;
    for (int s = 0; s < n_slabs; ++s) sum += ws[s * per_slab + i];
    const int co = (int)(i / (K + 1)), k = (int)(i % (K + 1));
    if (k < K)
        dweight[(long long)co * K + k] = sum;
    else if (dbias != nullptr)
        dbias[co] = sum;
}

int check_geometry(const char *what, int n, int cin, int h, int w, int cout, int kh, int kw, int stride, csi::Geom *g)
{
    if (!csi::geometry_ok(cin, cout, kh, kw, stride, h, w))
        return fail(PPO_E_INVALID, "%s: unsupported geometry cin=%d cout=%d k=%dx%d stride=%d on %dx%d", what, cin, cout, kh,
                    kw, stride, h, w);
    *g = csi::make_geom(n, cin, h, w, cout, kh, kw, stride);
    if (!csi::sizes_ok(*g)) return fail(PPO_E_INVALID, "%s: n=%d is not positive or a tensor exceeds 2^30 elements", what, n);
    return PPO_OK;
}

int wgrad_slabs(const csi::Geom &g, int *rows)
{
    *rows = csi::slab_rows(csi::fwd_m(g), kMaxSlabs, kTK);
    return csi::slab_count(csi::fwd_m(g), *rows);
}

}  // namespace
}  // namespace ppo

using namespace ppo;

extern "C" int ppo_conv2d_strided_supported(int cin, int cout, int kh, int kw, int stride, int h, int w)
{
    return csi::geometry_ok(cin, cout, kh, kw, stride, h, w) ? 1 : 0;
}

namespace {

template <class Act>
int launch_forward(const char *what, Act act, const void *in, int in_mode, const float *weight, const float *bias, float *out,
                   int act_out, int n, int cin, int h, int w, int cout, int kh, int kw, int stride, void *stream)
{
    csi::Geom g;
    if (int rc = check_geometry(what, n, cin, h, w, cout, kh, kw, stride, &g)) return rc;
    if (in == nullptr || weight == nullptr || out == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    if (in_mode != PPO_IN_NONE && in_mode != PPO_IN_U8)
        return fail(PPO_E_INVALID, "%s: in_mode %d (PPO_IN_NONE | PPO_IN_U8)", what, in_mode);
    ForwardOp<Act> op{g, act, in, in_mode, weight, bias, out, act_out ? 1 : 0, csi::fwd_m(g), cout, csi::fwd_k(g)};
    hipLaunchKernelGGL(conv_gemm_kernel<ForwardOp<Act>>, gemm_grid(op.M, op.N, 1), dim3(kThreads), 0, as_stream(stream), op);
    return check_launch(what);
}

template <class Act>
int launch_backward_data(const char *what, Act act, const float *dy, const float *gate, const float *weight, float *dx, int n,
                         int cin, int h, int w, int cout, int kh, int kw, int stride, void *stream)
{
    csi::Geom g;
    if (int rc = check_geometry(what, n, cin, h, w, cout, kh, kw, stride, &g)) return rc;
    if (dy == nullptr || weight == nullptr || dx == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    BackwardDataOp<Act> op{g, act, dy, gate, weight, dx, csi::dx_m(g), cin, csi::dx_k(g)};
    hipLaunchKernelGGL(conv_gemm_kernel<BackwardDataOp<Act>>, gemm_grid(op.M, op.N, 1), dim3(kThreads), 0, as_stream(stream),
                       op);
    return check_launch(what);
}

template <class Act>
int launch_backward_weight(const char *what, Act act, const void *in, int in_mode, const float *dy, const float *gate,
                           float *dweight, float *dbias, void *workspace, size_t workspace_bytes, int n, int cin, int h, int w,
                           int cout, int kh, int kw, int stride, void *stream)
{
    csi::Geom g;
    if (int rc = check_geometry(what, n, cin, h, w, cout, kh, kw, stride, &g)) return rc;
    if (in == nullptr || dy == nullptr || dweight == nullptr || workspace == nullptr)
        return fail(PPO_E_INVALID, "%s: null pointer", what);
    if (in_mode != PPO_IN_NONE && in_mode != PPO_IN_U8)
        return fail(PPO_E_INVALID, "%s: in_mode %d (PPO_IN_NONE | PPO_IN_U8)", what, in_mode);
    int rows;
    const int slabs = wgrad_slabs(g, &rows);
    const int K = csi::fwd_k(g);
    const size_t need = (size_t)slabs * cout * (K + 1) * sizeof(float);
    if (workspace_bytes < need) return fail(PPO_E_INVALID, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
    if (!aligned(workspace, 4)) return fail(PPO_E_ALIGN, "%s: workspace not 4-byte aligned", what);
    BackwardWeightOp<Act> op{g, act, in, in_mode, dy, gate, static_cast<float *>(workspace), rows, csi::fwd_m(g), K + 1, cout};
    hipLaunchKernelGGL(conv_gemm_kernel<BackwardWeightOp<Act>>, gemm_grid(op.M, op.N, slabs), dim3(kThreads), 0,
                       as_stream(stream), op);
    if (int rc = check_launch(what)) return rc;
    const long long per_slab = (long long)cout * (K + 1);
    hipLaunchKernelGGL(strided_wgrad_reduce_kernel, dim3((unsigned)((per_slab + 255) / 256)), dim3(256), 0, as_stream(stream),
                       static_cast<const float *>(workspace), dweight, dbias, slabs, cout, K);
    return check_launch(what);
}

bool slope_ok(const char *what, float slope)
{
    if (slope > 0.0f && slope <= 1.0f) return true;
    fail(PPO_E_INVALID, "%s: negative_slope %g outside (0, 1]", what, (double)slope);
    return false;
}

}  // namespace

extern "C" int ppo_conv2d_strided_forward_f32(const void *in, int in_mode, const float *weight, const float *bias, float *out,
                                              int relu_out, int n, int cin, int h, int w, int cout, int kh, int kw, int stride,
                                              void *stream)
{
    return launch_forward("ppo_conv2d_strided_forward_f32", Relu{}, in, in_mode, weight, bias, out, relu_out, n, cin, h, w, cout,
                          kh, kw, stride, stream);
}

extern "C" int ppo_conv2d_strided_backward_data_f32(const float *dy, const float *gate, const float *weight, float *dx, int n,
                                                    int cin, int h, int w, int cout, int kh, int kw, int stride, void *stream)
{
    return launch_backward_data("ppo_conv2d_strided_backward_data_f32", Relu{}, dy, gate, weight, dx, n, cin, h, w, cout, kh, kw,
                                stride, stream);
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
    return launch_backward_weight("ppo_conv2d_strided_backward_weight_f32", Relu{}, in, in_mode, dy, gate, dweight, dbias,
                                  workspace, workspace_bytes, n, cin, h, w, cout, kh, kw, stride, stream);
}

// The same three launches with F.leaky_relu(., negative_slope) behind the convolution instead of F.relu: the layers of
// the reference's RNDTarget / RNDPredictor (rl/models.py:228-230, 250-252, 270-272, 291-293).
extern "C" int ppo_conv2d_strided_forward_leaky_f32(const void *in, int in_mode, const float *weight, const float *bias,
                                                    float *out, float negative_slope, int n, int cin, int h, int w, int cout,
                                                    int kh, int kw, int stride, void *stream)
{
    const char *what = "ppo_conv2d_strided_forward_leaky_f32";
    if (!slope_ok(what, negative_slope)) return PPO_E_INVALID;
    return launch_forward(what, Leaky{negative_slope}, in, in_mode, weight, bias, out, 1, n, cin, h, w, cout, kh, kw, stride,
                          stream);
}

extern "C" int ppo_conv2d_strided_backward_data_leaky_f32(const float *dy, const float *gate, const float *weight, float *dx,
                                                          float negative_slope, int n, int cin, int h, int w, int cout, int kh,
                                                          int kw, int stride, void *stream)
{
    const char *what = "ppo_conv2d_strided_backward_data_leaky_f32";
    if (!slope_ok(what, negative_slope)) return PPO_E_INVALID;
    return launch_backward_data(what, Leaky{negative_slope}, dy, gate, weight, dx, n, cin, h, w, cout, kh, kw, stride, stream);
}

extern "C" int ppo_conv2d_strided_backward_weight_leaky_f32(const void *in, int in_mode, const float *dy, const float *gate,
                                                            float *dweight, float *dbias, void *workspace,
                                                            size_t workspace_bytes, float negative_slope, int n, int cin, int h,
                                                            int w, int cout, int kh, int kw, int stride, void *stream)
{
    const char *what = "ppo_conv2d_strided_backward_weight_leaky_f32";
    if (!slope_ok(what, negative_slope)) return PPO_E_INVALID;
    return launch_backward_weight(what, Leaky{negative_slope}, in, in_mode, dy, gate, dweight, dbias, workspace, workspace_bytes,
                                  n, cin, h, w, cout, kh, kw, stride, stream);
}
