// The operand descriptions (`Op`, see csrc/conv_gemm_tile.h) of the strided "valid" convolutions, their slab
// reduction, argument validation and launchers, shared by the exact-f32 entry points (conv_strided.hip) and the
// split-bf16 ones (conv_strided_bf16x3.hip).  A launcher takes the tile loop as a type `Loop` with
//     template <class Op> static void launch(const Op &op, dim3 grid, hipStream_t stream);
// so both precisions run the same index arithmetic, the same checks in the same order and the same messages.
#pragma once
#include "common.h"
#include "conv_gemm_tile.h"
#include "conv_stage.h"
#include "conv_strided_index.h"

namespace ppo {
namespace {

using tile::gemm_grid;
using tile::kMaxSlabs;
using tile::kTK;

__device__ __forceinline__ float load_in(const void *in, int in_mode, long long off)
{
    return in_mode_is_u8(in_mode) ? u8_prep((float)static_cast<const uint8_t *>(in)[off], in_mode)
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

// The slab partition of a weight gradient's reduction: one for both tile loops, so
// ppo_conv2d_strided_wgrad_workspace_bytes serves both precisions.
int wgrad_slabs(const csi::Geom &g, int *rows)
{
    *rows = csi::slab_rows(csi::fwd_m(g), kMaxSlabs, kTK);
    return csi::slab_count(csi::fwd_m(g), *rows);
}

template <class Loop, class Act>
int launch_forward(const char *what, Act act, const void *in, int in_mode, const float *weight, const float *bias, float *out,
                   int act_out, int n, int cin, int h, int w, int cout, int kh, int kw, int stride, void *stream)
{
    csi::Geom g;
    if (int rc = check_geometry(what, n, cin, h, w, cout, kh, kw, stride, &g)) return rc;
    if (in == nullptr || weight == nullptr || out == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    if (in_mode != PPO_IN_NONE && !in_mode_is_u8(in_mode))
        return fail(PPO_E_INVALID, "%s: in_mode %d (PPO_IN_NONE | PPO_IN_U8 | PPO_IN_U8_CENTERED | PPO_IN_U8_UNIT)", what, in_mode);
    ForwardOp<Act> op{g, act, in, in_mode, weight, bias, out, act_out ? 1 : 0, csi::fwd_m(g), cout, csi::fwd_k(g)};
    Loop::launch(op, gemm_grid(op.M, op.N, 1), as_stream(stream));
    return check_launch(what);
}

template <class Loop, class Act>
int launch_backward_data(const char *what, Act act, const float *dy, const float *gate, const float *weight, float *dx, int n,
                         int cin, int h, int w, int cout, int kh, int kw, int stride, void *stream)
{
    csi::Geom g;
    if (int rc = check_geometry(what, n, cin, h, w, cout, kh, kw, stride, &g)) return rc;
    if (dy == nullptr || weight == nullptr || dx == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    BackwardDataOp<Act> op{g, act, dy, gate, weight, dx, csi::dx_m(g), cin, csi::dx_k(g)};
    Loop::launch(op, gemm_grid(op.M, op.N, 1), as_stream(stream));
    return check_launch(what);
}

template <class Loop, class Act>
int launch_backward_weight(const char *what, Act act, const void *in, int in_mode, const float *dy, const float *gate,
                           float *dweight, float *dbias, void *workspace, size_t workspace_bytes, int n, int cin, int h, int w,
                           int cout, int kh, int kw, int stride, void *stream)
{
    csi::Geom g;
    if (int rc = check_geometry(what, n, cin, h, w, cout, kh, kw, stride, &g)) return rc;
    if (in == nullptr || dy == nullptr || dweight == nullptr || workspace == nullptr)
        return fail(PPO_E_INVALID, "%s: null pointer", what);
    if (in_mode != PPO_IN_NONE && !in_mode_is_u8(in_mode))
        return fail(PPO_E_INVALID, "%s: in_mode %d (PPO_IN_NONE | PPO_IN_U8 | PPO_IN_U8_CENTERED | PPO_IN_U8_UNIT)", what, in_mode);
    int rows;
    const int slabs = wgrad_slabs(g, &rows);
    const int K = csi::fwd_k(g);
    const size_t need = (size_t)slabs * cout * (K + 1) * sizeof(float);
    if (workspace_bytes < need) return fail(PPO_E_INVALID, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
    if (!aligned(workspace, 4)) return fail(PPO_E_ALIGN, "%s: workspace not 4-byte aligned", what);
    BackwardWeightOp<Act> op{g, act, in, in_mode, dy, gate, static_cast<float *>(workspace), rows, csi::fwd_m(g), K + 1, cout};
    Loop::launch(op, gemm_grid(op.M, op.N, slabs), as_stream(stream));
    if (int rc = check_launch(what)) return rc;
    const long long per_slab = (long long)cout * (K + 1);
    hipLaunchKernelGGL(strided_wgrad_reduce_kernel, dim3((unsigned)((per_slab + 255) / 256)), dim3(256), 0, as_stream(stream),
                       static_cast<const float *>(workspace), dweight, dbias, slabs, cout, K);
    return check_launch(what);
}

}  // namespace
}  // namespace ppo
