// 3x3 / stride 1 / zero-padding 1 convolutions of ANY geometry as implicit GEMMs on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32): the convolutions of the reference's IMPALA encoder (rl/impala.py:61-62, 96) at the
// observation shapes, channel lists and block counts the specialised kernels of conv3x3.hip / conv3x3_wgrad.hip have
// no instantiation for - forward, backward-data and backward-weight-plus-bias, with the load transforms, residual,
// ReLU gate and skip-gradient operands of those entry points, so a caller swaps them call for call.
//
// One tile loop (csrc/conv_gemm_tile.h, shared with conv_strided.hip), three operand descriptions;
// csrc/conv3x3_any_index.h holds the offset arithmetic and the GEMM views.  Padding taps are zeros by predicate, every
// global access is predicated on its own bounds, sums over K are blocked and in a fixed order: no atomics, the same
// bits on every launch.  Untuned: the specialised kernels stay the fast path wherever they exist.
//
// The same three passes at stride 2 (ppo_conv3x3s2_any_*, csrc/conv3x3s2_any_index.h): the stack-first convolution of
// the reference's down_sample='stride' encoder (rl/impala.py:96), three more operand descriptions on the same tile loop
// and the same slab reduction.
#include "common.h"
#include "conv3x3_any_index.h"
#include "conv3x3s2_any_index.h"
#include "conv_gemm_tile.h"
#include "conv_stage.h"
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
    if (in_mode_is_u8(in_mode)) return u8_prep((float)static_cast<const uint8_t *>(in)[off], in_mode);
    const float v = static_cast<const float *>(in)[off];
    return in_mode == IN_RELU ? fmaxf(v, 0.0f) : v;
}

// out[m, co] = bias[co] + sum_k f(in)[m + tap k] * weight[co, k] (+ residual[m, co])
struct ForwardOp {
    c3i::Geom g;
    const void *in;
    int in_mode;
    const float *weight, *bias, *residual;
    float *out;
    int M, N, K;
    typedef c3i::Pix ARow;
    typedef long long BCol;
    typedef c3i::Tap KCtx;
    __device__ void k_range(int, int &kb, int &ke) const { kb = 0, ke = K; }
    __device__ ARow a_row(int m) const { return c3i::pix(g, m, g.cin); }
    __device__ BCol b_col(int n) const { return c3i::fwd_weight_col(g, n); }
    __device__ KCtx k_ctx(int k) const { return c3i::fwd_tap(g, k); }
    __device__ float load_a(const ARow &p, const KCtx &t) const
    {
        long long off;
        return c3i::tap_hits(g, p, t, &off) ? load_in(in, in_mode, off) : 0.0f;
    }
    __device__ float load_b(BCol c, const KCtx &t) const { return weight[c + t.w_off]; }
    __device__ void store(int m, int n, float v, int) const
    {
        const c3i::Pix p = c3i::pix(g, m, g.cout);
        const long long off = p.base + c3i::chan_off(g, n) + p.plane;
        if (bias != nullptr) v += bias[n];
        if (residual != nullptr) v += residual[off];
        out[off] = v;
    }
};

// dx[m, ci] = (sum_{k = (co, ky, kx)} dy[m - tap k] * weight[co, ci, ky, kx]) * [relu_src[m, ci] > 0] + dres[m, ci]
struct BackwardDataOp {
    c3i::Geom g;
    const float *dy, *weight, *relu_src, *dres;
    float *dx;
    int M, N, K;
    typedef c3i::Pix ARow;
    typedef long long BCol;
    typedef c3i::Tap KCtx;
    __device__ void k_range(int, int &kb, int &ke) const { kb = 0, ke = K; }
    __device__ ARow a_row(int m) const { return c3i::pix(g, m, g.cout); }
    __device__ BCol b_col(int n) const { return c3i::dx_weight_col(g, n); }
    __device__ KCtx k_ctx(int k) const { return c3i::dx_tap(g, k); }
    __device__ float load_a(const ARow &p, const KCtx &t) const
    {
        long long off;
        return c3i::tap_hits(g, p, t, &off) ? dy[off] : 0.0f;
    }
    __device__ float load_b(BCol c, const KCtx &t) const { return weight[t.w_off + c]; }
    __device__ void store(int m, int n, float v, int) const
    {
        const c3i::Pix p = c3i::pix(g, m, g.cin);
        const long long off = p.base + c3i::chan_off(g, n) + p.plane;
        if (relu_src != nullptr && !(relu_src[off] > 0.0f)) v = 0.0f;  // the reference's ReLU has derivative 0 at 0
        if (dres != nullptr) v += dres[off];
        dx[off] = v;
    }
};

// slab z: ws[z, co, k] = sum_{m in slab z} dy[m, co] * f(in)[m + tap k];  k == 9 cin: the row of ones, i.e. the slab's
// share of dbias
struct BackwardWeightOp {
    c3i::Geom g;
    const void *in;
    int in_mode;
    const float *dy;
    float *ws;
    int rows;    // per slab
    int pixels;  // reduction length
    int M, N;    // 9 cin + 1, cout
    struct KCtx {
        c3i::Pix p;        // in the input
        long long dy_off;  // + chan_off(co)
    };
    typedef c3i::Tap ARow;  // c < 0: the row of ones
    typedef long long BCol;
    __device__ void k_range(int z, int &kb, int &ke) const { kb = c3i::slab_begin(z, rows), ke = c3i::slab_end(pixels, z, rows); }
    __device__ ARow a_row(int m) const
    {
        if (m < M - 1) return c3i::fwd_tap(g, m);
        return ARow{0, -1, 0, 0};
    }
    __device__ BCol b_col(int n) const { return c3i::chan_off(g, n); }
    __device__ KCtx k_ctx(int k) const
    {
        const c3i::Pix q = c3i::pix(g, k, g.cout);
        return KCtx{c3i::pix(g, k, g.cin), q.base + q.plane};
    }
    __device__ float load_a(const ARow &t, const KCtx &kc) const
    {
        if (t.c < 0) return 1.0f;
        long long off;
        return c3i::tap_hits(g, kc.p, t, &off) ? load_in(in, in_mode, off) : 0.0f;
    }
    __device__ float load_b(BCol c, const KCtx &kc) const { return dy[kc.dy_off + c]; }
    __device__ void store(int m, int n, float v, int z) const { ws[c3i::slab_off(g, z, n, m)] = v; }
};

// dweight[co, k] (+)= sum_s ws[s, co, k] (k < K), dbias[co] (+)= sum_s ws[s, co, K], slabs in ascending order
__global__ __launch_bounds__(256) void any_wgrad_reduce_kernel(const float *__restrict__ ws, float *__restrict__ dweight,
                                                               float *__restrict__ dbias, int n_slabs, int cout, int K,
                                                               int accumulate)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per_slab = (long long)cout * (K + 1);
    if (i >= per_slab) return;
    float sum = 0.0f;
    for (int s = 0; s < n_slabs; ++s) sum += ws[s * per_slab + i];
    const int co = (int)(i / (K + 1)), k = (int)(i % (K + 1));
    float *dst = k < K ? dweight + (long long)co * K + k : (dbias != nullptr ? dbias + co : nullptr);
    if (dst != nullptr) *dst = accumulate ? *dst + sum : sum;
}

int check_geometry(const char *what, int n, int cin, int cout, int h, int w, c3i::Geom *g)
{
    if (!c3i::geometry_ok(cin, cout, h, w))
        return fail(PPO_E_INVALID, "%s: unsupported geometry cin=%d cout=%d on %dx%d (each 1..4096)", what, cin, cout, h, w);
    *g = c3i::make_geom(n, cin, cout, h, w);
    if (!c3i::sizes_ok(*g)) return fail(PPO_E_INVALID, "%s: n=%d is not positive or a tensor exceeds 2^30 elements", what, n);
    return PPO_OK;
}

int wgrad_slabs(const c3i::Geom &g, int *rows)
{
    *rows = c3i::slab_rows(c3i::pix_m(g), kMaxSlabs, kTK);
    return c3i::slab_count(c3i::pix_m(g), *rows);
}

// ---- 3x3 / stride 2 / zero-padding 1 (csrc/conv3x3s2_any_index.h): the input is h x w, out / dy (h+1)/2 x (w+1)/2

// out[m, co] = bias[co] + sum_k f(in)[2 m + tap k - 1] * weight[co, k] (+ residual[m, co])
struct S2ForwardOp {
    c3s::Geom g;
    const void *in;
    int in_mode;
    const float *weight, *bias, *residual;
    float *out;
    int M, N, K;
    typedef c3s::OPix ARow;
    typedef long long BCol;
    typedef c3s::Tap KCtx;
    __device__ void k_range(int, int &kb, int &ke) const { kb = 0, ke = K; }
    __device__ ARow a_row(int m) const { return c3s::opix(g, m); }
    __device__ BCol b_col(int n) const { return c3s::fwd_weight_col(g, n); }
    __device__ KCtx k_ctx(int k) const { return c3s::fwd_tap(g, k); }
    __device__ float load_a(const ARow &p, const KCtx &t) const
    {
        long long off;
        return c3s::fwd_tap_hits(g, p, t, &off) ? load_in(in, in_mode, off) : 0.0f;
    }
    __device__ float load_b(BCol c, const KCtx &t) const { return weight[c + t.w_off]; }
    __device__ void store(int m, int n, float v, int) const
    {
        const c3s::OPix p = c3s::opix(g, m);
        const long long off = p.out_base + c3s::out_chan_off(g, n) + p.plane;
        if (bias != nullptr) v += bias[n];
        if (residual != nullptr) v += residual[off];
        out[off] = v;
    }
};

// dx[m, ci] = (sum over the taps k = (co, ky, kx) that reach input pixel m of dy[(m + 1 - tap k) / 2] *
// weight[co, ci, ky, kx]) * [relu_src[m, ci] > 0] + dres[m, ci]
struct S2BackwardDataOp {
    c3s::Geom g;
    const float *dy, *weight, *relu_src, *dres;
    float *dx;
    int M, N, K;
    typedef c3s::IPix ARow;
    typedef long long BCol;
    typedef c3s::Tap KCtx;
    __device__ void k_range(int, int &kb, int &ke) const { kb = 0, ke = K; }
    __device__ ARow a_row(int m) const { return c3s::ipix(g, m); }
    __device__ BCol b_col(int n) const { return c3s::dx_weight_col(g, n); }
    __device__ KCtx k_ctx(int k) const { return c3s::dx_tap(g, k); }
    __device__ float load_a(const ARow &p, const KCtx &t) const
    {
        long long off;
        return c3s::dx_tap_hits(g, p, t, &off) ? dy[off] : 0.0f;
    }
    __device__ float load_b(BCol c, const KCtx &t) const { return weight[t.w_off + c]; }
    __device__ void store(int m, int n, float v, int) const
    {
        const c3s::IPix p = c3s::ipix(g, m);
        const long long off = p.dx_base + c3s::in_chan_off(g, n) + p.plane;
        if (relu_src != nullptr && !(relu_src[off] > 0.0f)) v = 0.0f;  // the reference's ReLU has derivative 0 at 0
        if (dres != nullptr) v += dres[off];
        dx[off] = v;
    }
};

// slab z: ws[z, co, k] = sum_{m in slab z} dy[m, co] * f(in)[2 m + tap k - 1];  k == 9 cin: the row of ones, i.e. the
// slab's share of dbias
struct S2BackwardWeightOp {
    c3s::Geom g;
    const void *in;
    int in_mode;
    const float *dy;
    float *ws;
    int rows;    // per slab
    int pixels;  // reduction length
    int M, N;    // 9 cin + 1, cout
    struct KCtx {
        c3s::OPix p;
        long long dy_off;  // + out_chan_off(co)
    };
    typedef c3s::Tap ARow;  // c < 0: the row of ones
    typedef long long BCol;
    __device__ void k_range(int z, int &kb, int &ke) const { kb = c3s::slab_begin(z, rows), ke = c3s::slab_end(pixels, z, rows); }
    __device__ ARow a_row(int m) const
    {
        if (m < M - 1) return c3s::fwd_tap(g, m);
        return ARow{0, -1, 0, 0};
    }
    __device__ BCol b_col(int n) const { return c3s::out_chan_off(g, n); }
    __device__ KCtx k_ctx(int k) const
    {
        const c3s::OPix p = c3s::opix(g, k);
        return KCtx{p, p.out_base + p.plane};
    }
    __device__ float load_a(const ARow &t, const KCtx &kc) const
    {
        if (t.c < 0) return 1.0f;
        long long off;
        return c3s::fwd_tap_hits(g, kc.p, t, &off) ? load_in(in, in_mode, off) : 0.0f;
    }
    __device__ float load_b(BCol c, const KCtx &kc) const { return dy[kc.dy_off + c]; }
    __device__ void store(int m, int n, float v, int z) const { ws[c3s::slab_off(g, z, n, m)] = v; }
};

int check_geometry_s2(const char *what, int n, int cin, int cout, int h, int w, c3s::Geom *g)
{
    if (!c3s::geometry_ok(cin, cout, h, w))
        return fail(PPO_E_INVALID, "%s: unsupported geometry cin=%d cout=%d on %dx%d (each 1..4096)", what, cin, cout, h, w);
    *g = c3s::make_geom(n, cin, cout, h, w);
    if (!c3s::sizes_ok(*g)) return fail(PPO_E_INVALID, "%s: n=%d is not positive or a tensor exceeds 2^30 elements", what, n);
    return PPO_OK;
}

int wgrad_slabs_s2(const c3s::Geom &g, int *rows)
{
    *rows = c3s::slab_rows(c3s::fwd_m(g), kMaxSlabs, kTK);
    return c3s::slab_count(c3s::fwd_m(g), *rows);
}

}  // namespace
}  // namespace ppo

using namespace ppo;

extern "C" int ppo_conv3x3_any_supported(int cin, int cout, int h, int w) { return c3i::geometry_ok(cin, cout, h, w) ? 1 : 0; }

extern "C" int ppo_conv3x3_any_forward_f32(const void *in, int in_mode, const float *weight, const float *bias,
                                           const float *residual, float *out, int n, int cin, int cout, int h, int w,
                                           void *stream)
{
    const char *what = "ppo_conv3x3_any_forward_f32";
    c3i::Geom g;
    if (int rc = check_geometry(what, n, cin, cout, h, w, &g)) return rc;
    if (in == nullptr || weight == nullptr || out == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    if (in_mode != IN_NONE && in_mode != IN_RELU && !in_mode_is_u8(in_mode)) return fail(PPO_E_INVALID, "%s: unknown in_mode %d", what, in_mode);
    ForwardOp op{g, in, in_mode, weight, bias, residual, out, c3i::pix_m(g), cout, c3i::fwd_k(g)};
    hipLaunchKernelGGL(conv_gemm_kernel<ForwardOp>, gemm_grid(op.M, op.N, 1), dim3(kThreads), 0, as_stream(stream), op);
    return check_launch(what);
}

extern "C" int ppo_conv3x3_any_backward_data_f32(const float *dy, const float *weight, const float *relu_src, const float *dres,
                                                 float *dx, int n, int cin, int cout, int h, int w, void *stream)
{
    const char *what = "ppo_conv3x3_any_backward_data_f32";
    c3i::Geom g;
    if (int rc = check_geometry(what, n, cin, cout, h, w, &g)) return rc;
    if (dy == nullptr || weight == nullptr || dx == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    BackwardDataOp op{g, dy, weight, relu_src, dres, dx, c3i::pix_m(g), cin, c3i::dx_k(g)};
    hipLaunchKernelGGL(conv_gemm_kernel<BackwardDataOp>, gemm_grid(op.M, op.N, 1), dim3(kThreads), 0, as_stream(stream), op);
    return check_launch(what);
}

extern "C" size_t ppo_conv3x3_any_wgrad_workspace_bytes(int n, int cin, int cout, int h, int w)
{
    if (!c3i::geometry_ok(cin, cout, h, w)) return 0;
    const c3i::Geom g = c3i::make_geom(n, cin, cout, h, w);
    if (!c3i::sizes_ok(g)) return 0;
    int rows;
    const int slabs = wgrad_slabs(g, &rows);
    return (size_t)slabs * cout * (c3i::fwd_k(g) + 1) * sizeof(float);
}

extern "C" int ppo_conv3x3_any_backward_weight_f32(const void *in, int in_mode, const float *dy, float *dweight, float *dbias,
                                                   void *workspace, size_t workspace_bytes, int n, int cin, int cout, int h,
                                                   int w, int accumulate, void *stream)
{
    const char *what = "ppo_conv3x3_any_backward_weight_f32";
    c3i::Geom g;
    if (int rc = check_geometry(what, n, cin, cout, h, w, &g)) return rc;
    if (in == nullptr || dy == nullptr || dweight == nullptr || workspace == nullptr)
        return fail(PPO_E_INVALID, "%s: null pointer", what);
    if (in_mode != IN_NONE && in_mode != IN_RELU && !in_mode_is_u8(in_mode)) return fail(PPO_E_INVALID, "%s: unknown in_mode %d", what, in_mode);
    int rows;
    const int slabs = wgrad_slabs(g, &rows);
    const int K = c3i::fwd_k(g);
    const size_t need = (size_t)slabs * cout * (K + 1) * sizeof(float);
    if (workspace_bytes < need) return fail(PPO_E_INVALID, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
    if (!aligned(workspace, 4)) return fail(PPO_E_ALIGN, "%s: workspace not 4-byte aligned", what);
    BackwardWeightOp op{g, in, in_mode, dy, static_cast<float *>(workspace), rows, c3i::pix_m(g), K + 1, cout};
    hipLaunchKernelGGL(conv_gemm_kernel<BackwardWeightOp>, gemm_grid(op.M, op.N, slabs), dim3(kThreads), 0, as_stream(stream), op);
    if (int rc = check_launch(what)) return rc;
    const long long per_slab = (long long)cout * (K + 1);
    hipLaunchKernelGGL(any_wgrad_reduce_kernel, dim3((unsigned)((per_slab + 255) / 256)), dim3(256), 0, as_stream(stream),
                       static_cast<const float *>(workspace), dweight, dbias, slabs, cout, K, accumulate ? 1 : 0);
    return check_launch(what);
}

// ---- 3x3 / stride 2 / zero-padding 1: n, cin, cout, h, w describe the INPUT; out / dy are [n, cout, (h+1)/2, (w+1)/2]

extern "C" int ppo_conv3x3s2_any_supported(int cin, int cout, int h, int w) { return c3s::geometry_ok(cin, cout, h, w) ? 1 : 0; }

extern "C" int ppo_conv3x3s2_any_forward_f32(const void *in, int in_mode, const float *weight, const float *bias,
                                             const float *residual, float *out, int n, int cin, int cout, int h, int w,
                                             void *stream)
{
    const char *what = "ppo_conv3x3s2_any_forward_f32";
    c3s::Geom g;
    if (int rc = check_geometry_s2(what, n, cin, cout, h, w, &g)) return rc;
    if (in == nullptr || weight == nullptr || out == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    if (in_mode != IN_NONE && in_mode != IN_RELU && !in_mode_is_u8(in_mode)) return fail(PPO_E_INVALID, "%s: unknown in_mode %d", what, in_mode);
    S2ForwardOp op{g, in, in_mode, weight, bias, residual, out, c3s::fwd_m(g), cout, c3s::fwd_k(g)};
    hipLaunchKernelGGL(conv_gemm_kernel<S2ForwardOp>, gemm_grid(op.M, op.N, 1), dim3(kThreads), 0, as_stream(stream), op);
    return check_launch(what);
}

extern "C" int ppo_conv3x3s2_any_backward_data_f32(const float *dy, const float *weight, const float *relu_src,
                                                   const float *dres, float *dx, int n, int cin, int cout, int h, int w,
                                                   void *stream)
{
    const char *what = "ppo_conv3x3s2_any_backward_data_f32";
    c3s::Geom g;
    if (int rc = check_geometry_s2(what, n, cin, cout, h, w, &g)) return rc;
    if (dy == nullptr || weight == nullptr || dx == nullptr) return fail(PPO_E_INVALID, "%s: null pointer", what);
    S2BackwardDataOp op{g, dy, weight, relu_src, dres, dx, c3s::dx_m(g), cin, c3s::dx_k(g)};
    hipLaunchKernelGGL(conv_gemm_kernel<S2BackwardDataOp>, gemm_grid(op.M, op.N, 1), dim3(kThreads), 0, as_stream(stream), op);
    return check_launch(what);
}

extern "C" size_t ppo_conv3x3s2_any_wgrad_workspace_bytes(int n, int cin, int cout, int h, int w)
{
    if (!c3s::geometry_ok(cin, cout, h, w)) return 0;
    const c3s::Geom g = c3s::make_geom(n, cin, cout, h, w);
    if (!c3s::sizes_ok(g)) return 0;
    int rows;
    const int slabs = wgrad_slabs_s2(g, &rows);
    return (size_t)slabs * cout * (c3s::fwd_k(g) + 1) * sizeof(float);
}

extern "C" int ppo_conv3x3s2_any_backward_weight_f32(const void *in, int in_mode, const float *dy, float *dweight, float *dbias,
                                                     void *workspace, size_t workspace_bytes, int n, int cin, int cout, int h,
                                                     int w, int accumulate, void *stream)
{
    const char *what = "ppo_conv3x3s2_any_backward_weight_f32";
    c3s::Geom g;
    if (int rc = check_geometry_s2(what, n, cin, cout, h, w, &g)) return rc;
    if (in == nullptr || dy == nullptr || dweight == nullptr || workspace == nullptr)
        return fail(PPO_E_INVALID, "%s: null pointer", what);
    if (in_mode != IN_NONE && in_mode != IN_RELU && !in_mode_is_u8(in_mode)) return fail(PPO_E_INVALID, "%s: unknown in_mode %d", what, in_mode);
    int rows;
    const int slabs = wgrad_slabs_s2(g, &rows);
    const int K = c3s::fwd_k(g);
    const size_t need = (size_t)slabs * cout * (K + 1) * sizeof(float);
    if (workspace_bytes < need) return fail(PPO_E_INVALID, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
    if (!aligned(workspace, 4)) return fail(PPO_E_ALIGN, "%s: workspace not 4-byte aligned", what);
    S2BackwardWeightOp op{g, in, in_mode, dy, static_cast<float *>(workspace), rows, c3s::fwd_m(g), K + 1, cout};
    hipLaunchKernelGGL(conv_gemm_kernel<S2BackwardWeightOp>, gemm_grid(op.M, op.N, slabs), dim3(kThreads), 0, as_stream(stream), op);
    if (int rc = check_launch(what)) return rc;
    const long long per_slab = (long long)cout * (K + 1);
    hipLaunchKernelGGL(any_wgrad_reduce_kernel, dim3((unsigned)((per_slab + 255) / 256)), dim3(256), 0, as_stream(stream),
                       static_cast<const float *>(workspace), dweight, dbias, slabs, cout, K, accumulate ? 1 : 0);
    return check_launch(what);
}
