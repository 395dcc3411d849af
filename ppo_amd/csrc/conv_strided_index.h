// Offset arithmetic of the strided ("valid", no padding) convolution kernels in conv_strided.hip, as plain functions
// that also compile as ordinary C++ (tests/test_conv_strided_index.py walks them on the host under a sanitizer).
//
// Tensors: activations NCHW, weights OIHW, contiguous.  ho = (h - kh) / stride + 1, wo likewise.
// GEMM views (row-major C[M, N] = A[M, K] * B[K, N]):
//   forward          M = n*ho*wo (img, oy, ox)   N = cout   K = cin*kh*kw (ci, ky, kx)   A = im2col(in)   B = weight^T
//   backward-data    M = n*h*w   (img, y, x)     N = cin    K = cout*kh*kw (co, ky, kx)  A = the taps of dy that reach
//                    the dx element (zero where a tap does not exist)                      B = weight
//   backward-weight  M = cin*kh*kw + 1           N = cout   K = n*ho*wo, cut into slabs   A = im2col(in)^T, last row all
//                    ones (its output row is dbias)                                        B = dy
// Every element offset is split into a part that depends on the GEMM row and a part that depends on the GEMM column,
// so a thread decomposes each index once.
#pragma once

#if defined(__HIPCC__)
#define CSI_HD __host__ __device__ __forceinline__
#else
#define CSI_HD inline
#endif

namespace ppo {
namespace csi {

struct Geom {
    int n, cin, h, w, cout, kh, kw, stride, ho, wo;
};

CSI_HD Geom make_geom(int n, int cin, int h, int w, int cout, int kh, int kw, int stride)
{
    Geom g;
    g.n = n, g.cin = cin, g.h = h, g.w = w, g.cout = cout, g.kh = kh, g.kw = kw, g.stride = stride;
    g.ho = (h - kh) / stride + 1;
    g.wo = (w - kw) / stride + 1;
    return g;
}

// Geometries the kernels take: everything positive, the window inside the image, bounded extents.  sizes_ok then
// checks, for a batch, that every tensor and GEMM extent fits the kernels' 32-bit row / column indices.
CSI_HD bool geometry_ok(int cin, int cout, int kh, int kw, int stride, int h, int w)
{
    return cin >= 1 && cout >= 1 && kh >= 1 && kw >= 1 && stride >= 1 && h >= kh && w >= kw && cin <= 4096 && cout <= 4096 &&
           kh <= 16 && kw <= 16 && stride <= 16 && h <= 4096 && w <= 4096;
}
CSI_HD bool sizes_ok(const Geom &g)
{
    const long long lim = 1ll << 30;  // elements: byte offsets of float tensors stay below 2^32, GEMM indices below 2^31
    return g.n >= 1 && (long long)g.n * g.cin * g.h * g.w < lim && (long long)g.n * g.cout * g.ho * g.wo < lim &&
           (long long)g.cout * g.cin * g.kh * g.kw < lim;
}

CSI_HD long long in_elems(const Geom &g) { return (long long)g.n * g.cin * g.h * g.w; }
CSI_HD long long out_elems(const Geom &g) { return (long long)g.n * g.cout * g.ho * g.wo; }
CSI_HD long long weight_elems(const Geom &g) { return (long long)g.cout * g.cin * g.kh * g.kw; }
CSI_HD int fwd_m(const Geom &g) { return g.n * g.ho * g.wo; }
CSI_HD int fwd_k(const Geom &g) { return g.cin * g.kh * g.kw; }
CSI_HD int dx_m(const Geom &g) { return g.n * g.h * g.w; }
CSI_HD int dx_k(const Geom &g) { return g.cout * g.kh * g.kw; }

// ---- forward / backward-weight: in[in_row_base(m) + in_col_off(k)] is im2col(in)[m, k]
CSI_HD long long in_row_base(const Geom &g, int m)
{
    const int img = m / (g.ho * g.wo), pix = m % (g.ho * g.wo);
    const int oy = pix / g.wo, ox = pix % g.wo;
    return ((long long)img * g.cin * g.h + oy * g.stride) * g.w + ox * g.stride;
}
CSI_HD long long in_col_off(const Geom &g, int k)
{
    const int ci = k / (g.kh * g.kw), r = k % (g.kh * g.kw);
    const int ky = r / g.kw, kx = r % g.kw;
    return ((long long)ci * g.h + ky) * g.w + kx;
}
// out / dy / gate [n, cout, ho, wo]: element (m, co) at out_row_base(m) + out_col_off(co)
CSI_HD long long out_row_base(const Geom &g, int m)
{
    const int img = m / (g.ho * g.wo), pix = m % (g.ho * g.wo);
    return (long long)img * g.cout * g.ho * g.wo + pix;
}
CSI_HD long long out_col_off(const Geom &g, int co) { return (long long)co * g.ho * g.wo; }
// weight [cout, cin, kh, kw]: element (co, k) with k = (ci, ky, kx) flattened
CSI_HD long long weight_off(const Geom &g, int co, int k) { return (long long)co * fwd_k(g) + k; }

// ---- backward-data (gather form): dx element m = (img, y, x) of channel ci sums, over k = (co, ky, kx), the taps
// with oy * stride + ky == y and ox * stride + kx == x, 0 <= oy < ho, 0 <= ox < wo.
struct DxRow {
    long long dx_base;  // + ci * h * w
    long long dy_base;  // img * cout * ho * wo
    int qy, ry, qx, rx; // y = qy * stride + ry, x = qx * stride + rx
};
struct DxTap {
    long long w_base;   // (co * cin) * kh * kw + ky * kw + kx;  + ci * kh * kw
    int co, ay, ry, ax, rx; // ky = ay * stride + ry, kx = ax * stride + rx
};
CSI_HD DxRow dx_row(const Geom &g, int m)
{
    const int img = m / (g.h * g.w), pix = m % (g.h * g.w);
    const int y = pix / g.w, x = pix % g.w;
    DxRow r;
    r.dx_base = (long long)img * g.cin * g.h * g.w + pix;
    r.dy_base = (long long)img * g.cout * g.ho * g.wo;
    r.qy = y / g.stride, r.ry = y % g.stride, r.qx = x / g.stride, r.rx = x % g.stride;
    return r;
}
CSI_HD long long dx_col_off(const Geom &g, int ci) { return (long long)ci * g.h * g.w; }
CSI_HD DxTap dx_tap(const Geom &g, int k)
{
    const int co = k / (g.kh * g.kw), r = k % (g.kh * g.kw);
    const int ky = r / g.kw, kx = r % g.kw;
    DxTap t;
    t.w_base = (long long)co * g.cin * g.kh * g.kw + r;
    t.co = co;
    t.ay = ky / g.stride, t.ry = ky % g.stride, t.ax = kx / g.stride, t.rx = kx % g.stride;
    return t;
}
CSI_HD long long dx_weight_col_off(const Geom &g, int ci) { return (long long)ci * g.kh * g.kw; }
// whether tap t reaches row r, and the dy / gate element it reads
CSI_HD bool dx_tap_hits(const Geom &g, const DxRow &r, const DxTap &t, long long *dy_off)
{
    if (t.ry != r.ry || t.rx != r.rx) return false;
    const int oy = r.qy - t.ay, ox = r.qx - t.ax;
    if (oy < 0 || oy >= g.ho || ox < 0 || ox >= g.wo) return false;
    *dy_off = r.dy_base + ((long long)t.co * g.ho + oy) * g.wo + ox;
    return true;
}

// ---- backward-weight: the reduction over the rows m of the forward GEMM is cut into slabs of slab_rows(M) rows (a
// multiple of `ktile`), slab s = [s * rows, min(M, (s + 1) * rows)); at most `max_slabs` of them, none empty.
CSI_HD int slab_rows(int M, int max_slabs, int ktile)
{
    int rows = (M + max_slabs - 1) / max_slabs;
    rows = (rows + ktile - 1) / ktile * ktile;
    return rows < ktile ? ktile : rows;
}
CSI_HD int slab_count(int M, int rows) { return (M + rows - 1) / rows; }
CSI_HD int slab_begin(int s, int rows) { return s * rows; }
CSI_HD int slab_end(int M, int s, int rows) { return (s + 1) * rows < M ? (s + 1) * rows : M; }
// slab s's partial result [cout, K + 1] (column K: dbias) in the workspace
CSI_HD long long slab_off(const Geom &g, int s, int co, int k) { return ((long long)s * g.cout + co) * (fwd_k(g) + 1) + k; }

}  // namespace csi
}  // namespace ppo
