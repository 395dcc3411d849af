// Offset arithmetic of the generic 3x3 / stride 1 / zero-padding 1 convolution kernels in conv3x3_any.hip, as plain
// functions that also compile as ordinary C++ (tests/test_conv3x3_any_index.py walks them on the host under a
// sanitizer).
//
// Tensors: activations NCHW, weights [cout, cin, 3, 3], contiguous; the output map has the input's h x w.
// GEMM views (row-major C[M, N] = A[M, K] * B[K, N]):
//   forward          M = n*h*w (img, y, x)   N = cout   K = 9*cin (ci, ky, kx)   A = padded im2col(in)   B = weight^T
//   backward-data    M = n*h*w (img, y, x)   N = cin    K = 9*cout (co, ky, kx)  A = the taps of dy that reach the dx
//                    element: dy[img, co, y - ky + 1, x - kx + 1]                  B = weight
//   backward-weight  M = 9*cin + 1           N = cout   K = n*h*w, cut into slabs  A = padded im2col(in)^T, last row
//                    all ones (its output row is dbias)                            B = dy
// All three A operands read a map of some channel count at (pixel + displacement): a pixel (Pix) and a tap (Tap) are
// decomposed once each, and tap_hits says whether the displaced position lies inside the image and, only then, forms
// its offset - a padding tap reads as zero by predicate and no out-of-range offset ever exists.
#pragma once

#include "conv_strided_index.h"  // the slab partition of a weight gradient's reduction is that family's

#if defined(__HIPCC__)
#define C3I_HD __host__ __device__ __forceinline__
#else
#define C3I_HD inline
#endif

namespace ppo {
namespace c3i {

struct Geom {
    int n, cin, cout, h, w;
};

C3I_HD Geom make_geom(int n, int cin, int cout, int h, int w)
{
    Geom g;
    g.n = n, g.cin = cin, g.cout = cout, g.h = h, g.w = w;
    return g;
}

// Geometries the kernels take: every extent in 1 .. 4096.  sizes_ok then checks, for a batch, that every tensor and
// GEMM extent fits the kernels' 32-bit row / column indices.
C3I_HD bool geometry_ok(int cin, int cout, int h, int w)
{
    return cin >= 1 && cout >= 1 && h >= 1 && w >= 1 && cin <= 4096 && cout <= 4096 && h <= 4096 && w <= 4096;
}
C3I_HD bool sizes_ok(const Geom &g)
{
    const long long lim = 1ll << 30;  // elements: byte offsets of float tensors stay below 2^32, GEMM indices below 2^31
    return g.n >= 1 && (long long)g.n * g.cin * g.h * g.w < lim && (long long)g.n * g.cout * g.h * g.w < lim &&
           (long long)g.cout * g.cin * 9 < lim;
}

C3I_HD long long in_elems(const Geom &g) { return (long long)g.n * g.cin * g.h * g.w; }
C3I_HD long long out_elems(const Geom &g) { return (long long)g.n * g.cout * g.h * g.w; }
C3I_HD long long weight_elems(const Geom &g) { return (long long)g.cout * g.cin * 9; }
C3I_HD int pix_m(const Geom &g) { return g.n * g.h * g.w; }  // rows of the forward / backward-data views
C3I_HD int fwd_k(const Geom &g) { return 9 * g.cin; }
C3I_HD int dx_k(const Geom &g) { return 9 * g.cout; }

// ---- a pixel m = (img, y, x) of a map with `channels` channels: element (m, c) at base + chan_off(c) + plane
struct Pix {
    long long base;   // img * channels * h * w
    int plane, y, x;  // plane = y * w + x
};
C3I_HD Pix pix(const Geom &g, int m, int channels)
{
    const int img = m / (g.h * g.w), p = m % (g.h * g.w);
    Pix r;
    r.base = (long long)img * channels * g.h * g.w;
    r.plane = p, r.y = p / g.w, r.x = p % g.w;
    return r;
}
C3I_HD long long chan_off(const Geom &g, int c) { return (long long)c * g.h * g.w; }

// ---- a tap k = (c, ky, kx): channel c of the map read, displaced by (dy, dx); w_off locates its weight
struct Tap {
    long long w_off;
    int c, dy, dx;
};
// forward / backward-weight: the input at (y + ky - 1, x + kx - 1); weight[co, k] at fwd_weight_col(co) + w_off
C3I_HD Tap fwd_tap(const Geom &, int k)
{
    const int r = k % 9;
    Tap t;
    t.w_off = k, t.c = k / 9, t.dy = r / 3 - 1, t.dx = r % 3 - 1;
    return t;
}
C3I_HD long long fwd_weight_col(const Geom &g, int co) { return (long long)co * fwd_k(g); }
// backward-data: dy at (y - ky + 1, x - kx + 1); weight[co, ci, ky, kx] at w_off + dx_weight_col(ci)
C3I_HD Tap dx_tap(const Geom &g, int k)
{
    const int co = k / 9, r = k % 9;
    Tap t;
    t.w_off = (long long)co * g.cin * 9 + r, t.c = co, t.dy = 1 - r / 3, t.dx = 1 - r % 3;
    return t;
}
C3I_HD long long dx_weight_col(const Geom &, int ci) { return (long long)ci * 9; }

// whether tap t of pixel p lies inside the image (else it is padding: zero), and the element it reads
C3I_HD bool tap_hits(const Geom &g, const Pix &p, const Tap &t, long long *off)
{
    const int yy = p.y + t.dy, xx = p.x + t.dx;
    if (yy < 0 || yy >= g.h || xx < 0 || xx >= g.w) return false;
    *off = p.base + ((long long)t.c * g.h + yy) * g.w + xx;
    return true;
}

// ---- backward-weight: the reduction over the pixels m is cut into slabs as the strided family's (conv_strided_index.h)
using csi::slab_begin;
using csi::slab_count;
using csi::slab_end;
using csi::slab_rows;
// slab s's partial result [cout, 9 cin + 1] (last column: dbias) in the workspace
C3I_HD long long slab_off(const Geom &g, int s, int co, int k) { return ((long long)s * g.cout + co) * (fwd_k(g) + 1) + k; }

}  // namespace c3i
}  // namespace ppo
