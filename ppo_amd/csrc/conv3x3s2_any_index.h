// Offset arithmetic of the generic 3x3 / stride 2 / zero-padding 1 convolution kernels in conv3x3_any.hip (the
// ppo_conv3x3s2_any_* entry points), as plain functions that also compile as ordinary C++
// (tests/test_conv3x3s2_any_index.py walks them on the host under a sanitizer).
//
// Tensors: activations NCHW, weights [cout, cin, 3, 3], contiguous; the input map is h x w, the output map
// ho x wo = (h + 1) / 2 x (w + 1) / 2: output (oy, ox) reads the input at (2 oy + ky - 1, 2 ox + kx - 1).
// GEMM views (row-major C[M, N] = A[M, K] * B[K, N]):
//   forward          M = n*ho*wo (img, oy, ox)   N = cout   K = 9*cin (ci, ky, kx)   A = padded, strided im2col(in)
//                                                                                     B = weight^T
//   backward-data    M = n*h*w (img, y, x)       N = cin    K = 9*cout (co, ky, kx)  A = the taps of dy that reach the dx
//                    element: dy[img, co, (y + 1 - ky) / 2, (x + 1 - kx) / 2] where both numerators are even and the
//                    quotient lies inside the output map                              B = weight
//   backward-weight  M = 9*cin + 1               N = cout   K = n*ho*wo, in slabs    A = padded, strided im2col(in)^T,
//                    last row all ones (its output row is dbias)                      B = dy
// An output pixel (OPix) or an input pixel (IPix) and a tap (Tap) are decomposed once each; fwd_tap_hits / dx_tap_hits
// say whether the tap exists and, only then, form its offset - a padding tap reads as zero by predicate and no
// out-of-range offset ever exists.
#pragma once

#include "conv_strided_index.h"  // the slab partition of a weight gradient's reduction is that family's

#if defined(__HIPCC__)
#define C3S_HD __host__ __device__ __forceinline__
#else
#define C3S_HD inline
#endif

namespace ppo {
namespace c3s {

struct Geom {
    int n, cin, cout, h, w, ho, wo;
};

C3S_HD Geom make_geom(int n, int cin, int cout, int h, int w)
{
    Geom g;
    g.n = n, g.cin = cin, g.cout = cout, g.h = h, g.w = w;
    g.ho = (h + 1) / 2, g.wo = (w + 1) / 2;
    return g;
}

// Geometries the kernels take: every extent in 1 .. 4096.  sizes_ok then checks, for a batch, that every tensor and
// GEMM extent fits the kernels' 32-bit row / column indices.
C3S_HD bool geometry_ok(int cin, int cout, int h, int w)
{
    return cin >= 1 && cout >= 1 && h >= 1 && w >= 1 && cin <= 4096 && cout <= 4096 && h <= 4096 && w <= 4096;
}
C3S_HD bool sizes_ok(const Geom &g)
{
    const long long lim = 1ll << 30;  // elements: byte offsets of float tensors stay below 2^32, GEMM indices below 2^31
    return g.n >= 1 && (long long)g.n * g.cin * g.h * g.w < lim && (long long)g.n * g.cout * g.ho * g.wo < lim &&
           (long long)g.cout * g.cin * 9 < lim;
}

C3S_HD long long in_elems(const Geom &g) { return (long long)g.n * g.cin * g.h * g.w; }
C3S_HD long long out_elems(const Geom &g) { return (long long)g.n * g.cout * g.ho * g.wo; }
C3S_HD long long weight_elems(const Geom &g) { return (long long)g.cout * g.cin * 9; }
C3S_HD int fwd_m(const Geom &g) { return g.n * g.ho * g.wo; }  // rows of the forward view, reduction of backward-weight
C3S_HD int dx_m(const Geom &g) { return g.n * g.h * g.w; }     // rows of the backward-data view
C3S_HD int fwd_k(const Geom &g) { return 9 * g.cin; }
C3S_HD int dx_k(const Geom &g) { return 9 * g.cout; }

// ---- an output pixel m = (img, oy, ox): out / dy element (m, co) at out_base + out_chan_off(co) + plane; the input
// elements it reads lie in image in_base
struct OPix {
    long long in_base;   // img * cin * h * w
    long long out_base;  // img * cout * ho * wo
    int plane, oy, ox;   // plane = oy * wo + ox
};
C3S_HD OPix opix(const Geom &g, int m)
{
    const int img = m / (g.ho * g.wo), p = m % (g.ho * g.wo);
    OPix r;
    r.in_base = (long long)img * g.cin * g.h * g.w;
    r.out_base = (long long)img * g.cout * g.ho * g.wo;
    r.plane = p, r.oy = p / g.wo, r.ox = p % g.wo;
    return r;
}
C3S_HD long long out_chan_off(const Geom &g, int co) { return (long long)co * g.ho * g.wo; }

// ---- an input pixel m = (img, y, x): dx / relu_src / dres element (m, ci) at dx_base + in_chan_off(ci) + plane; the
// dy elements that reach it lie in image dy_base
struct IPix {
    long long dx_base;  // img * cin * h * w
    long long dy_base;  // img * cout * ho * wo
    int plane, y, x;    // plane = y * w + x
};
C3S_HD IPix ipix(const Geom &g, int m)
{
    const int img = m / (g.h * g.w), p = m % (g.h * g.w);
    IPix r;
    r.dx_base = (long long)img * g.cin * g.h * g.w;
    r.dy_base = (long long)img * g.cout * g.ho * g.wo;
    r.plane = p, r.y = p / g.w, r.x = p % g.w;
    return r;
}
C3S_HD long long in_chan_off(const Geom &g, int ci) { return (long long)ci * g.h * g.w; }

// ---- a tap k = (c, ky, kx): channel c of the map read; w_off locates its weight
struct Tap {
    long long w_off;
    int c, ky, kx;
};
// forward / backward-weight: the input at (2 oy + ky - 1, 2 ox + kx - 1); weight[co, k] at fwd_weight_col(co) + w_off
C3S_HD Tap fwd_tap(const Geom &, int k)
{
    const int r = k % 9;
    Tap t;
    t.w_off = k, t.c = k / 9, t.ky = r / 3, t.kx = r % 3;
    return t;
}
C3S_HD long long fwd_weight_col(const Geom &g, int co) { return (long long)co * fwd_k(g); }
// whether tap t of output pixel p lies inside the image (else it is padding: zero), and the input element it reads
C3S_HD bool fwd_tap_hits(const Geom &g, const OPix &p, const Tap &t, long long *off)
{
    const int yy = 2 * p.oy + t.ky - 1, xx = 2 * p.ox + t.kx - 1;
    if (yy < 0 || yy >= g.h || xx < 0 || xx >= g.w) return false;
    *off = p.in_base + ((long long)t.c * g.h + yy) * g.w + xx;
    return true;
}

// backward-data: weight[co, ci, ky, kx] at w_off + dx_weight_col(ci)
C3S_HD Tap dx_tap(const Geom &g, int k)
{
    const int co = k / 9, r = k % 9;
    Tap t;
    t.w_off = (long long)co * g.cin * 9 + r, t.c = co, t.ky = r / 3, t.kx = r % 3;
    return t;
}
C3S_HD long long dx_weight_col(const Geom &, int ci) { return (long long)ci * 9; }
// whether tap t reaches input pixel p - 2 oy + ky - 1 == y and 2 ox + kx - 1 == x for an (oy, ox) inside the output
// map - and the dy element it reads
C3S_HD bool dx_tap_hits(const Geom &g, const IPix &p, const Tap &t, long long *off)
{
    const int ty = p.y + 1 - t.ky, tx = p.x + 1 - t.kx;  // 2 oy, 2 ox
    if (ty < 0 || tx < 0 || (ty & 1) || (tx & 1)) return false;
    const int oy = ty >> 1, ox = tx >> 1;
    if (oy >= g.ho || ox >= g.wo) return false;
    *off = p.dy_base + ((long long)t.c * g.ho + oy) * g.wo + ox;
    return true;
}

// ---- backward-weight: the reduction over the output pixels m is cut into slabs as the strided family's
using csi::slab_begin;
using csi::slab_count;
using csi::slab_end;
using csi::slab_rows;
// slab s's partial result [cout, 9 cin + 1] (last column: dbias) in the workspace
C3S_HD long long slab_off(const Geom &g, int s, int co, int k) { return ((long long)s * g.cout + co) * (fwd_k(g) + 1) + k; }

}  // namespace c3s
}  // namespace ppo
