// Host walk through csrc/conv_strided_index.h (built and run by tests/test_conv_strided_index.py with
// -fsanitize=address,undefined): for each geometry given on the command line as n,cin,h,w,cout,kh,kw,stride
//   * every (m, k) of the forward / backward-weight view lands inside the input, and on exactly the element the
//     definition of the convolution names; every (m, co) inside the output; every (co, k) inside the weights;
//   * every dx element's taps are exactly those of a brute-force enumeration over (co, oy, ox, ky, kx), each reading
//     the right dy and weight elements;
//   * the slabs of the weight gradient partition [0, M) in order, each a non-empty multiple of the K tile but the last,
//     and every slab element lies inside the workspace.
// Prints "ok <count>" per geometry; any violation prints what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <utility>
#include <vector>

#include "conv_strided_index.h"

using namespace ppo::csi;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::printf("FAIL %s: ", #cond);  \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
            if (++failures > 20) std::exit(1); \
        }                                     \
    } while (0)

static long long check_geometry(const Geom &g)
{
    long long count = 0;
    const int M = fwd_m(g), K = fwd_k(g);
    CHECK(geometry_ok(g.cin, g.cout, g.kh, g.kw, g.stride, g.h, g.w) && sizes_ok(g), "geometry rejected");
    // touching real buffers lets the sanitizer see any offset that is out of range
    std::vector<unsigned char> in(in_elems(g), 0), out(out_elems(g), 0), wt(weight_elems(g), 0);
    for (int m = 0; m < M; ++m) {
        const int img = m / (g.ho * g.wo), oy = m / g.wo % g.ho, ox = m % g.wo;
        const long long rb = in_row_base(g, m);
        for (int k = 0; k < K; ++k) {
            const int ci = k / (g.kh * g.kw), ky = k / g.kw % g.kh, kx = k % g.kw;
            const long long off = rb + in_col_off(g, k);
            const long long want = (((long long)img * g.cin + ci) * g.h + oy * g.stride + ky) * g.w + ox * g.stride + kx;
            CHECK(off >= 0 && off < in_elems(g), "input offset %lld outside [0, %lld) at m=%d k=%d", off, in_elems(g), m, k);
            CHECK(off == want, "input offset %lld != %lld at m=%d k=%d", off, want, m, k);
            in[off] = 1;
            ++count;
        }
        for (int co = 0; co < g.cout; ++co) {
            const long long off = out_row_base(g, m) + out_col_off(g, co);
            const long long want = (((long long)img * g.cout + co) * g.ho + oy) * g.wo + ox;
            CHECK(off >= 0 && off < out_elems(g) && off == want, "output offset %lld (want %lld) at m=%d co=%d", off, want, m, co);
            CHECK(out[off] == 0, "output element %lld written twice", off);
            out[off] = 1;
        }
    }
    for (long long i = 0; i < out_elems(g); ++i) CHECK(out[i] == 1, "output element %lld never written", i);
    for (int co = 0; co < g.cout; ++co)
        for (int k = 0; k < K; ++k) {
            const long long off = weight_off(g, co, k);
            CHECK(off >= 0 && off < weight_elems(g) && wt[off] == 0, "weight offset %lld at co=%d k=%d", off, co, k);
            wt[off] = 1;
        }

    // backward-data: taps per dx element against brute force
    const int Mx = dx_m(g), Kx = dx_k(g);
    std::vector<unsigned char> dx(in_elems(g), 0);
    for (int m = 0; m < Mx; ++m) {
        const int img = m / (g.h * g.w), y = m / g.w % g.h, x = m % g.w;
        const DxRow row = dx_row(g, m);
        std::vector<std::pair<long long, long long>> got, want;  // (dy offset, weight offset at ci = 0)
        for (int k = 0; k < Kx; ++k) {
            const DxTap tap = dx_tap(g, k);
            long long dy_off = -1;
            if (!dx_tap_hits(g, row, tap, &dy_off)) continue;
            CHECK(dy_off >= 0 && dy_off < out_elems(g), "dy offset %lld outside at m=%d k=%d", dy_off, m, k);
            out[dy_off] = 2;
            got.push_back({dy_off, tap.w_base});
            for (int ci = 0; ci < g.cin; ++ci) {
                const long long w_off = tap.w_base + dx_weight_col_off(g, ci);
                CHECK(w_off >= 0 && w_off < weight_elems(g), "weight offset %lld outside at k=%d ci=%d", w_off, k, ci);
                wt[w_off] = 2;
            }
            ++count;
        }
        for (int oy = 0; oy < g.ho; ++oy)
            for (int ky = 0; ky < g.kh; ++ky) {
                if (oy * g.stride + ky != y) continue;
                for (int ox = 0; ox < g.wo; ++ox)
                    for (int kx = 0; kx < g.kw; ++kx) {
                        if (ox * g.stride + kx != x) continue;
                        for (int co = 0; co < g.cout; ++co)
                            want.push_back({(((long long)img * g.cout + co) * g.ho + oy) * g.wo + ox,
                                            (((long long)co * g.cin) * g.kh + ky) * g.kw + kx});
                    }
            }
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        CHECK(std::adjacent_find(got.begin(), got.end()) == got.end(), "a tap of dx element m=%d is repeated", m);
        CHECK(got == want, "taps of dx element m=%d: %zu found, %zu expected", m, got.size(), want.size());
        for (int ci = 0; ci < g.cin; ++ci) {
            const long long off = row.dx_base + dx_col_off(g, ci);
            const long long ref = (((long long)img * g.cin + ci) * g.h + y) * g.w + x;
            CHECK(off >= 0 && off < in_elems(g) && off == ref && dx[off] == 0, "dx offset %lld (want %lld) at m=%d ci=%d", off, ref, m, ci);
            dx[off] = 1;
        }
    }
    for (long long i = 0; i < in_elems(g); ++i) CHECK(dx[i] == 1, "dx element %lld never written", i);

    // backward-weight slabs
    const int ktile = 16;
    for (int max_slabs : {1, 3, 64}) {
        const int rows = slab_rows(M, max_slabs, ktile), slabs = slab_count(M, rows);
        CHECK(rows % ktile == 0 && slabs >= 1 && slabs <= max_slabs, "slab plan rows=%d slabs=%d for M=%d", rows, slabs, M);
        std::vector<unsigned char> ws((size_t)slabs * g.cout * (K + 1), 0);
        int next = 0;
        for (int s = 0; s < slabs; ++s) {
            const int b = slab_begin(s, rows), e = slab_end(M, s, rows);
            CHECK(b == next && e > b && e <= M, "slab %d = [%d, %d), expected to start at %d", s, b, e, next);
            next = e;
            for (int co = 0; co < g.cout; ++co)
                for (int k = 0; k <= K; ++k) {
                    const long long off = slab_off(g, s, co, k);
                    CHECK(off >= 0 && off < (long long)ws.size() && ws[off] == 0, "slab offset %lld at s=%d co=%d k=%d", off, s, co, k);
                    ws[off] = 1;
                }
        }
        CHECK(next == M, "slabs end at %d, M = %d", next, M);
    }
    return count;
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        int v[8];
        if (std::sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) != 8) {
            std::printf("bad geometry '%s'\n", argv[a]);
            return 2;
        }
        const Geom g = make_geom(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        const long long count = check_geometry(g);
        std::printf("ok %lld %s\n", count, argv[a]);
    }
    // what supported() must turn down
    if (geometry_ok(4, 32, 8, 8, 4, 7, 84) || geometry_ok(4, 32, 8, 8, 0, 84, 84) || geometry_ok(0, 32, 8, 8, 4, 84, 84) ||
        geometry_ok(4, 0, 8, 8, 4, 84, 84) || geometry_ok(4, 32, 0, 8, 4, 84, 84)) {
        std::printf("FAIL: an impossible geometry was accepted\n");
        return 1;
    }
    return failures ? 1 : 0;
}
