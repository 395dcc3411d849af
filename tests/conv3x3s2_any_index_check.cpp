// Host walk through csrc/conv3x3s2_any_index.h (built and run by tests/test_conv3x3s2_any_index.py with
// -fsanitize=address,undefined): for each geometry given on the command line as n,cin,cout,h,w (of the INPUT)
//   * every (m, k) of the forward / backward-weight view is either a padding tap - exactly where the definition of the
//     zero-padded stride-2 convolution says so - or lands inside the input on the element that definition names, and
//     every output's nine taps per channel are those of a brute-force enumeration; every (m, co) inside the output,
//     each once; every (co, k) inside the weights, each once;
//   * every dx element's taps are exactly those of a brute-force enumeration over (co, oy, ox, ky, kx), each reading the
//     right dy and weight elements, and every dx element is written once;
//   * the slabs of the weight gradient partition [0, n*ho*wo) in order, each a non-empty multiple of the K tile but the
//     last, and every slab element lies inside the workspace, each once.
// Prints "ok <count>" per geometry; any violation prints what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <utility>
#include <vector>

#include "conv3x3s2_any_index.h"

using namespace ppo::c3s;

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::printf("FAIL %s: ", #cond);   \
            std::printf(__VA_ARGS__);          \
            std::printf("\n");                 \
            if (++failures > 20) std::exit(1); \
        }                                      \
    } while (0)

static long long check_geometry(const Geom &g)
{
    long long count = 0;
    const int M = fwd_m(g), K = fwd_k(g);
    CHECK(geometry_ok(g.cin, g.cout, g.h, g.w) && sizes_ok(g), "geometry rejected");
    // the output side of torch.nn.Conv2d(., ., 3, stride=2, padding=1): floor((h + 2 - 3) / 2) + 1
    CHECK(g.ho == (g.h - 1) / 2 + 1 && g.wo == (g.w - 1) / 2 + 1, "output map %dx%d for input %dx%d", g.ho, g.wo, g.h, g.w);
    // touching real buffers lets the sanitizer see any offset that is out of range
    std::vector<unsigned char> in(in_elems(g), 0), out(out_elems(g), 0), wt(weight_elems(g), 0);
    for (int m = 0; m < M; ++m) {
        const int img = m / (g.ho * g.wo), oy = m / g.wo % g.ho, ox = m % g.wo;
        const OPix p = opix(g, m);
        std::vector<std::pair<long long, long long>> got, want;  // (input offset, k)
        for (int k = 0; k < K; ++k) {
            const int ci = k / 9, ky = k / 3 % 3, kx = k % 3;
            const int yy = 2 * oy + ky - 1, xx = 2 * ox + kx - 1;
            const bool inside = yy >= 0 && yy < g.h && xx >= 0 && xx < g.w;
            long long off = -1;
            const bool hit = fwd_tap_hits(g, p, fwd_tap(g, k), &off);
            CHECK(hit == inside, "tap m=%d k=%d: hit %d, inside %d", m, k, (int)hit, (int)inside);
            if (!hit) continue;
            const long long ref = (((long long)img * g.cin + ci) * g.h + yy) * g.w + xx;
            CHECK(off >= 0 && off < in_elems(g), "input offset %lld outside [0, %lld) at m=%d k=%d", off, in_elems(g), m, k);
            CHECK(off == ref, "input offset %lld != %lld at m=%d k=%d", off, ref, m, k);
            in[off] = 1;
            got.push_back({off, k});
            ++count;
        }
        // brute force: every input element (ci, y, x) of the image and every (ky, kx) with 2 oy + ky - 1 == y, 2 ox + kx - 1 == x
        for (int ci = 0; ci < g.cin; ++ci)
            for (int y = 0; y < g.h; ++y)
                for (int ky = 0; ky < 3; ++ky) {
                    if (2 * oy + ky - 1 != y) continue;
                    for (int x = 0; x < g.w; ++x)
                        for (int kx = 0; kx < 3; ++kx)
                            if (2 * ox + kx - 1 == x)
                                want.push_back({(((long long)img * g.cin + ci) * g.h + y) * g.w + x, (ci * 3 + ky) * 3 + kx});
                }
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        CHECK(got == want, "taps of output m=%d: %zu found, %zu expected", m, got.size(), want.size());
        for (int co = 0; co < g.cout; ++co) {
            const long long off = p.out_base + out_chan_off(g, co) + p.plane;
            const long long ref = (((long long)img * g.cout + co) * g.ho + oy) * g.wo + ox;
            CHECK(off >= 0 && off < out_elems(g) && off == ref, "output offset %lld (want %lld) at m=%d co=%d", off, ref, m, co);
            CHECK(out[off] == 0, "output element %lld written twice", off);
            out[off] = 1;
        }
    }
    // (an even side's last row / column is read only by the kernel's last tap, which exists: every input element is read)
    for (long long i = 0; i < in_elems(g); ++i) CHECK(in[i] == 1, "input element %lld never read", i);
    for (long long i = 0; i < out_elems(g); ++i) CHECK(out[i] == 1, "output element %lld never written", i);
    for (int co = 0; co < g.cout; ++co)
        for (int k = 0; k < K; ++k) {
            const long long off = fwd_weight_col(g, co) + fwd_tap(g, k).w_off;
            const long long ref = ((long long)co * g.cin + k / 9) * 9 + k % 9;
            CHECK(off >= 0 && off < weight_elems(g) && off == ref && wt[off] == 0, "weight offset %lld at co=%d k=%d", off, co, k);
            wt[off] = 1;
        }

    // backward-data: taps per dx element against brute force
    const int Mx = dx_m(g), Kx = dx_k(g);
    std::vector<unsigned char> dx(in_elems(g), 0);
    for (int m = 0; m < Mx; ++m) {
        const int img = m / (g.h * g.w), y = m / g.w % g.h, x = m % g.w;
        const IPix p = ipix(g, m);
        std::vector<std::pair<long long, long long>> got, want;  // (dy offset, weight offset at ci = 0)
        for (int k = 0; k < Kx; ++k) {
            const Tap tap = dx_tap(g, k);
            long long dy_off = -1;
            if (!dx_tap_hits(g, p, tap, &dy_off)) continue;
            CHECK(dy_off >= 0 && dy_off < out_elems(g), "dy offset %lld outside at m=%d k=%d", dy_off, m, k);
            out[dy_off] = 2;
            got.push_back({dy_off, tap.w_off});
            for (int ci = 0; ci < g.cin; ++ci) {
                const long long w_off = tap.w_off + dx_weight_col(g, ci);
                CHECK(w_off >= 0 && w_off < weight_elems(g), "weight offset %lld outside at k=%d ci=%d", w_off, k, ci);
                wt[w_off] = 2;
            }
            ++count;
        }
        // dy[img, co, oy, ox] reaches dx[img, ., y, x] through weight tap (ky, kx) when 2 oy + ky - 1 == y, 2 ox + kx - 1 == x
        for (int oy = 0; oy < g.ho; ++oy)
            for (int ky = 0; ky < 3; ++ky) {
                if (2 * oy + ky - 1 != y) continue;
                for (int ox = 0; ox < g.wo; ++ox)
                    for (int kx = 0; kx < 3; ++kx) {
                        if (2 * ox + kx - 1 != x) continue;
                        for (int co = 0; co < g.cout; ++co)
                            want.push_back({(((long long)img * g.cout + co) * g.ho + oy) * g.wo + ox,
                                            (((long long)co * g.cin) * 3 + ky) * 3 + kx});
                    }
            }
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        CHECK(std::adjacent_find(got.begin(), got.end()) == got.end(), "a tap of dx element m=%d is repeated", m);
        CHECK(got == want, "taps of dx element m=%d: %zu found, %zu expected", m, got.size(), want.size());
        for (int ci = 0; ci < g.cin; ++ci) {
            const long long off = p.dx_base + in_chan_off(g, ci) + p.plane;
            const long long ref = (((long long)img * g.cin + ci) * g.h + y) * g.w + x;
            CHECK(off >= 0 && off < in_elems(g) && off == ref && dx[off] == 0, "dx offset %lld (want %lld) at m=%d ci=%d", off, ref, m, ci);
            dx[off] = 1;
        }
    }
    for (long long i = 0; i < in_elems(g); ++i) CHECK(dx[i] == 1, "dx element %lld never written", i);
    for (long long i = 0; i < out_elems(g); ++i) CHECK(out[i] == 2, "dy element %lld never read", i);
    if (g.h >= 3 && g.w >= 3)  // (with one output row or column the taps ky = 0 / kx = 0 are padding everywhere)
        for (long long i = 0; i < weight_elems(g); ++i) CHECK(wt[i] == 2, "weight element %lld never read by backward-data", i);

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
        for (size_t i = 0; i < ws.size(); ++i) CHECK(ws[i] == 1, "workspace element %zu never written", i);
    }
    return count;
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        int v[5];
        if (std::sscanf(argv[a], "%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4) != 5) {
            std::printf("bad geometry '%s'\n", argv[a]);
            return 2;
        }
        const Geom g = make_geom(v[0], v[1], v[2], v[3], v[4]);
        const long long count = check_geometry(g);
        std::printf("ok %lld %s\n", count, argv[a]);
    }
    // what supported() and the size check must turn down
    if (geometry_ok(0, 16, 8, 8) || geometry_ok(4, 0, 8, 8) || geometry_ok(4, 16, 0, 8) || geometry_ok(4, 16, 8, 0) ||
        geometry_ok(4097, 16, 8, 8) || geometry_ok(4, 4097, 8, 8) || geometry_ok(4, 16, 4097, 8) || geometry_ok(4, 16, 8, 4097) ||
        !geometry_ok(1, 1, 1, 1) || !geometry_ok(4096, 4096, 4096, 4096) || sizes_ok(make_geom(0, 4, 16, 8, 8)) ||
        sizes_ok(make_geom(-1, 4, 16, 8, 8)) || sizes_ok(make_geom(1, 64, 1, 4096, 4096)) ||
        sizes_ok(make_geom(1, 1, 256, 4096, 4096)) /* the output is a quarter of the stride-1 one */ ||
        !sizes_ok(make_geom(1, 1, 64, 4096, 4096)) || !sizes_ok(make_geom(1, 4096, 4096, 64, 64)) /* 9 * 2^24 weights: fine */ ||
        sizes_ok(make_geom(1 << 20, 1, 1, 32, 32))) {
        std::printf("FAIL: the geometry / size checks accept or reject the wrong cases\n");
        return 1;
    }
    return failures ? 1 : 0;
}
