// test_orient_map.cpp -- csrc/orient_map.h on the CPU (g++, ASan + UBSan): the
// map from the upright image to the stored one for the eight TIFF Orientation
// values, over every stored size from 1 x 1 to 70 x 70.
//
//  * bijection: every upright pixel names a stored pixel inside the image, and
//    no stored pixel is named twice;
//  * inverse: the map of o followed by the map of orient_inverse(o), taken on
//    the upright image's size, is the identity;
//  * table: the map is the one include/jp2hip.h's table states (numpy's flips,
//    swapaxes and rot90 written out);
//  * source rows: for every band [r0, r1) of upright rows, orient_source_rows
//    is exactly the range of stored rows the map reads, and, where the axes
//    swap, orient_source_cols exactly the range of stored columns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orient_map.h"

using namespace jp2hip;

static int g_fail = 0;
#define CHECK(c, ...)                                        \
    do {                                                     \
        if (!(c)) {                                          \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            if (++g_fail > 20) std::exit(1);                 \
        }                                                    \
    } while (0)

constexpr int kMax = 70;

// jp2hip.h's table, index by index: upright[uy][ux] = a[y][x]
static void table(int o, int w, int h, int ux, int uy, int &x, int &y) {
    switch (o) {
    case 1: x = ux; y = uy; break;
    case 2: x = w - 1 - ux; y = uy; break;                // a[:, ::-1]
    case 3: x = w - 1 - ux; y = h - 1 - uy; break;        // a[::-1, ::-1]
    case 4: x = ux; y = h - 1 - uy; break;                // a[::-1]
    case 5: x = uy; y = ux; break;                        // a.swapaxes(0, 1)
    case 6: x = uy; y = h - 1 - ux; break;                // rot90(a, -1)[i][j] = a[h - 1 - j][i]
    case 7: x = w - 1 - uy; y = h - 1 - ux; break;        // a[::-1, ::-1].swapaxes(0, 1)
    default: x = w - 1 - uy; y = ux; break;               // rot90(a, 1)[i][j] = a[j][w - 1 - i]
    }
}

static void check_size(int o, int w, int h) {
    int64_t ow, oh;
    orient_size(w, h, o, ow, oh);
    CHECK(ow == (o >= 5 ? h : w) && oh == (o >= 5 ? w : h), "o %d %dx%d: size %lld x %lld", o, w, h, (long long)ow,
          (long long)oh);
    CHECK(ow * oh == (int64_t)w * h, "o %d %dx%d: pixel count", o, w, h);
    std::vector<char> seen((size_t)w * h, 0);
    const int inv = orient_inverse(o);
    int64_t iw, ih;
    orient_size(ow, oh, inv, iw, ih);
    CHECK(iw == w && ih == h, "o %d %dx%d: inverse %d gives %lld x %lld", o, w, h, inv, (long long)iw, (long long)ih);
    for (int64_t uy = 0; uy < oh; uy++)
        for (int64_t ux = 0; ux < ow; ux++) {
            int64_t x, y;
            orient_source(o, w, h, ux, uy, x, y);
            CHECK(x >= 0 && x < w && y >= 0 && y < h, "o %d %dx%d: (%lld, %lld) -> (%lld, %lld) outside", o, w, h,
                  (long long)ux, (long long)uy, (long long)x, (long long)y);
            if (x < 0 || x >= w || y < 0 || y >= h) continue;
            CHECK(!seen[(size_t)(y * w + x)], "o %d %dx%d: stored (%lld, %lld) named twice", o, w, h, (long long)x,
                  (long long)y);
            seen[(size_t)(y * w + x)] = 1;
            int tx, ty;
            table(o, w, h, (int)ux, (int)uy, tx, ty);
            CHECK(tx == x && ty == y, "o %d %dx%d: (%lld, %lld) -> (%lld, %lld), the table says (%d, %d)", o, w, h,
                  (long long)ux, (long long)uy, (long long)x, (long long)y, tx, ty);
            // the stored image seen as the upright image's inverse: stored
            // pixel (x, y) is upright pixel (bx, by), which must be (ux, uy)
            int64_t bx, by;
            orient_source(inv, ow, oh, x, y, bx, by);
            CHECK(bx == ux && by == uy, "o %d %dx%d: inverse of (%lld, %lld) is (%lld, %lld)", o, w, h, (long long)ux,
                  (long long)uy, (long long)bx, (long long)by);
        }
    for (char s : seen) CHECK(s, "o %d %dx%d: a stored pixel is never named", o, w, h);
}

// every band of every upright height up to kMax, at three widths
static void check_rows(int o, int w, int h) {
    int64_t ow, oh;
    orient_size(w, h, o, ow, oh);
    for (int64_t r0 = 0; r0 <= oh; r0++)
        for (int64_t r1 = r0; r1 <= oh; r1++) {
            int64_t s0, s1;
            orient_source_rows(h, w, o, r0, r1, s0, s1);
            int64_t lo = INT64_MAX, hi = -1, clo = INT64_MAX, chi = -1;
            // (the map is separable: the first and last pixel of the first
            // and last row of the band reach every extreme)
            for (int64_t uy : {r0, r1 - 1})
                for (int64_t ux : {(int64_t)0, ow - 1}) {
                    if (r1 <= r0) continue;
                    int64_t x, y;
                    orient_source(o, w, h, ux, uy, x, y);
                    lo = y < lo ? y : lo;
                    hi = y > hi ? y : hi;
                    clo = x < clo ? x : clo;
                    chi = x > chi ? x : chi;
                }
            if (r1 <= r0) {
                CHECK(s0 == s1, "o %d %dx%d band [%lld, %lld): empty band reads rows", o, w, h, (long long)r0, (long long)r1);
                continue;
            }
            CHECK(s0 == lo && s1 == hi + 1, "o %d %dx%d band [%lld, %lld): rows [%lld, %lld), the map reads [%lld, %lld]", o,
                  w, h, (long long)r0, (long long)r1, (long long)s0, (long long)s1, (long long)lo, (long long)hi);
            if (orient_swaps(o)) {
                int64_t c0, c1;
                orient_source_cols(w, o, r0, r1, c0, c1);
                CHECK(c0 == clo && c1 == chi + 1, "o %d %dx%d band [%lld, %lld): columns [%lld, %lld), the map reads [%lld, %lld]",
                      o, w, h, (long long)r0, (long long)r1, (long long)c0, (long long)c1, (long long)clo, (long long)chi);
            }
        }
    // ranges past the image are clipped to it
    int64_t s0, s1, t0, t1;
    orient_source_rows(h, w, o, -5, oh + 9, s0, s1);
    orient_source_rows(h, w, o, 0, oh, t0, t1);
    CHECK(s0 == t0 && s1 == t1 && t0 == 0 && t1 == h, "o %d %dx%d: the whole image reads rows [%lld, %lld)", o, w, h,
          (long long)t0, (long long)t1);
}

int main() {
    for (int o = 1; o <= 8; o++) {
        CHECK(orient_valid(o), "o %d is valid", o);
        for (int h = 1; h <= kMax; h++)
            for (int w = 1; w <= kMax; w++) check_size(o, w, h);
        for (int n = 1; n <= kMax; n++)
            for (int m : {1, 7, kMax}) {
                check_rows(o, m, n);  // upright height n for o <= 4
                check_rows(o, n, m);  // ... and for o >= 5
            }
    }
    CHECK(!orient_valid(0) && !orient_valid(9) && !orient_valid(-1), "0, 9 and -1 are no orientations");
    if (g_fail) return 1;
    std::printf("ORIENT MAP OK\n");
    return 0;
}
