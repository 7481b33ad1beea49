// test_dwt_chunk.cpp -- csrc/dwt_chunk.h on the CPU (g++, ASan + UBSan): the
// column chunks the DWT kernels take when a level's rows do not fit in LDS.
//
//  * geometry: for every row width 1..20000 and each chunked kernel's kept
//    width, the kept ranges tile [0, W) exactly once, every chunk starts on a
//    multiple of 16, the staged range lies inside the row, the four
//    neighbours on each side of a kept sample are staged or beyond a true row
//    end, and the low / high output ranges are disjoint and cover
//    [0, ceil(W/2)) and [0, floor(W/2));
//  * lifting: random rows lifted chunk by chunk -- each chunk sees only its
//    staged samples, a buffer of exactly that many (ASan's red zones on both
//    sides), an update whose neighbour is not staged is skipped as the
//    kernels leave a window's edge stale -- equal whole-row lifting written
//    out here, bit for bit, 5/3 on int32 and 9/7 on float, for widths around
//    every chunk boundary.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "dwt_chunk.h"

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

static const int kKept[] = {kL1ChunkW, kBandChunkW};

static void geometry(int W, int C) {
    const int n = dwt_chunk_count(W, C);
    const int nlo = (W + 1) / 2, nhi = W / 2;
    int next = 0, next_lo = 0, next_hi = 0;
    CHECK(n >= 1, "W %d C %d: no chunk", W, C);
    for (int k = 0; k < n; k++) {
        const DwtChunk c = dwt_chunk(W, C, k);
        CHECK(c.c0 == next && c.c1 > c.c0 && c.c1 <= W, "W %d C %d k %d: kept [%d, %d) after %d", W, C, k, c.c0, c.c1, next);
        next = c.c1;
        CHECK(c.c0 % 16 == 0, "W %d C %d k %d: start %d", W, C, k, c.c0);
        CHECK(c.c1 - c.c0 <= C, "W %d C %d k %d: keeps %d", W, C, k, c.c1 - c.c0);
        CHECK(0 <= c.s0 && c.s0 <= c.c0 && c.c1 <= c.s1 && c.s1 <= W, "W %d C %d k %d: staged [%d, %d)", W, C, k, c.s0, c.s1);
        CHECK(c.s1 - c.s0 <= dwt_chunk_staged(C), "W %d C %d k %d: stages %d", W, C, k, c.s1 - c.s0);
        // the footprint of the first and last kept sample (the others lie between)
        for (int d = 1; d <= 4; d++) {
            CHECK(c.c0 - d >= c.s0 || c.c0 - d < 0, "W %d C %d k %d: left neighbour %d", W, C, k, c.c0 - d);
            CHECK(c.c1 - 1 + d < c.s1 || c.c1 - 1 + d > W - 1, "W %d C %d k %d: right neighbour %d", W, C, k, c.c1 - 1 + d);
        }
        CHECK(c.lo0 == next_lo && c.nlo >= 0, "W %d C %d k %d: low [%d, +%d) after %d", W, C, k, c.lo0, c.nlo, next_lo);
        CHECK(c.hi0 == next_hi && c.nhi >= 0, "W %d C %d k %d: high [%d, +%d) after %d", W, C, k, c.hi0, c.nhi, next_hi);
        next_lo = c.lo0 + c.nlo;
        next_hi = c.hi0 + c.nhi;
        // sample c0 + 2 j is low output c0 / 2 + j, sample c0 + 2 j + 1 high output c0 / 2 + j
        CHECK(c.lo0 * 2 == c.c0 && c.hi0 * 2 == c.c0, "W %d C %d k %d: outputs not at c0 / 2", W, C, k);
        CHECK(c.nlo == (c.c1 + 1) / 2 - c.c0 / 2 && c.nhi == c.c1 / 2 - c.c0 / 2, "W %d C %d k %d: output counts", W, C, k);
    }
    CHECK(next == W && next_lo == nlo && next_hi == nhi, "W %d C %d: covers %d, low %d, high %d", W, C, next, next_lo, next_hi);
}

// ---- lifting: oracle_fdwt's expressions (fwd53_1d / fwd97_1d), one row ----
static const float A97 = -1.586134342059924f, B97 = -0.052980118572961f, G97 = 0.882911075530934f,
                   D97 = 0.443506852043971f, K97 = 1.230174104914001f, INVK97 = 0.8128930661159609f;

static inline void update(int32_t &x, int32_t l, int32_t r, int step) {
    if (step == 0) x -= (l + r) >> 1;
    else x += (l + r + 2) >> 2;
}
static inline void update(float &x, float l, float r, int step) {
    const float cf = step == 0 ? A97 : (step == 1 ? B97 : (step == 2 ? G97 : D97));
    float t = l + r;
    t = cf * t;
    x = x + t;
}
template <typename T> constexpr int steps() { return std::is_same<T, float>::value ? 4 : 2; }
static inline int32_t scaled(int32_t v, bool) { return v; }
static inline float scaled(float v, bool odd) { return v * (odd ? K97 : INVK97); }

// whole-row lifting, de-interleaved: low outputs then high outputs
template <typename T>
static std::vector<T> lift_row(const std::vector<T> &in) {
    const int W = (int)in.size();
    std::vector<T> x = in, out((size_t)W);
    if (W > 1) {
        for (int s = 0; s < steps<T>(); s++)
            for (int i = (s & 1) ? 0 : 1; i < W; i += 2) {
                const int l = i > 0 ? i - 1 : i + 1, r = i + 1 < W ? i + 1 : i - 1;
                update(x[(size_t)i], x[(size_t)l], x[(size_t)r], s);
            }
    }
    const int nlo = (W + 1) / 2;
    for (int i = 0; i < W; i++) out[(size_t)((i & 1) ? nlo + i / 2 : i / 2)] = W > 1 ? scaled(x[(size_t)i], (i & 1) != 0) : x[(size_t)i];
    return out;
}

// the same row, chunk by chunk with the header's geometry
template <typename T>
static std::vector<T> lift_chunks(const std::vector<T> &in, int C, T poison) {
    const int W = (int)in.size();
    std::vector<T> out((size_t)W, poison);
    std::vector<char> written((size_t)W, 0);
    const int nlo = (W + 1) / 2;
    for (int k = 0; k < dwt_chunk_count(W, C); k++) {
        const DwtChunk c = dwt_chunk(W, C, k);
        // exactly the staged samples: sample x at st[x - c.s0]
        T *st = (T *)std::malloc(sizeof(T) * (size_t)(c.s1 - c.s0));
        std::memcpy(st, in.data() + c.s0, sizeof(T) * (size_t)(c.s1 - c.s0));
        if (W > 1) {
            for (int s = 0; s < steps<T>(); s++)
                for (int i = c.s0 + ((c.s0 & 1) == ((s & 1) ? 0 : 1) ? 0 : 1); i < c.s1; i += 2) {
                    const int l = i > 0 ? i - 1 : i + 1, r = i + 1 < W ? i + 1 : i - 1;  // true row ends only
                    if (l < c.s0 || l >= c.s1 || r < c.s0 || r >= c.s1) continue;      // stale halo edge
                    update(st[i - c.s0], st[l - c.s0], st[r - c.s0], s);
                }
        }
        for (int j = 0; j < c.nlo; j++) {
            const T v = st[c.c0 + 2 * j - c.s0];
            const size_t o = (size_t)(c.lo0 + j);
            CHECK(!written[o], "low output %zu written twice", o);
            written[o] = 1;
            out[o] = W > 1 ? scaled(v, false) : v;
        }
        for (int j = 0; j < c.nhi; j++) {
            const T v = st[c.c0 + 2 * j + 1 - c.s0];
            const size_t o = (size_t)(nlo + c.hi0 + j);
            CHECK(!written[o], "high output %zu written twice", o);
            written[o] = 1;
            out[o] = scaled(v, true);
        }
        std::free(st);
    }
    for (int i = 0; i < W; i++) CHECK(written[(size_t)i], "W %d C %d: output %d not written", W, C, i);
    return out;
}

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

static long lifting(int W, int C) {
    std::vector<int32_t> xi((size_t)W);
    std::vector<float> xf((size_t)W);
    for (int i = 0; i < W; i++) {
        xi[(size_t)i] = (int32_t)(rnd() & 0xFFFF) - 32768;                 // level-shifted 16-bit samples
        xf[(size_t)i] = (float)((int32_t)(rnd() & 0xFFFF) - 32768) * 0.37f;  // any floats: rounding in every step
    }
    const std::vector<int32_t> wi = lift_row(xi), ci = lift_chunks(xi, C, INT32_MIN);
    const std::vector<float> wf = lift_row(xf), cf = lift_chunks(xf, C, -1.0f);
    CHECK(std::memcmp(wi.data(), ci.data(), sizeof(int32_t) * (size_t)W) == 0, "5/3: W %d C %d differs from whole-row lifting", W, C);
    CHECK(std::memcmp(wf.data(), cf.data(), sizeof(float) * (size_t)W) == 0, "9/7: W %d C %d differs from whole-row lifting", W, C);
    return 2;
}

int main() {
    long ngeo = 0, nlift = 0;
    for (int C : kKept) {
        CHECK(C > 0 && C % 16 == 0, "kept width %d", C);
        for (int W = 1; W <= 20000; W++) {
            geometry(W, C);
            ngeo++;
        }
        // widths around every chunk boundary up to 6 chunks, and a few small and large ones
        for (int m = 1; m <= 6; m++)
            for (int d = -18; d <= 18; d++) nlift += lifting(m * C + d, C);
        for (int W : {1, 2, 3, 4, 5, 15, 16, 17, 12345, 20000}) nlift += lifting(W, C);
    }
    if (g_fail) {
        std::printf("DWT CHUNK FAILED: %d checks\n", g_fail);
        return 1;
    }
    std::printf("DWT CHUNK OK kL1ChunkW=%d kBandChunkW=%d halo=%d: %ld geometries, %ld rows lifted\n", kL1ChunkW,
                kBandChunkW, kDwtChunkHalo, ngeo, nlift);
    return 0;
}
