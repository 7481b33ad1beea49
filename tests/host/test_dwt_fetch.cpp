// test_dwt_fetch.cpp -- csrc/dwt_fetch.h on the CPU (g++, ASan + UBSan): the
// one-access-per-pixel fetch of k_dwt_l1s never leaves its source buffer and
// brings the samples the per-sample path reads.
//
//  * bounds: for every layout below the source is a heap block of exactly
//    the file's bytes (ASan's red zones stand on both sides), every pixel of
//    every row is fetched the way the kernel does it, and the access
//    [addr - back, addr - back + load) is checked against [0, nbytes);
//  * extraction: every fetched pixel's samples equal the bytes read one by
//    one; all 256 byte values and all 65 536 16-bit values, in both byte
//    orders and every component slot, and the level-shifted float formed
//    both ways (convert-then-subtract, subtract-then-convert) bit for bit.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dwt_fetch.h"

using namespace jp2hip;

static int g_fail = 0;
#define CHECK(c, ...)                                 \
    do {                                              \
        if (!(c)) {                                   \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                 \
            std::printf("\n");                        \
            if (++g_fail > 20) std::exit(1);          \
        }                                             \
    } while (0)

static uint32_t ref_sample(const uint8_t *p, int bps, bool be) {
    if (bps == 1) return p[0];
    return be ? ((uint32_t)p[0] << 8) | p[1] : p[0] | ((uint32_t)p[1] << 8);
}

// One image of w x h pixels, NC samples of BPS bytes, strips of rps rows laid
// out after `head` bytes in the order `rev` says; `tail` bytes follow the
// last strip.  Every pixel is fetched as k_dwt_l1s does it.
template <int NC, int BPS>
static void run_layout(int w, int h, int rps, size_t head, size_t tail, bool rev, bool be, long &npull) {
    const uint64_t row_bytes = (uint64_t)w * NC * BPS;
    const int nstrips = (h + rps - 1) / rps;
    std::vector<uint64_t> off((size_t)nstrips);
    uint64_t pos = head;
    for (int k = 0; k < nstrips; k++) {
        const int s = rev ? nstrips - 1 - k : k;
        off[(size_t)s] = pos;
        pos += (uint64_t)std::min(rps, h - s * rps) * row_bytes;
    }
    const size_t nbytes = (size_t)pos + tail;
    uint8_t *src = (uint8_t *)std::malloc(nbytes);  // exactly the file: ASan guards both ends
    for (size_t i = 0; i < nbytes; i++) src[i] = (uint8_t)(i * 131 + (i >> 8) * 17 + 5);
    const uint64_t src_end = source_end(off.data(), rps, nstrips, 1, 0, h, row_bytes);
    CHECK(src_end == pos, "source_end %llu, strips end at %llu", (unsigned long long)src_end, (unsigned long long)pos);
    if (!px_fetch_usable(src_end)) {  // the kernel keeps the per-sample path
        std::free(src);
        return;
    }
    constexpr int LB = px_load_bytes(NC, BPS);
    for (int y = 0; y < h; y++) {
        const uint64_t ro = off[(size_t)(y / rps)] + (uint64_t)(y % rps) * row_bytes;
        const bool pull = row_needs_pullback(ro, row_bytes, NC, BPS, src_end);
        for (int x = 0; x < w; x++) {
            const uint64_t addr = ro + (uint64_t)x * NC * BPS;
            const int back = pull ? px_pullback(addr, LB, src_end) : 0;
            npull += back != 0;
            CHECK(addr >= (uint64_t)back && addr - back + LB <= nbytes && addr - back + LB <= src_end,
                  "access [%llu, +%d) outside [0, %zu) (w %d h %d rps %d)", (unsigned long long)(addr - back), LB,
                  nbytes, w, h, rps);
            uint32_t w0, w1;
            px_fetch<NC, BPS>(src, addr, pull, src_end, w0, w1);  // ASan: the access itself
            for (int c = 0; c < NC; c++) {
                const uint32_t got = BPS == 1 ? px_sample8(w0, c) : px_sample16(w0, w1, c, be);
                const uint32_t want = ref_sample(src + addr + (size_t)c * BPS, BPS, be);
                CHECK(got == want, "sample (%d, %d, %d): %u, want %u (NC %d BPS %d)", x, y, c, got, want, NC, BPS);
            }
        }
    }
    std::free(src);
}

template <int NC, int BPS>
static void run_format(long &npull) {
    static const int sizes[][2] = {{1, 1}, {1, 5}, {5, 1}, {17, 9}, {33, 64}, {48, 40}, {2, 2}, {3, 1}};
    for (const auto &sz : sizes) {
        const int w = sz[0], h = sz[1];
        for (int rps : {1, 4, 64, h}) {
            if (rps > h && rps != 64) continue;
            for (int be = 0; be < (BPS == 2 ? 2 : 1); be++) {
                // the file ends with the last row's last pixel (a TIFF whose
                // strips come last), with bytes behind it, with the strips in
                // reverse order, and with no header at all (a decoded image)
                run_layout<NC, BPS>(w, h, std::min(rps, h), 8 + 150, 0, false, be != 0, npull);
                run_layout<NC, BPS>(w, h, std::min(rps, h), 8 + 151, 3, false, be != 0, npull);
                run_layout<NC, BPS>(w, h, std::min(rps, h), 8, 0, true, be != 0, npull);
                run_layout<NC, BPS>(w, h, std::min(rps, h), 0, 0, false, be != 0, npull);
                run_layout<NC, BPS>(w, h, std::min(rps, h), 0, 1, true, be != 0, npull);
            }
        }
    }
}

// all byte / 16-bit values in every component slot, through the real fetch
template <int NC>
static void run_values() {
    constexpr int LB8 = px_load_bytes(NC, 1), LB16 = px_load_bytes(NC, 2);
    uint8_t buf[16 + 8];
    for (int c = 0; c < NC; c++) {
        for (uint32_t v = 0; v < 256; v++) {
            for (int i = 0; i < 24; i++) buf[i] = (uint8_t)(0xA5 ^ i);
            buf[8 + c] = (uint8_t)v;
            uint32_t w0, w1;
            px_load<LB8>(buf + 8, 0, w0, w1);
            CHECK(px_sample8(w0, c) == v, "u8 %u in slot %d -> %u", v, c, px_sample8(w0, c));
            // the over-read pixel: one byte back, shifted
            if (LB8 > NC) {
                px_load<LB8>(buf + 8, LB8 - NC, w0, w1);
                CHECK(px_sample8(w0, c) == v, "pulled-back u8 %u in slot %d -> %u", v, c, px_sample8(w0, c));
            }
            const float a = px_shift_f32(v, 128.0f), b = (float)((int32_t)v - 128);
            CHECK(std::memcmp(&a, &b, 4) == 0, "f32 level shift of %u differs", v);
        }
        for (int be = 0; be < 2; be++)
            for (uint32_t v = 0; v < 65536; v++) {
                for (int i = 0; i < 24; i++) buf[i] = (uint8_t)(0x5A ^ i);
                buf[8 + 2 * c] = (uint8_t)(be ? v >> 8 : v);
                buf[8 + 2 * c + 1] = (uint8_t)(be ? v : v >> 8);
                uint32_t w0, w1;
                px_load<LB16>(buf + 8, 0, w0, w1);
                CHECK(px_sample16(w0, w1, c, be != 0) == v, "u16 %u (be %d) in slot %d -> %u", v, be, c,
                      px_sample16(w0, w1, c, be != 0));
                if (LB16 > 2 * NC) {
                    px_load<LB16>(buf + 8, LB16 - 2 * NC, w0, w1);
                    CHECK(px_sample16(w0, w1, c, be != 0) == v, "pulled-back u16 %u (be %d) in slot %d", v, be, c);
                }
                const float a = px_shift_f32(v, 32768.0f), b = (float)((int32_t)v - 32768);
                CHECK(std::memcmp(&a, &b, 4) == 0, "f32 level shift of %u differs", v);
            }
    }
}

int main() {
    long npull = 0;
    run_format<1, 1>(npull);
    run_format<2, 1>(npull);
    run_format<3, 1>(npull);
    run_format<4, 1>(npull);
    run_format<1, 2>(npull);
    run_format<2, 2>(npull);
    run_format<3, 2>(npull);
    run_format<4, 2>(npull);
    CHECK(npull > 0, "no access was ever pulled back: the overrun case was not reached");
    run_values<1>();
    run_values<2>();
    run_values<3>();
    run_values<4>();
    // planar sources: source_end over the planes' strips
    {
        const uint64_t off[4] = {100, 140, 20, 60};  // plane 0: strips at 100, 140; plane 1: 20, 60
        CHECK(source_end(off, 4, 2, 2, 0, 7, 10) == 170, "planar source_end");
        CHECK(source_end(off, 4, 2, 2, 0, 4, 10) == 140, "planar source_end, first strip only");
        CHECK(source_end(off, 4, 2, 2, 4, 6, 10) == 160, "planar source_end, a band of the second strip");
    }
    if (g_fail) return 1;
    std::printf("DWT FETCH OK (%ld pulled-back accesses)\n", npull);
    return 0;
}
