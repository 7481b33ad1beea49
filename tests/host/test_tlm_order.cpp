// Stand-alone CPU driver for the TLM's host side (csrc/t2.cpp tile_part_count,
// tile_parts_in, tile_part_order, tlm_bytes, tlm_segments over csrc/plan.cpp's
// geometry), built with AddressSanitizer / UBSan by tests/test_tlm.py.
//
// For a fixed list of geometries, with a tile-part per resolution and with one
// per tile, with several -flush_period values, and for the whole image as well
// as for every band of tile rows a two- or three-rank split makes, it checks
// what the encodes rely on: tile_part_order names the tiles of T2Tables::tp
// in its order (the order the device leaves tp_len in); tile_parts_in counts
// them; a band's tile-parts are the contiguous run of the full order that
// starts after those of the tiles before it (where the split's ranks add their
// lengths); and tlm_segments writes exactly tlm_bytes bytes (the buffer is
// that long to the byte) in the layout of A.7.1.
#include <cstdio>
#include <string>
#include <vector>

#include "jp2hip_internal.h"

using namespace jp2hip;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");       \
            failures++;                       \
        }                                     \
    } while (0)

struct Geo {
    int w, h, nc, levels, tile_w, tile_h;
};

static void check_geometry(const Geo &g, int tparts_r, int flush_period) {
    jp2hip_recipe rc = {};
    rc.levels = g.levels;
    rc.layers = 2;
    rc.tile_w = g.tile_w;
    rc.tile_h = g.tile_h;
    rc.cblk_w_log2 = rc.cblk_h_log2 = 6;
    rc.progression = JP2HIP_ORDER_RPCL;
    rc.sop = rc.eph = rc.plt = 1;
    rc.tparts_r = tparts_r;
    rc.guard_bits = 1;
    rc.reversible = 1;
    rc.flush_period = flush_period;
    char name[128];
    std::snprintf(name, sizeof name, "%dx%dx%d L%d T%dx%d tparts_r %d flush %d", g.w, g.h, g.nc, g.levels, g.tile_w,
                  g.tile_h, tparts_r, flush_period);
    Plan P;
    std::string err;
    if (!build_plan(P, rc, g.w, g.h, g.nc, 8, err)) {
        CHECK(false, "%s: refused: %s", name, err.c_str());
        return;
    }
    const int ntiles = P.ntx * P.nty;
    T2Tables T;
    t2_tables(P, 0, ntiles, 0, T);
    std::vector<uint16_t> full;
    tile_part_order(P, 0, ntiles, full);
    CHECK(full.size() == T.tp.size(), "%s: %zu tile-parts in the order, %zu in the tables", name, full.size(), T.tp.size());
    CHECK((int64_t)T.tp.size() == tile_parts_in(P, 0, ntiles), "%s: tile_parts_in counts %lld of %zu", name,
          (long long)tile_parts_in(P, 0, ntiles), T.tp.size());
    for (size_t i = 0; i < full.size() && i < T.tp.size(); i++)
        CHECK(full[i] == T.tp[i].tile, "%s: entry %zu is tile %d, the tables' is %d", name, i, full[i], T.tp[i].tile);
    int64_t per_tile = 0;
    for (int t = 0; t < ntiles; t++) per_tile += tile_part_count(P, t);
    CHECK(per_tile == (int64_t)full.size(), "%s: the tiles' counts sum to %lld", name, (long long)per_tile);
    // the bands of a split: each a contiguous run of the full order
    for (int world = 2; world <= 3; world++)
        for (int rank = 0; rank < world; rank++) {
            int tr0, tr1;
            split_tile_rows(P.nty, rc.tile_h, P.h, rc.flush_period, rank, world, tr0, tr1);
            const int tile0 = tr0 * P.ntx, tile1 = tr1 * P.ntx;
            T2Tables B;
            t2_tables(P, tile0, tile1, 0, B);
            std::vector<uint16_t> band;
            tile_part_order(P, tile0, tile1, band);
            const int64_t first = tile_parts_in(P, 0, tile0);
            CHECK(band.size() == B.tp.size() && (int64_t)band.size() == tile_parts_in(P, tile0, tile1),
                  "%s: rank %d of %d: %zu tile-parts, the tables have %zu", name, rank, world, band.size(), B.tp.size());
            CHECK(first + (int64_t)band.size() <= (int64_t)full.size(), "%s: rank %d of %d: past the end", name, rank, world);
            for (size_t i = 0; i < band.size() && first + (int64_t)i < (int64_t)full.size(); i++)
                CHECK(band[i] == full[(size_t)first + i] && band[i] == B.tp[i].tile,
                      "%s: rank %d of %d: entry %zu is tile %d, the file's entry %lld is tile %d", name, rank, world, i,
                      band[i], (long long)(first + (int64_t)i), full[(size_t)first + i]);
        }
}

static void check_segments(int64_t n) {
    std::vector<uint16_t> tiles((size_t)n);
    std::vector<uint32_t> lens((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        tiles[(size_t)i] = (uint16_t)(i * 7919);
        lens[(size_t)i] = (uint32_t)(0xFFFFFFFFu - (uint32_t)i * 2654435761u);
    }
    const int64_t bytes = tlm_bytes(n);
    CHECK(bytes == (n ? 6 * n + 6 * ((n + kTlmSegEntries - 1) / kTlmSegEntries) : 0), "tlm_bytes(%lld)", (long long)n);
    std::vector<uint8_t> buf((size_t)bytes);  // exact: a byte more written is the sanitizer's
    tlm_segments(tiles.data(), lens.data(), n, buf.data());
    int64_t p = 0, i = 0;
    for (int z = 0; p < bytes; z++) {
        const int64_t k = (n - i < kTlmSegEntries) ? n - i : kTlmSegEntries;
        CHECK(buf[p] == 0xFF && buf[p + 1] == 0x55 && ((buf[p + 2] << 8) | buf[p + 3]) == 4 + 6 * k && buf[p + 4] == z &&
                  buf[p + 5] == 0x60,
              "n %lld: header of segment %d", (long long)n, z);
        p += 6;
        for (int64_t e = 0; e < k; e++, i++, p += 6) {
            const uint32_t t = ((uint32_t)buf[p] << 8) | buf[p + 1];
            const uint32_t len = ((uint32_t)buf[p + 2] << 24) | ((uint32_t)buf[p + 3] << 16) | ((uint32_t)buf[p + 4] << 8) |
                                 buf[p + 5];
            if (t != tiles[(size_t)i] || len != lens[(size_t)i]) {
                CHECK(false, "n %lld: entry %lld", (long long)n, (long long)i);
                return;
            }
        }
    }
    CHECK(p == bytes && i == n, "n %lld: %lld bytes, %lld entries read", (long long)n, (long long)p, (long long)i);
}

int main() {
    const Geo geos[] = {
        {700, 1100, 3, 6, 512, 512},   // the suites' first case: 2 x 3 tiles, two flush stripes at 1024
        {200, 150, 1, 2, 64, 64},      // 4 x 3 tiles
        {300, 200, 1, 6, 320, 256},    // one tile
        {130, 67, 2, 5, 64, 64},       // a last tile row of 3 samples: its low resolutions are empty
        {65, 260, 1, 6, 64, 64},       // a last tile column of 1 sample; five tile rows
        {840, 840, 1, 1, 8, 8},        // 11 025 tiles
        {100, 100, 1, 0, 32, 32},      // no decomposition: one resolution
    };
    int n = 0;
    for (const Geo &g : geos)
        for (int tpr = 0; tpr < 2; tpr++)
            for (int fp : {0, 64, 128, 1024}) {
                check_geometry(g, tpr, fp);
                n++;
            }
    for (int64_t k : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)10920, (int64_t)10921, (int64_t)10922, (int64_t)21842,
                      (int64_t)21843, kTlmMaxEntries})
        check_segments(k);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("TLM ORDER OK (%d geometries)\n", n);
    return 0;
}
