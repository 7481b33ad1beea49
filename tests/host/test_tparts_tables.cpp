// Stand-alone CPU driver for the tile-part divisions' host side (csrc/t2.cpp
// tile_part_runs, t2_tables, tile_part_count, tile_parts_in, tile_part_order,
// tile_part_counts, tile_parts_fit over csrc/plan.cpp's geometry), built with AddressSanitizer /
// UBSan by tests/test_tparts.py.
//
// For a fixed list of geometries, every progression order (tile-parts per
// resolution too where the order allows them) and the letters 0, L, C, LC it
// checks what the device kernels rely on: each tile-part of the tables is a
// non-empty run [s0, s0 + ns) inside its tile's packets, a tile's runs follow
// each other and cover its packets, TPsot counts up and TNsot is the count on
// the last part only, every flagged index is constant inside a run and one of
// them changes between two runs; and the counts and the file order agree with
// the tables, for whole images and for split bands.
#include <cstdio>
#include <map>
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
    const char *name;
    int w, h, nc, levels, layers, tile, period;
};

static void check(const Geo &G, int order, int tpr, int letters) {
    jp2hip_recipe rc = {};
    rc.levels = G.levels;
    rc.layers = G.layers;
    rc.tile_w = rc.tile_h = G.tile;
    rc.cblk_w_log2 = rc.cblk_h_log2 = 6;
    rc.nprecincts = 2;
    rc.prec_w_log2[0] = rc.prec_h_log2[0] = 6;
    rc.prec_w_log2[1] = rc.prec_h_log2[1] = 5;
    rc.sop = rc.eph = rc.plt = 1;
    rc.guard_bits = 1;
    rc.reversible = 1;
    rc.flush_period = G.period;
    rc.progression = order;
    rc.tparts_r = tpr;
    Plan P;
    std::string err;
    char tag[128];
    std::snprintf(tag, sizeof tag, "%s order %d tparts_r %d letters %d", G.name, order, tpr, letters);
    if (!build_plan(P, rc, G.w, G.h, G.nc, 8, err)) {
        CHECK(false, "%s: refused: %s", tag, err.c_str());
        return;
    }
    const int L = rc.layers, ntiles = P.ntx * P.nty;
    std::vector<int> count;
    const bool fits = tile_part_counts(P, letters, count, err);
    bool over = false;
    for (int t = 0; t < ntiles; t++) over = over || tile_part_count(P, t, letters) > kMaxTileParts;
    CHECK(fits == !over, "%s: tile_part_counts says %d", tag, (int)fits);
    {
        T2Tables U;  // the same verdict from tables built for every tile
        std::string e2;
        t2_tables(P, 0, ntiles, 0, U, letters);
        CHECK(tile_parts_fit(P, U, e2) == fits && e2 == err, "%s: tile_parts_fit on the tables: %s", tag, e2.c_str());
    }
    if (!fits) {
        CHECK(err.find("tile ") != std::string::npos && err.find("ORGtparts=") != std::string::npos, "%s: message %s", tag,
              err.c_str());
        return;
    }
    T2Tables T;
    t2_tables(P, 0, ntiles, 0, T, letters);
    CHECK(T.letters == letters, "%s: the tables do not carry their letters", tag);
    const size_t npk = T.prec.size() * (size_t)L;
    CHECK((int64_t)T.tp.size() == tile_parts_in(P, 0, ntiles, letters), "%s: %zu tile-parts, tile_parts_in %lld", tag,
          T.tp.size(), (long long)tile_parts_in(P, 0, ntiles, letters));
    std::vector<uint16_t> order_tiles;
    tile_part_order(P, 0, ntiles, order_tiles, letters);
    CHECK(order_tiles.size() == T.tp.size(), "%s: tile_part_order names %zu tiles", tag, order_tiles.size());
    // per tile: base of its packets, and the runs in TPsot order
    std::vector<size_t> base((size_t)ntiles + 1, 0);
    std::vector<uint32_t> seq;
    for (int t = 0; t < ntiles; t++) {
        packet_sequence(P, t, seq);
        base[(size_t)t + 1] = base[(size_t)t] + seq.size();
    }
    CHECK(base[(size_t)ntiles] == npk, "%s: the tiles hold %zu packets of %zu", tag, base[(size_t)ntiles], npk);
    std::map<int, std::vector<const TpDesc *>> of;
    for (size_t i = 0; i < T.tp.size(); i++) {
        const TpDesc &tp = T.tp[i];
        if (i < order_tiles.size()) CHECK(order_tiles[i] == tp.tile, "%s: tile-part %zu: tile_part_order differs", tag, i);
        CHECK(tp.tile >= 0 && tp.tile < ntiles && tp.ns > 0, "%s: tile-part %zu: bad tile or empty", tag, i);
        if (tp.tile < 0 || tp.tile >= ntiles) continue;
        CHECK(tp.tpsot == (int)of[tp.tile].size(), "%s: tile-part %zu: TPsot %d", tag, i, tp.tpsot);
        CHECK((size_t)tp.s0 >= base[(size_t)tp.tile] && (size_t)tp.s0 + tp.ns <= base[(size_t)tp.tile + 1],
              "%s: tile-part %zu leaves its tile's packets", tag, i);
        of[tp.tile].push_back(&tp);
    }
    std::vector<uint32_t> first;
    for (int t = 0; t < ntiles; t++) {
        const std::vector<const TpDesc *> &tps = of[t];
        CHECK((int)tps.size() == tile_part_count(P, t, letters), "%s: tile %d: %zu parts, tile_part_count %d", tag, t,
              tps.size(), tile_part_count(P, t, letters));
        CHECK((int)tps.size() == tile_part_runs(P, t, letters, nullptr, first), "%s: tile %d: runs differ", tag, t);
        packet_sequence(P, t, seq);
        size_t at = base[(size_t)t];
        // (r, c) of the tile's precincts in storage order
        std::vector<int> r_of, c_of;
        for (int r = 0; r <= rc.levels; r++) {
            const Resolution &R0 = P.tiles[(size_t)t].tc[0].res[r];
            for (int i = 0; i < R0.npx * R0.npy; i++)
                for (int c = 0; c < P.nc; c++) {
                    r_of.push_back(r);
                    c_of.push_back(c);
                }
        }
        auto flagged = [&](size_t s, int f[3]) {
            const size_t k = seq[s - base[(size_t)t]];
            f[0] = tpr ? r_of[k / (size_t)L] : 0;
            f[1] = (letters & JP2HIP_TPARTS_L) ? (int)(k % (size_t)L) : 0;
            f[2] = (letters & JP2HIP_TPARTS_C) ? c_of[k / (size_t)L] : 0;
        };
        for (size_t i = 0; i < tps.size(); i++) {
            const TpDesc &tp = *tps[i];
            CHECK(tp.s0 == at, "%s: tile %d part %zu starts at %u, the one before ended at %zu", tag, t, i, tp.s0, at);
            CHECK(i < first.size() && first[i] == tp.s0 - base[(size_t)t], "%s: tile %d part %zu: not the run's start", tag, t, i);
            CHECK(tp.tnsot == (i + 1 == tps.size() ? (int)tps.size() : 0), "%s: tile %d part %zu: TNsot %d", tag, t, i, tp.tnsot);
            if (!T.seq.empty())
                for (size_t s = tp.s0; s < (size_t)tp.s0 + tp.ns && s < npk; s++) {
                    CHECK(T.seq[s] == base[(size_t)t] + seq[s - base[(size_t)t]], "%s: tile %d: the map differs at %zu", tag, t, s);
                    const size_t p = T.seq[s] / (size_t)L;
                    CHECK((int)p >= tp.prec0 && (int)p < tp.prec0 + tp.nprec, "%s: tile %d part %zu: precinct range", tag, t, i);
                }
            int f0[3], f1[3];
            flagged(tp.s0, f0);
            for (size_t s = tp.s0; s < (size_t)tp.s0 + tp.ns && s < base[(size_t)t + 1]; s++) {
                flagged(s, f1);
                CHECK(f0[0] == f1[0] && f0[1] == f1[1] && f0[2] == f1[2], "%s: tile %d part %zu: a flagged index changes inside", tag, t, i);
            }
            if (i) {
                flagged(tp.s0 - 1, f1);
                CHECK(f0[0] != f1[0] || f0[1] != f1[1] || f0[2] != f1[2], "%s: tile %d part %zu: no index changes at its start", tag, t, i);
            }
            at = (size_t)tp.s0 + tp.ns;
        }
        CHECK(at == base[(size_t)t + 1], "%s: tile %d: its parts end at %zu of %zu", tag, t, at, base[(size_t)t + 1]);
    }
    // split bands: whole flush stripes, their parts a contiguous run of the file's
    const std::vector<int> ends = flush_stripe_ends(P.nty, rc.tile_h, P.h, rc.flush_period);
    int ty0 = 0;
    for (int e : ends) {
        const int tile0 = ty0 * P.ntx, tile1 = e * P.ntx;
        T2Tables B;
        t2_tables(P, tile0, tile1, 0, B, letters);
        const int64_t f = tile_parts_in(P, 0, tile0, letters);
        CHECK((int64_t)B.tp.size() == tile_parts_in(P, tile0, tile1, letters), "%s: band %d: count", tag, ty0);
        for (size_t i = 0; i < B.tp.size() && (size_t)f + i < T.tp.size(); i++) {
            const TpDesc &a = B.tp[i], &b = T.tp[(size_t)f + i];
            CHECK(a.tile == b.tile && a.tpsot == b.tpsot && a.tnsot == b.tnsot && a.ns == b.ns &&
                      a.s0 + base[(size_t)tile0] == b.s0,
                  "%s: band %d: tile-part %zu differs from the file's", tag, ty0, i);
        }
        ty0 = e;
    }
}

int main() {
    static const Geo geos[] = {
        {"rgb 200x300 t128", 200, 300, 3, 3, 3, 128, 256},
        {"grey 150x130 t64", 150, 130, 1, 2, 2, 64, 0},
        {"rgba 101x77 t64", 101, 77, 4, 2, 4, 64, 128},
        {"rgb 300x300 t512", 300, 300, 3, 5, 6, 512, 1024},
        {"rgb 70x40 t32 deep", 70, 40, 3, 5, 2, 32, 64},   // tiles whose low resolutions are empty
        {"grey 64x64 one layer", 64, 64, 1, 3, 1, 64, 64}, // letters cut nowhere
    };
    int n = 0;
    for (const Geo &G : geos)
        for (int order = JP2HIP_ORDER_LRCP; order <= JP2HIP_ORDER_CPRL; order++)
            for (int tpr = 0; tpr < 2; tpr++) {
                if (tpr && order != JP2HIP_ORDER_RLCP && order != JP2HIP_ORDER_RPCL) continue;
                for (int letters : {0, JP2HIP_TPARTS_L, JP2HIP_TPARTS_C, JP2HIP_TPARTS_L | JP2HIP_TPARTS_C}) {
                    check(G, order, tpr, letters);
                    n++;
                }
            }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("TPARTS TABLES OK (%d cases)\n", n);
    return 0;
}
