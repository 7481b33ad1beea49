// Stand-alone CPU driver for the progression-order tables (csrc/t2.cpp
// packet_sequence and t2_tables, over csrc/plan.cpp's geometry), built with
// AddressSanitizer / UBSan by tests/test_progression_orders.py.
//
// Reads cases from the file named on the command line, one per line:
//   width height components levels layers tile_w tile_h nprecincts pw.. ph..
// and, for each of the five orders (tile-parts per resolution too where the
// order allows them), checks what the device kernels rely on: every tile's
// sequence is a permutation of its packets; the forward map keeps each
// tile-part's packets inside the tile-part's own storage range; and a packet's
// place in its tile's sequence is nsop0 + layer * nsop_step (mod 65536).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
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

static void check_case(const std::string &line, jp2hip_recipe rc, int w, int h, int nc) {
    Plan P;
    std::string err;
    if (!build_plan(P, rc, w, h, nc, 8, err)) {
        CHECK(false, "%s: order %d tparts_r %d refused: %s", line.c_str(), rc.progression, rc.tparts_r, err.c_str());
        return;
    }
    const int L = rc.layers, ntiles = P.ntx * P.nty;
    T2Tables T;
    t2_tables(P, 0, ntiles, 0, T);
    const size_t npk = T.prec.size() * (size_t)L;
    CHECK((int64_t)npk == P.npackets, "%s: %zu packets in the tables, the plan counts %lld", line.c_str(), npk,
          (long long)P.npackets);
    if (rc.progression == JP2HIP_ORDER_RPCL) CHECK(T.seq.empty(), "%s: RPCL with a forward map", line.c_str());
    else CHECK(T.seq.size() == npk, "%s: forward map of %zu entries for %zu packets", line.c_str(), T.seq.size(), npk);
    // tile-parts: disjoint storage ranges that cover every packet; the map stays inside each
    std::vector<int> owner(npk, -1);
    for (size_t i = 0; i < T.tp.size(); i++) {
        const TpDesc &tp = T.tp[i];
        const size_t p0 = (size_t)tp.prec0 * L, p1 = (size_t)(tp.prec0 + tp.nprec) * L;
        CHECK(p1 <= npk, "%s: tile-part %zu ends past the packets", line.c_str(), i);
        std::vector<char> seen(p1 - p0, 0);
        for (size_t s = p0; s < p1 && s < npk; s++) {
            CHECK(owner[s] < 0, "%s: packet %zu in two tile-parts", line.c_str(), s);
            owner[s] = (int)i;
            const size_t k = T.seq.empty() ? s : T.seq[s];
            CHECK(k >= p0 && k < p1, "%s: tile-part %zu sends packet %zu of another", line.c_str(), i, k);
            if (k >= p0 && k < p1) {
                CHECK(!seen[k - p0], "%s: tile-part %zu sends packet %zu twice", line.c_str(), i, k);
                seen[k - p0] = 1;
            }
        }
    }
    for (size_t s = 0; s < npk; s++) CHECK(owner[s] >= 0, "%s: packet %zu in no tile-part", line.c_str(), s);
    // per tile: the exported sequence is the map's, and the SOP numbers follow it
    size_t base = 0;
    std::vector<uint32_t> seq;
    for (int t = 0; t < ntiles; t++) {
        packet_sequence(P, t, seq);
        for (size_t s = 0; s < seq.size(); s++) {
            const size_t k = seq[s];
            CHECK(k < seq.size(), "%s: tile %d: entry %zu out of range", line.c_str(), t, s);
            if (k >= seq.size()) continue;
            if (!T.seq.empty()) CHECK(T.seq[base + s] == base + k, "%s: tile %d: the map differs at %zu", line.c_str(), t, s);
            const PrecDesc &d = T.prec[(base + k) / L];
            const uint32_t ns = (uint32_t)(d.nsop0 + (int)(k % L) * (int)d.nsop_step) & 0xFFFFu;
            CHECK(ns == (s & 0xFFFFu), "%s: tile %d: packet %zu at place %zu has Nsop %u", line.c_str(), t, k, s, ns);
        }
        base += seq.size();
    }
    CHECK(base == npk, "%s: the tiles' sequences hold %zu packets of %zu", line.c_str(), base, npk);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    int ncases = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        int w, h, nc;
        jp2hip_recipe rc = {};
        if (!(ss >> w >> h >> nc >> rc.levels >> rc.layers >> rc.tile_w >> rc.tile_h >> rc.nprecincts)) continue;
        for (int i = 0; i < rc.nprecincts; i++) ss >> rc.prec_w_log2[i];
        for (int i = 0; i < rc.nprecincts; i++) ss >> rc.prec_h_log2[i];
        rc.cblk_w_log2 = rc.cblk_h_log2 = 6;
        rc.sop = rc.eph = rc.plt = 1;
        rc.guard_bits = 1;
        rc.reversible = 1;
        rc.flush_period = 128;
        for (int order = JP2HIP_ORDER_LRCP; order <= JP2HIP_ORDER_CPRL; order++)
            for (int tpr = 0; tpr < 2; tpr++) {
                if (tpr && order != JP2HIP_ORDER_RLCP && order != JP2HIP_ORDER_RPCL) continue;
                rc.progression = order;
                rc.tparts_r = tpr;
                check_case(line, rc, w, h, nc);
            }
        ncases++;
    }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("PACKET SEQUENCE OK (%d cases)\n", ncases);
    return 0;
}
