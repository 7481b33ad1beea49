// t2.cpp -- host side of code-stream assembly: the main header (SIZ, COD,
// QCD, COM), the tables that lay out packets and tile-parts for the device
// tier-2 (t2_device.hip), and the JP2 / JPX boxes around the code-stream
// (ISO/IEC 15444-1 Annex A, I; 15444-2 for 'jpx ').
//
// Structure produced for the Bucketeer recipe (KakaduConverter.java:38-44):
// RPCL packets, SOP before and EPH after every packet header, one tile-part
// per resolution (ORGtparts=R) each carrying a PLT marker (ORGgen_plt=yes),
// tile-parts in -flush_period stripe order, COM markers in Kakadu's layout.
// The layout is the one oracle/jp2_oracle.c writes (write_codestream).
// The other progression orders (LRCP, RLCP, PCRL, CPRL) keep the packets and
// their storage; packet_sequence says in which order a tile sends them, and
// t2_tables turns that into the device's forward map and SOP numbers.  A
// tile-part is a run of that sequence: tile_part_runs cuts it where the
// resolution (R), the layer (L) or the component (C) changes, whichever of
// ORGtparts' letters are set (jp2hip_set_tile_part_divisions for L and C).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>

#include "jp2hip_internal.h"

namespace jp2hip {

namespace {

inline void be16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; }
inline void be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

}  // namespace

// COM markers in Kakadu's layout (test.jpx): a
// version string, then "Kdu-Layer-Info", one fixed-width line per layer --
// log2 of the layer's slope threshold (squared error of samples normalised to
// unit range, summed over the image, per byte; -192.0 = every pass) and the
// code-stream bytes through that layer (oracle: write_main_header).
static constexpr char kComVersion[] = "jp2hip-v0.2.0";
static constexpr char kLayerHdr[] = "Kdu-Layer-Info: log_2{Delta-D(squared-error)/Delta-L(bytes)}, L(bytes)\n";

static double layer_log_slope(uint64_t K, int bits) {
    if (K == 0) return -192.0;
    if (K >= 0x7FF0000000000000ull) return 192.0;  // nothing included
    double s;
    std::memcpy(&s, &K, 8);
    const double v = std::log2(s) - 2.0 * bits;
    return v < -192.0 ? -192.0 : (v > 192.0 ? 192.0 : v);
}

void main_header(const Plan &P, std::vector<uint8_t> &v, const uint64_t *K, const int64_t *layer_end) {
    const jp2hip_recipe &rc = P.rc;
    const int L = rc.levels, nc = P.nc;
    v.clear();
    auto u8 = [&](int x) { v.push_back((uint8_t)x); };
    auto u16 = [&](int x) { u8(x >> 8); u8(x); };
    auto u32 = [&](uint32_t x) { u16((int)(x >> 16)); u16((int)(x & 0xFFFF)); };
    auto raw = [&](const char *p, size_t n) { v.insert(v.end(), p, p + n); };
    u16(0xFF4F);
    u16(0xFF51);  // SIZ
    u16(38 + 3 * nc);
    u16(0);
    u32((uint32_t)P.w); u32((uint32_t)P.h);
    u32(0); u32(0);
    u32((uint32_t)rc.tile_w); u32((uint32_t)rc.tile_h);
    u32(0); u32(0);
    u16(nc);
    for (int c = 0; c < nc; c++) { u8(P.bits - 1); u8(1); u8(1); }
    u16(0xFF52);  // COD
    u16(12 + L + 1);
    u8(0x01 | (rc.sop ? 2 : 0) | (rc.eph ? 4 : 0));
    u8(rc.progression);
    u16(rc.layers);
    u8((rc.mct && nc >= 3) ? 1 : 0);
    u8(L);
    u8(rc.cblk_w_log2 - 2);
    u8(rc.cblk_h_log2 - 2);
    u8(0);
    u8(rc.reversible ? 1 : 0);
    for (int r = 0; r <= L; r++) u8((prec_log2(rc, r, true) << 4) | prec_log2(rc, r, false));
    u16(0xFF5C);  // QCD
    const int nbands = 3 * L + 1;
    u16(3 + (rc.reversible ? nbands : 2 * nbands));
    u8((rc.guard_bits << 5) | (rc.reversible ? 0 : 2));
    for (int i = 0; i < nbands; i++) {
        const int d = (i == 0) ? L : L - (i - 1) / 3;
        const int band = (i == 0) ? 0 : 1 + (i - 1) % 3;
        const BandQuant q = band_quant(rc, P.bits, d, band);
        if (rc.reversible) u8(q.eps << 3);
        else u16((q.eps << 11) | q.mu);
    }
    if (rc.comment) {
        const size_t nv = sizeof kComVersion - 1, nh = sizeof kLayerHdr - 1;
        u16(0xFF64);
        u16(4 + (int)nv);
        u16(1);  // Rcom: Latin-1 text
        raw(kComVersion, nv);
        u16(0xFF64);
        u16(4 + (int)nh + 17 * rc.layers);
        u16(1);
        raw(kLayerHdr, nh);
        for (int l = 0; l < rc.layers; l++) {
            char line[64];
            const int n = std::snprintf(line, sizeof line, "%6.1f, %8.1e\n", K ? layer_log_slope(K[l], P.bits) : 0.0,
                                        layer_end ? (double)layer_end[l] : 0.0);
            if (n != 17) {  // never for |slope| <= 192 and < 1e100 bytes
                std::memset(line, ' ', 16);
                line[16] = '\n';
            }
            raw(line, 17);
        }
    }
}

static int64_t tree_nodes(int w, int h) {
    int64_t n = 0;
    for (;;) {
        n += (int64_t)w * h;
        if (w == 1 && h == 1) return n;
        w = (w + 1) / 2;
        h = (h + 1) / 2;
    }
}

void packet_sequence(const Plan &P, int t, std::vector<uint32_t> &seq) {
    const jp2hip_recipe &rc = P.rc;
    const int Lv = rc.levels, L = rc.layers, order = rc.progression;
    const Tile &Tl = P.tiles[(size_t)t];
    // the tile's precincts in storage order, each with what the orders sort
    // by: resolution, component, raster index in the resolution's precinct
    // grid, and its position on the reference grid (B.12.1.3-5 with no
    // subsampling: the precinct's corner, or the tile's where that lies
    // before it)
    struct Prec {
        int32_t r, c, raster;
        int64_t x, y;
        uint32_t p;
    };
    std::vector<Prec> pv;
    for (int r = 0; r <= Lv; r++) {
        const Resolution &R0 = Tl.tc[0].res[r];
        if (R0.npx * R0.npy == 0) continue;
        const int sh = Lv - r, ppx = prec_log2(rc, r, false), ppy = prec_log2(rc, r, true);
        const int64_t px0 = ((int64_t)Tl.tx0 >> sh) >> ppx, py0 = ((int64_t)Tl.ty0 >> sh) >> ppy;
        for (int py = 0; py < R0.npy; py++)
            for (int px = 0; px < R0.npx; px++)
                for (int c = 0; c < P.nc; c++) {
                    Prec e;
                    e.r = r;
                    e.c = c;
                    e.raster = py * R0.npx + px;
                    e.x = std::max<int64_t>(Tl.tx0, (px0 + px) << (ppx + sh));
                    e.y = std::max<int64_t>(Tl.ty0, (py0 + py) << (ppy + sh));
                    e.p = (uint32_t)pv.size();
                    pv.push_back(e);
                }
    }
    seq.clear();
    seq.reserve(pv.size() * (size_t)L);
    if (order == JP2HIP_ORDER_LRCP || order == JP2HIP_ORDER_RLCP) {
        // (r, c, raster) is the order inside a layer of both; storage order
        // is (r, raster, c)
        std::stable_sort(pv.begin(), pv.end(), [](const Prec &a, const Prec &b) {
            return a.r != b.r ? a.r < b.r : (a.c != b.c ? a.c < b.c : a.raster < b.raster);
        });
        if (order == JP2HIP_ORDER_LRCP) {
            for (int l = 0; l < L; l++)
                for (const Prec &e : pv) seq.push_back(e.p * (uint32_t)L + (uint32_t)l);
        } else {
            for (size_t i = 0; i < pv.size();) {
                size_t j = i;
                while (j < pv.size() && pv[j].r == pv[i].r) j++;
                for (int l = 0; l < L; l++)
                    for (size_t k = i; k < j; k++) seq.push_back(pv[k].p * (uint32_t)L + (uint32_t)l);
                i = j;
            }
        }
        return;
    }
    if (order == JP2HIP_ORDER_PCRL)
        std::stable_sort(pv.begin(), pv.end(), [](const Prec &a, const Prec &b) {
            return a.y != b.y ? a.y < b.y : (a.x != b.x ? a.x < b.x : (a.c != b.c ? a.c < b.c : a.r < b.r));
        });
    else if (order == JP2HIP_ORDER_CPRL)
        std::stable_sort(pv.begin(), pv.end(), [](const Prec &a, const Prec &b) {
            return a.c != b.c ? a.c < b.c : (a.y != b.y ? a.y < b.y : (a.x != b.x ? a.x < b.x : a.r < b.r));
        });
    // (RPCL: storage order)
    for (const Prec &e : pv)
        for (int l = 0; l < L; l++) seq.push_back(e.p * (uint32_t)L + (uint32_t)l);
}

int tile_part_runs(const Plan &P, int t, int letters, const std::vector<uint32_t> *seq, std::vector<uint32_t> &first) {
    const jp2hip_recipe &rc = P.rc;
    const int L = rc.layers;
    const bool byR = rc.tparts_r != 0, byL = (letters & JP2HIP_TPARTS_L) != 0, byC = (letters & JP2HIP_TPARTS_C) != 0;
    first.assign(1, 0u);
    if (!byR && !byL && !byC) return 1;
    // resolution and component of the tile's precincts, in storage order
    const Tile &Tl = P.tiles[(size_t)t];
    std::vector<uint16_t> rc_of;  // r << 8 | c
    for (int r = 0; r <= rc.levels; r++) {
        const Resolution &R0 = Tl.tc[0].res[r];
        for (int i = 0; i < R0.npx * R0.npy; i++)
            for (int c = 0; c < P.nc; c++) rc_of.push_back((uint16_t)((r << 8) | c));
    }
    std::vector<uint32_t> own;
    if (!seq && rc.progression != JP2HIP_ORDER_RPCL) {
        packet_sequence(P, t, own);
        seq = &own;
    }
    const size_t n = rc_of.size() * (size_t)L;
    const uint16_t keep = (uint16_t)((byR ? 0xFF00 : 0) | (byC ? 0x00FF : 0));
    uint32_t prev = 0;
    for (size_t s = 0; s < n; s++) {
        const size_t k = seq ? (*seq)[s] : s;
        // the flagged indices of packet k as one word
        const uint32_t flagged = (uint32_t)(rc_of[k / (size_t)L] & keep) | (byL ? (uint32_t)(k % (size_t)L) << 16 : 0u);
        if (s && flagged != prev) first.push_back((uint32_t)s);
        prev = flagged;
    }
    return (int)first.size();
}

static std::string division_letters(const Plan &P, int letters) {
    std::string s;
    if (P.rc.tparts_r) s += 'R';
    if (letters & JP2HIP_TPARTS_L) s += 'L';
    if (letters & JP2HIP_TPARTS_C) s += 'C';
    return s;
}

static bool too_many(const Plan &P, int t, int n, int letters, std::string &err) {
    if (n <= kMaxTileParts) return false;
    err = "tile " + std::to_string(t) + ": " + std::to_string(n) + " tile-parts with ORGtparts=" +
          division_letters(P, letters) + " (TNsot holds at most " + std::to_string(kMaxTileParts) + ")";
    return true;
}

bool tile_part_counts(const Plan &P, int letters, std::vector<int> &count, std::string &err) {
    count.assign((size_t)(P.ntx * P.nty), 0);
    for (int t = 0; t < P.ntx * P.nty; t++) {
        count[(size_t)t] = tile_part_count(P, t, letters);
        if (too_many(P, t, count[(size_t)t], letters, err)) return false;
    }
    return true;
}

bool tile_parts_fit(const Plan &P, const T2Tables &T, std::string &err) {
    // a tile's count stands on its last part; the first such tile in tile order is named
    const TpDesc *worst = nullptr;
    for (const TpDesc &tp : T.tp)
        if (tp.tnsot > kMaxTileParts && (!worst || tp.tile < worst->tile)) worst = &tp;
    return !worst || !too_many(P, worst->tile, worst->tnsot, T.letters, err);
}

// File order of the tile-parts of tiles [tile0, tile1), whose counts are
// count[t - tile0]: per -flush_period stripe, part 0 of every tile of the
// stripe in tile order, then part 1, ... (test.jpx); emit(t, k) for each.
template <typename F>
static void file_order(const Plan &P, int tile0, int tile1, const std::vector<int> &count, F emit) {
    const std::vector<int> ends = flush_stripe_ends(P.nty, P.rc.tile_h, P.h, P.rc.flush_period);
    int ty0 = 0;
    for (int e : ends) {
        const int a = std::max(tile0, ty0 * P.ntx), b = std::min(tile1, e * P.ntx);
        int most = 0;
        for (int t = a; t < b; t++) most = std::max(most, count[(size_t)(t - tile0)]);
        for (int k = 0; k < most; k++)
            for (int t = a; t < b; t++)
                if (k < count[(size_t)(t - tile0)]) emit(t, k);
        ty0 = e;
    }
}

void t2_tables(const Plan &P, int tile0, int tile1, int block0, T2Tables &T, int letters) {
    const jp2hip_recipe &rc = P.rc;
    const int Lv = rc.levels, L = rc.layers;
    const bool resequence = rc.progression != JP2HIP_ORDER_RPCL;
    std::vector<uint32_t> tseq, pos, first;
    T.prec.clear();
    T.tp.clear();
    T.seq.clear();
    T.tt_nodes = 0;
    T.max_prec_blocks = 0;
    T.letters = letters;
    // tile-parts per tile, in tile order first
    std::vector<std::vector<TpDesc>> per_tile((size_t)std::max(0, tile1 - tile0));
    std::vector<int> count(per_tile.size(), 0);
    for (int t = tile0; t < tile1; t++) {
        const Tile &Tl = P.tiles[t];
        int nsop = 0;
        const size_t tile_prec0 = T.prec.size();
        for (int r = 0; r <= Lv; r++) {
            const Resolution &R0 = Tl.tc[0].res[r];
            for (int py = 0; py < R0.npy; py++)
                for (int px = 0; px < R0.npx; px++)
                    for (int c = 0; c < P.nc; c++) {
                        const Precinct &pr = Tl.tc[c].res[r].prec[(size_t)py * R0.npx + px];
                        PrecDesc d;
                        std::memset(&d, 0, sizeof d);
                        d.nb = (uint8_t)pr.nb;
                        d.tt_off = (int32_t)T.tt_nodes;
                        d.nsop0 = nsop;
                        d.nsop_step = 1;
                        int blocks = 0;
                        for (int bi = 0; bi < pr.nb; bi++) {
                            const PrecBand &pb = pr.pb[bi];
                            d.first[bi] = pb.first - block0;
                            d.ncw[bi] = (uint16_t)pb.ncw;
                            d.nch[bi] = (uint16_t)pb.nch;
                            blocks += pb.ncw * pb.nch;
                            if (pb.ncw && pb.nch) T.tt_nodes += 2 * tree_nodes(pb.ncw, pb.nch);
                        }
                        T.max_prec_blocks = std::max(T.max_prec_blocks, blocks);
                        T.prec.push_back(d);
                        nsop += L;
                    }
        }
        const uint32_t base = (uint32_t)(tile_prec0 * (size_t)L);
        const uint32_t npk = (uint32_t)((T.prec.size() - tile_prec0) * (size_t)L);
        if (resequence) {
            // another order: the tile's sequence, and each packet's place in
            // it as its Nsop -- nsop0 for layer 0, then nsop_step a layer: 1
            // where layers are innermost, else the packets of one layer of
            // the resolution (RLCP) or of the tile (LRCP)
            packet_sequence(P, t, tseq);
            pos.resize(tseq.size());
            for (size_t s = 0; s < tseq.size(); s++) pos[tseq[s]] = (uint32_t)s;
            for (size_t i = tile_prec0; i < T.prec.size(); i++) {
                const size_t k = (i - tile_prec0) * (size_t)L;
                T.prec[i].nsop0 = (int32_t)pos[k];
                T.prec[i].nsop_step = L > 1 ? (uint16_t)(pos[k + 1] - pos[k]) : 1;
            }
            for (uint32_t s : tseq) T.seq.push_back(base + s);
        }
        // its tile-parts: the runs its divisions cut the sequence into
        if (!npk) continue;
        const int ntp = tile_part_runs(P, t, letters, resequence ? &tseq : nullptr, first);
        std::vector<TpDesc> &tps = per_tile[(size_t)(t - tile0)];
        for (int i = 0; i < ntp; i++) {
            const uint32_t s0 = first[(size_t)i], s1 = i + 1 < ntp ? first[(size_t)i + 1] : npk;
            uint32_t lo = UINT32_MAX, hi = 0;  // the precincts the run's packets come from
            for (uint32_t s = s0; s < s1; s++) {
                const uint32_t p = (resequence ? tseq[s] : s) / (uint32_t)L;
                lo = std::min(lo, p);
                hi = std::max(hi, p);
            }
            TpDesc tp;
            tp.tile = t;
            tp.tpsot = i;
            tp.tnsot = i == ntp - 1 ? ntp : 0;
            tp.prec0 = (int32_t)(tile_prec0 + lo);
            tp.nprec = (int32_t)(hi - lo + 1);
            tp.s0 = base + s0;
            tp.ns = s1 - s0;
            tps.push_back(tp);
        }
        count[(size_t)(t - tile0)] = ntp;
    }
    file_order(P, tile0, tile1, count, [&](int t, int k) { T.tp.push_back(per_tile[(size_t)(t - tile0)][(size_t)k]); });
}

// ---- tile-part counts and order without the tables; TLM marker segments
// (A.7.1; jp2hip_set_organisation) ----

int tile_part_count(const Plan &P, int t, int letters) {
    const Tile &Tl = P.tiles[(size_t)t];
    bool any = false;
    for (int r = 0; r <= P.rc.levels && !any; r++) any = Tl.tc[0].res[r].npx * Tl.tc[0].res[r].npy != 0;
    if (!any) return 0;
    std::vector<uint32_t> first;
    return tile_part_runs(P, t, letters, nullptr, first);
}

int64_t tile_parts_in(const Plan &P, int tile0, int tile1, int letters) {
    int64_t n = 0;
    for (int t = tile0; t < tile1; t++) n += tile_part_count(P, t, letters);
    return n;
}

void tile_part_order(const Plan &P, int tile0, int tile1, std::vector<uint16_t> &tiles, int letters) {
    tiles.clear();
    std::vector<int> count((size_t)std::max(0, tile1 - tile0));
    for (int t = tile0; t < tile1; t++) count[(size_t)(t - tile0)] = tile_part_count(P, t, letters);
    file_order(P, tile0, tile1, count, [&](int t, int) { tiles.push_back((uint16_t)t); });
}

int64_t tile_part_division_bytes(const Plan &P, int letters, int64_t ntp) {
    if (!letters) return 0;
    return (14 + (P.rc.plt ? 5 : 0)) * (ntp - tile_parts_in(P, 0, P.ntx * P.nty, 0));
}

int64_t tlm_bytes(int64_t ntp) {
    return ntp > 0 ? 6 * ntp + 6 * ((ntp + kTlmSegEntries - 1) / kTlmSegEntries) : 0;
}

void tlm_segments(const uint16_t *tiles, const uint32_t *lengths, int64_t n, uint8_t *dst) {
    for (int64_t i0 = 0, z = 0; i0 < n; i0 += kTlmSegEntries, z++) {
        const int64_t k = std::min<int64_t>(kTlmSegEntries, n - i0);
        dst[0] = 0xFF; dst[1] = 0x55;
        be16(dst + 2, (uint32_t)(4 + 6 * k));
        dst[4] = (uint8_t)z;
        dst[5] = 0x60;  // Stlm: ST = 2 (16-bit Ttlm), SP = 1 (32-bit Ptlm)
        dst += 6;
        for (int64_t i = i0; i < i0 + k; i++, dst += 6) {
            be16(dst, tiles[i]);
            be32(dst + 2, lengths[i]);
        }
    }
}

// ---- the boxes in front of the code-stream ----
// What the source states about its pixels goes into jp2h (DESIGN.md "Source
// metadata"): its ICC profile into colr, its ExtraSamples into cdef, its
// resolution into res.  A source that states nothing (SourceMeta all zero)
// gets the header the oracle writes (write_file_header there).

SourceMeta source_meta(const jp2hip_layout &lay) {
    SourceMeta m;
    m.extra_samples = lay.extra_samples;
    m.res_unit = lay.res_unit;
    m.xres_num = lay.xres_num; m.xres_den = lay.xres_den;
    m.yres_num = lay.yres_num; m.yres_den = lay.yres_den;
    if (lay.icc && lay.icc_bytes) { m.icc = lay.icc; m.icc_bytes = lay.icc_bytes; }
    return m;
}

namespace {

inline uint32_t rd32(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
inline bool sig_is(const uint8_t *p, const char *s) { return std::memcmp(p, s, 4) == 0; }

// a profile this long would not leave jp2h's 32-bit box length room for the rest
constexpr uint64_t kMaxIccBytes = 0xFFFFFFFFull - 1024;

struct Resc {
    uint32_t n = 0, d = 0;
    int e = 0;
};

// One axis of the capture resolution in points per metre, as resc stores it
// (N / D * 10^E, N and D 16 bits).  The value is the exact ratio P / Q; when
// the reduced P and Q fit they are stored as they are, else D = 1 and N is
// the value rounded (half up) to the most digits 16 bits hold: 6553.5 <=
// v / 10^E < 65535.5, a relative error of at most 0.5 / 6553.5.  (E stays
// within -13..9 for 32-bit rationals, far inside resc's int8.)
bool resc_axis(uint32_t num, uint32_t den, int unit, Resc &r) {
    if (!num || !den || (unit != 2 && unit != 3)) return false;
    uint64_t P = (uint64_t)num * (unit == 2 ? 10000 : 100), Q = (uint64_t)den * (unit == 2 ? 254 : 1);
    const uint64_t g = std::gcd(P, Q);
    P /= g;
    Q /= g;
    if (P <= 65535 && Q <= 65535) {
        r.n = (uint32_t)P; r.d = (uint32_t)Q; r.e = 0;
        return true;
    }
    typedef unsigned __int128 u128;
    for (int E = -20; E <= 20; E++) {  // the smallest E whose N fits: the one of the rule above
        u128 A = P, B = Q;             // A / B = v / 10^E
        for (int k = 0; k < (E < 0 ? -E : E); k++) (E < 0 ? A : B) *= 10;
        const u128 N = (2 * A + B) / (2 * B);
        if (N > 65535) continue;
        if (N < 6554) return false;  // (not reached: E - 1 gave N > 65535)
        r.n = (uint32_t)N; r.d = 1; r.e = E;
        return true;
    }
    return false;
}

// Which boxes jp2h holds for this image and source, and its length.
struct HeaderBoxes {
    bool enum_colr = true;   // the 15-byte enumerated colr box
    int meth = 0;            // 2 / 3: a colr box with the profile follows; 0: none
    uint32_t icc_len = 0;
    int cdef_typ = -1;       // Typ of the last channel; -1: no cdef box
    bool res = false;
    Resc v, h;
    uint32_t jp2h = 0;
};

HeaderBoxes header_boxes(const Plan &P, const SourceMeta &m) {
    HeaderBoxes b;
    const int nc = P.nc;
    uint32_t embed = 0;
    const int cls = classify_icc(m.icc, m.icc_bytes, nc, &embed);
    if (cls == 1) {
        b.enum_colr = false;
        b.meth = 2;
    } else if (cls == 2 && P.rc.format == JP2HIP_FORMAT_JPX) {
        b.meth = 3;  // after the enumerated box: a JP2 reader uses the first colr
    }
    b.icc_len = b.meth ? embed : 0;
    if (nc == 4 || nc == 2) {
        // ExtraSamples + 1: 1 unspecified (the channel is not opacity: no
        // cdef), 2 associated = premultiplied opacity, 3 unassociated; 0 (or
        // anything else): not stated, the last channel is opacity
        b.cdef_typ = m.extra_samples == 1 ? -1 : (m.extra_samples == 2 ? 2 : 1);
    }
    b.res = resc_axis(m.yres_num, m.yres_den, m.res_unit, b.v) && resc_axis(m.xres_num, m.xres_den, m.res_unit, b.h);
    b.jp2h = 8 + (8 + 14) + (b.enum_colr ? 8 + 7 : 0) + (b.meth ? 8 + 3 + b.icc_len : 0) +
             (b.cdef_typ >= 0 ? (uint32_t)(8 + 2 + 6 * nc) : 0) + (b.res ? 8 + (8 + 10) : 0);
    return b;
}

}  // namespace

int classify_icc(const uint8_t *icc, uint64_t n, int nc, uint32_t *embed) {
    *embed = 0;
    if (!icc || n < 132) return 0;
    const uint64_t S = rd32(icc);  // the profile's own size: what is embedded
    if (S < 132 || S > n || S > kMaxIccBytes) return 0;
    if (!sig_is(icc + 36, "acsp")) return 0;
    const bool rgb = nc >= 3;
    if (!sig_is(icc + 16, rgb ? "RGB " : "GRAY")) return 0;
    *embed = (uint32_t)S;
    // restricted (15444-1 I.5.3.3 METH 2): a matrix / TRC input profile; display
    // class counts too -- the working spaces masters carry (sRGB, Adobe RGB,
    // eciRGB, ProPhoto) are mntr matrix / TRC profiles and JP2 readers take them
    if (!sig_is(icc + 12, "scnr") && !sig_is(icc + 12, "mntr")) return 2;
    if (!sig_is(icc + 20, "XYZ ")) return 2;
    const uint64_t ntags = rd32(icc + 128);
    if (132 + 12 * ntags > S) return 2;
    static const char *const kRgbTags[] = {"rXYZ", "gXYZ", "bXYZ", "rTRC", "gTRC", "bTRC"};
    static const char *const kGrayTags[] = {"kTRC"};
    const char *const *need = rgb ? kRgbTags : kGrayTags;
    const int nneed = rgb ? 6 : 1;
    unsigned have = 0;
    for (uint64_t i = 0; i < ntags; i++) {
        const uint8_t *t = icc + 132 + 12 * i;
        if (sig_is(t, "A2B0")) return 2;
        for (int k = 0; k < nneed; k++)
            if (sig_is(t, need[k])) have |= 1u << k;
    }
    return have == (1u << nneed) - 1 ? 1 : 2;
}

size_t file_header_bytes(const Plan &P, const SourceMeta &meta) {
    if (P.rc.format == JP2HIP_FORMAT_J2K) return 0;
    size_t n = 12;                                                                    // signature
    n += (P.rc.format == JP2HIP_FORMAT_JPX) ? (8 + 4 + 4 + 12) + (8 + 10) : (8 + 4 + 4 + 4);  // ftyp (+rreq)
    n += header_boxes(P, meta).jp2h;
    return n + 8;                                                                     // jp2c box header
}

void write_file_header(const Plan &P, const SourceMeta &meta, uint64_t cs_bytes, uint8_t *dst) {
    if (P.rc.format == JP2HIP_FORMAT_J2K) return;
    uint8_t *p = dst;
    auto raw = [&](const void *s, size_t n) { std::memcpy(p, s, n); p += n; };
    auto u8 = [&](int x) { *p++ = (uint8_t)x; };
    auto u16 = [&](int x) { be16(p, (uint32_t)x); p += 2; };
    auto u32 = [&](uint32_t x) { be32(p, x); p += 4; };
    auto box = [&](uint32_t len, const char *type) { u32(len); raw(type, 4); };
    static const uint8_t sig[12] = {0, 0, 0, 12, 'j', 'P', ' ', ' ', 0x0D, 0x0A, 0x87, 0x0A};
    raw(sig, 12);
    const int nc = P.nc;
    if (P.rc.format == JP2HIP_FORMAT_JPX) {
        box(8 + 4 + 4 + 12, "ftyp");
        raw("jpx ", 4); u32(0);
        raw("jpx ", 4); raw("jp2 ", 4); raw("jpxb", 4);
        box(8 + 10, "rreq");  // reader requirements: feature 5 (JP2-compatible)
        u8(1); u8(0x80); u8(0x80);
        u16(1); u16(5); u8(0x80);
        u16(0);
    } else {
        box(8 + 4 + 4 + 4, "ftyp");
        raw("jp2 ", 4); u32(0); raw("jp2 ", 4);
    }
    const HeaderBoxes hb = header_boxes(P, meta);
    box(hb.jp2h, "jp2h");
    box(8 + 14, "ihdr");
    u32((uint32_t)P.h); u32((uint32_t)P.w);
    u16(nc); u8(P.bits - 1); u8(7); u8(0); u8(0);
    if (hb.enum_colr) {
        box(8 + 7, "colr");
        u8(1); u8(0); u8(0);
        u32(nc >= 3 ? 16 : 17);  // sRGB / greyscale
    }
    if (hb.meth) {
        box(8 + 3 + hb.icc_len, "colr");
        u8(hb.meth);
        u8(hb.meth == 3 ? 1 : 0);  // PREC: above the enumerated box's 0
        u8(hb.meth == 3 ? 1 : 0);  // APPROX (JPX): accurate
        raw(meta.icc, hb.icc_len);
    }
    if (hb.cdef_typ >= 0) {
        box((uint32_t)(8 + 2 + 6 * nc), "cdef");
        u16(nc);
        for (int c = 0; c < nc; c++) {
            const bool alpha = (c == nc - 1);
            u16(c); u16(alpha ? hb.cdef_typ : 0); u16(alpha ? 0 : c + 1);
        }
    }
    if (hb.res) {
        box(8 + (8 + 10), "res ");
        box(8 + 10, "resc");  // capture resolution; vertical first
        u16((int)hb.v.n); u16((int)hb.v.d); u16((int)hb.h.n); u16((int)hb.h.d);
        u8(hb.v.e); u8(hb.h.e);
    }
    // a code-stream past 4 GiB: length 0 = "to the end of the file" (last box)
    box(8 + cs_bytes > 0xFFFFFFFFull ? 0u : (uint32_t)(8 + cs_bytes), "jp2c");
}

}  // namespace jp2hip
