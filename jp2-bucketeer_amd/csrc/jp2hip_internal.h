// jp2hip_internal.h -- host-side model of one encode (geometry, quantiser,
// code-block table) shared by the HIP launch code (the .hip stage files), tier-2
// (t2.cpp) and the encodes behind the C ABI (encode.cpp).  Where the source's samples lie (TIFF
// parser, strip / tile grid, band bounds) is source_layout.h, not here.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "jp2hip.h"

namespace jp2hip {

constexpr int kMaxPasses = 96;    // 3*32-2 rounded up; per-block pass table stride
// slope prediction (front.hip k_plane_*, oracle predict_and_code): 1/8-octave
// bins of the double slope's bit pattern covering 2^-64 .. 2^64, and the
// margin (bins) kept below the predicted rate-target bin
constexpr int kSlopeBins = 1024;
constexpr int kSlopeBinBase = (1023 - 64) << 3;
constexpr int kSkipMargin = 12;
// PCRD threshold selection (pcrd.hip k_hull / k_select): hull segment bytes
// histogrammed over 1/32-octave bins of the slope key (bits 47..62 of the
// IEEE double, 2^-64 .. 2^64, clamped at both ends); the exact threshold is
// then resolved inside the one bin where a layer's budget falls
constexpr int kPcrdBins = 4096;
constexpr int kPcrdBinBase = (1023 - 64) << 5;
constexpr int kMaxLayers = 32;
constexpr int kMaxLevels = 12;

// Per-band quantiser (Annex E).  For the reversible path eps follows the
// 5/3 BIBO-gain rule that reproduces test.jpx's QCD.
struct BandQuant {
    int eps = 0, mu = 0, Mb = 0;
    float inv_delta = 1.0f;
    double wnorm = 1.0;  // Delta^2 * synthesis energy gain
};

BandQuant band_quant(const jp2hip_recipe &rc, int bits, int level, int band);

// Every band's deadzone quantiser as the DWT's final writes apply it
// (dwt.hip): the coefficient plane holds quantisation indices in
// sign-magnitude, 16-bit when every band has at most 15 magnitude bit-planes
// (8-bit sources), else 32-bit; k_quant reads them.  Entry [d][b] = level d,
// band b (the LL band only at d = levels; levels = 0: [0][0]).
struct QuantTab {
    float inv[kMaxLevels + 1][4];    // 1 / Delta (1 for the reversible path)
    uint32_t lim[kMaxLevels + 1][4]; // 2^Mb - 1: the largest index
    int q16;
};
QuantTab quant_tab(const jp2hip_recipe &rc, int bits);

// One code-block, as the kernels see it (uploaded as-is).
// device error word bit: the decision-stream pool was too small for the
// coded planes (emit_t1_items); the host grows it and encodes again
constexpr int kErrSlotPool = 8;

struct BlockDesc {
    int32_t tc;         // tile-component plane index
    int16_t x0, y0;     // top-left inside the tile-component plane (Mallat layout)
    int16_t w, h;       // <= 64
    int8_t band;        // 0 LL, 1 HL, 2 LH, 3 HH
    int8_t Mb;          // magnitude bit-planes of the band
    int8_t pad0, pad1;
    float inv_delta;    // irreversible quantiser reciprocal
    uint32_t pad2;
    uint64_t bp_off;    // bit-plane storage offset, in uint64 words: (Mb+1)*64 column masks
                        // (front.hip k_quant)
    uint64_t sm_off;    // sign-magnitude storage offset, in int32 words
    uint64_t out_off;   // tier-1 output offset, bytes
    uint32_t out_cap;   // tier-1 output capacity, bytes
    uint32_t pad3;
};
static_assert(sizeof(BlockDesc) == 56, "BlockDesc layout");

struct PrecBand {
    int ncw = 0, nch = 0;
    int first = 0;  // index of the first block (raster order, contiguous)
};
struct Precinct {
    PrecBand pb[3];
    int nb = 0;
};
struct Resolution {
    int npx = 0, npy = 0;
    std::vector<Precinct> prec;
};
struct TileComp {
    Resolution res[kMaxLevels + 1];
};
struct Tile {
    int tx0, ty0, tx1, ty1;
    std::vector<TileComp> tc;
};

struct Plan {
    jp2hip_recipe rc;
    int w = 0, h = 0, nc = 0, bits = 0;
    int ntx = 0, nty = 0, ntc = 0;
    int plane_w = 0, plane_h = 0;           // tile-component plane stride / rows
    std::vector<Tile> tiles;
    std::vector<BlockDesc> blocks;
    std::vector<double> weight;             // PCRD weight per block
    std::vector<int32_t> t1_order;          // lane -> block mapping for tier-1
    std::vector<int32_t> tc_w, tc_h;        // tile-component sizes
    uint64_t bp_words = 0, sm_words = 0, out_bytes = 0;
    int64_t npackets = 0, ntileparts = 0;
    double compw[4] = {1, 1, 1, 1};
    // tile-split band (make_subplan): the device part covers tiles
    // [tile0, tile0 + ntc/nc) = image rows [row0, row0 + band_h); its blocks
    // are the full plan's blocks [block0, block0 + blocks.size())
    int row0 = 0, band_h = 0, tile0 = 0, block0 = 0;
    // first block of each tile of this plan (tiles in raster order; blocks
    // are emitted tile by tile), ntiles + 1 entries
    std::vector<int32_t> tile_b0;
    // rate-control groups: block ranges [grp_b0[g], grp_b0[g + 1]) whose
    // layer thresholds are chosen together.  Lossless ("-rate -"): one group
    // per -flush_period stripe (each stripe's layers from its own tier-1
    // bytes, oracle lossless_budget); rate-driven: the whole image, one group
    std::vector<int32_t> grp_b0;
    int ngroups() const { return (int)grp_b0.size() - 1; }
    // one group whatever the recipe: a lossless recipe encoded by per-layer
    // rates (jp2hip_set_layer_rates), whose byte targets are the whole image's
    bool one_group = false;
    // identity of this plan's contents (build_plan / make_subplan): a device
    // context that already holds the tables of generation `gen` skips
    // uploading them again
    uint64_t gen = 0;
};

bool build_plan(Plan &plan, const jp2hip_recipe &rc, int w, int h, int nc, int bits,
                std::string &err, bool one_group = false);
// The largest tile side: BlockDesc::x0 / y0 are 16 bits, and a
// tile-component plane of at most 2^30 elements is indexed with an int.
constexpr int kMaxTileSide = 32768;
// What rc.tile_w / tile_h mean for a w x h image, resolved before build_plan
// by everything that takes a caller's recipe: 0 and 0 become one tile for the
// whole image, the smallest multiples of 2^levels not below w and h (written
// to SIZ as they are); one of them 0, or a negative one, is refused.
bool resolve_tiles(jp2hip_recipe &rc, int w, int h, std::string &err);
inline bool untiled(const jp2hip_recipe *rc) { return rc && rc->tile_w == 0 && rc->tile_h == 0; }

int prec_log2(const jp2hip_recipe &rc, int r, bool vertical);

// Lossless layer l of NL: the fraction (1/65536 units) of its stripe's
// tier-1 bytes the layer's threshold fits (oracle/jp2_oracle.c
// lossless_layer_frac, fitted to test.jpx's Kdu-Layer-Info); the last layer
// takes every pass (65536).
int32_t lossless_layer_frac(int l, int NL);

// Tile rows grouped the way "-flush_period P" flushes them
// (KakaduConverter.java:40; oracle flush_stripes): a stripe ends once the rows
// pushed reach the next multiple of P, and at the last tile row.  Returns one
// past the last tile row of each stripe.  P <= 0: one stripe per tile row.
std::vector<int> flush_stripe_ends(int nty, int tile_h, int h, int period);
// Tile rows [tr0, tr1) of rank `rank` out of `world`: contiguous runs of
// whole flush stripes, so each rank's tile-parts are contiguous in the file.
void split_tile_rows(int nty, int tile_h, int h, int period, int rank, int world, int &tr0, int &tr1);
// The device part of `full` for tile rows [tr0, tr1): same blocks, offsets
// rebased to the band (tier-2 keeps using `full` and global block indices).
void make_subplan(const Plan &full, int tr0, int tr1, Plan &sub);

// --------------------------------------------------------------------------
// Device tier-2 (t2_device.hip).  The host lays out, once per encode, the precincts
// of the tiles being coded in storage order (tile, resolution, py, px,
// component: the RPCL packet order) and the tile-parts in code-stream order
// (-flush_period stripes); the kernels code every packet header, size the
// tile-parts and write the code-stream in HBM.  Packet k of precinct p is
// stored as packet p * L + k in every progression order: the order moves only
// where a packet lies in its tile-part (T2Tables::seq), its Nsop and its place
// in the PLT, never its bytes.
// --------------------------------------------------------------------------
struct PrecDesc {
    int32_t first[3];        // first code-block (encode-local index) of each precinct-band
    uint16_t ncw[3], nch[3]; // code-block grid of each precinct-band
    int32_t tt_off;          // tag-tree node scratch: (inclusion, zero bit-planes) per band
    int32_t nsop0;           // SOP sequence number of the precinct's first packet in its tile
    uint8_t nb, pad0;
    // Nsop of the layer-l packet = nsop0 + l * nsop_step (mod 65536, so the
    // step's low 16 bits are all that count): 1 where layers are innermost
    // (RPCL, PCRL, CPRL), the resolution's packets per layer in RLCP, the
    // tile's in LRCP
    uint16_t nsop_step;
};
static_assert(sizeof(PrecDesc) == 36, "PrecDesc layout");
// A tile-part: a run of its tile's packet sequence (tile_part_runs).
struct TpDesc {
    int32_t tile, tpsot, tnsot;  // SOT fields (Isot, TPsot, TNsot)
    // the precincts (PrecDesc table) its packets come from, first to last in
    // storage order -- host side only; without the L and C divisions the
    // tile-parts' ranges are disjoint and hold exactly their packets
    int32_t prec0, nprec;
    // what the kernels walk: its packets are the places [s0, s0 + ns) of the
    // forward map T2Tables::seq (no map, RPCL: the packets stored there)
    uint32_t s0, ns;
};
static_assert(sizeof(TpDesc) == 28, "TpDesc layout");
struct T2Tables {
    std::vector<PrecDesc> prec;
    std::vector<TpDesc> tp;   // code-stream order
    // Forward map of the progression order: the packets of the tables' i-th
    // tile lie at [b, b + n) in storage and in this map alike (n its packet
    // count), and the s-th packet the tile sends is packet seq[b + s]; a
    // tile-part takes a run of those places.  Empty = identity (RPCL: storage
    // order is sequence order).
    std::vector<uint32_t> seq;
    int64_t tt_nodes = 0;
    int max_prec_blocks = 0;  // code-blocks of the largest precinct
    int letters = 0;          // the L / C divisions the tile-parts were cut with
};
// Tables for tiles [tile0, tile1) of `P` (blocks rebased by -block0: a
// tile-split rank's blocks are its sub-plan's).
// `letters`: JP2HIP_TPARTS_L | _C (jp2hip_set_tile_part_divisions); the
// caller checks the tile-part counts (tile_parts_fit, tile_part_counts)
// before the tables reach the device: TNsot is stored as it comes.
void t2_tables(const Plan &P, int tile0, int tile1, int block0, T2Tables &T, int letters = 0);
// Tile t's packets in the order rc.progression sends them (B.12.1; no
// component is subsampled): each entry the packet's storage index within the
// tile, p * L + l for the tile's p-th precinct in (resolution, py, px,
// component) order.  RPCL gives the identity.  A tile-part per resolution
// (RLCP, RPCL) takes its packets as a contiguous run of this sequence.
void packet_sequence(const Plan &P, int t, std::vector<uint32_t> &seq);
// TLM marker segments (A.7.1, jp2hip_set_organisation): an entry per
// tile-part in file order (the order of T2Tables::tp), at most kTlmSegEntries
// to a segment (Ltlm is 16 bits: 4 + 6 * 10921 = 65530), Ztlm up to 255.
constexpr int kTlmSegEntries = 10921;
constexpr int64_t kTlmMaxEntries = (int64_t)256 * kTlmSegEntries;
constexpr int64_t kTlmSegBytes = 6 + 6 * (int64_t)kTlmSegEntries;  // a full segment
// The segments' byte count for ntp tile-parts: 6 an entry, 6 a segment.
int64_t tlm_bytes(int64_t ntp);
// Writes them (tlm_bytes(n) bytes) on the host: the split's rank 0, and
// jp2hip_tlm_segments; the single-GPU encode writes the same bytes on the
// device (t2_device.hip k_t2_tlm).
void tlm_segments(const uint16_t *tiles, const uint32_t *lengths, int64_t n, uint8_t *dst);
// Tile t's tile-parts as runs of its packet sequence (ORGtparts): the
// divisions are R (rc.tparts_r) plus `letters` (JP2HIP_TPARTS_L | _C), and a
// tile-part starts at place 0 and before every place whose packet differs
// from the one before it in a flagged index -- resolution for R, layer for L,
// component for C.  `first` receives the places the parts start at; returns
// their count.  seq: the tile's packet_sequence when the caller has it (else
// it is built here; RPCL needs none).  The only place that knows the rule:
// t2_tables, the counts below and jp2hip_tile_parts all come here.
int tile_part_runs(const Plan &P, int t, int letters, const std::vector<uint32_t> *seq, std::vector<uint32_t> &first);
// TNsot is 8 bits: false, with a message that names the tile, its count and
// the letters, when a tile's divisions give more than 255 tile-parts -- from
// the counts of every tile of P (count[t]; a split's ranks, jp2hip_tile_parts),
// or from tables already built for all of them (the single encode).
constexpr int kMaxTileParts = 255;
bool tile_part_counts(const Plan &P, int letters, std::vector<int> &count, std::string &err);
bool tile_parts_fit(const Plan &P, const T2Tables &T, std::string &err);
// Tile-parts of tile t, of tiles [tile0, tile1), and the tile of each of
// their tile-parts in file order -- T2Tables::tp's order and count without
// the precinct tables: per -flush_period stripe, part 0 of every tile of the
// stripe, then part 1, ... (a tile with fewer parts drops out).
// (Plan::ntileparts is the rate loop's header estimate: it counts a tile-part
// per resolution whatever the divisions are.)
int tile_part_count(const Plan &P, int t, int letters = 0);
int64_t tile_parts_in(const Plan &P, int tile0, int tile1, int letters = 0);
void tile_part_order(const Plan &P, int tile0, int tile1, std::vector<uint16_t> &tiles, int letters = 0);
// The bytes the L / C divisions add to a code-stream whose PLTs are one
// segment each: SOT + SOD (14) and a PLT header (5, with plt) per tile-part
// they add; ntp: the image's tile-parts with the letters.  A rate-driven
// encode with letters is the encode without them whose target is this much
// lower (jp2hip.h).
int64_t tile_part_division_bytes(const Plan &P, int letters, int64_t ntp);
// What the host reads back after a tier-2 sizing pass (one D2H per pass).
struct T2Summary {
    int64_t part_bytes;               // tile-parts of the tiles coded (SOT .. last packet)
    int64_t tp_hdr_bytes;             // SOT + PLT + SOD of those tile-parts
    int64_t layer_bytes[kMaxLayers];  // packet bytes per layer
    uint64_t kc[kMaxLayers];          // Kdu-Layer-Info slope keys (select() only)
    int64_t t1_bytes, coded_passes;   // tier-1 totals (every coded pass)
    int64_t decisions;                // MQ-coded decisions
    int32_t skipped, err;             // slope prediction skipped planes; tier-1 overflow
    int64_t stream_need;              // decision-stream pool bytes the coded planes took
};
// Rate control of a rate-driven encode, run on the device (pcrd.hip rate_loop,
// device_common.h rate_step; the oracle's loop in oracle_encode): iteration `it` selects
// with `budget`, sizes the code-stream, stops when it fits `target` (or after
// 8 iterations), else lowers the budget.  `halt` stops the remaining
// iterations' kernels; `safety` = slope prediction's safety net fired
// (planes were skipped yet every coded byte fits: the host re-runs the front
// with every plane coded).
struct RateState {
    int64_t budget, target, fixed, skip_target, cs_bytes;
    int32_t it, halt, safety, iters;
};
// Rate control by per-layer rates (jp2hip_set_layer_rates): one
// step of the loop after iteration `it`'s tier-2 sizing pass, the text the
// device (rate_step_layers, device_common.h), the tile-split's host loop and
// jp2hip_layer_rate_step all run.  target[l] < 0: the layer has no target (a
// lossless top layer; its budget is kRateNoBudget and stays).  The
// code-stream through layer l is S[l] = fixed + part_bytes - sum over m > l
// of layer_bytes[m].  Returns 1 (halt: every targeted layer fits, or it == 7;
// the budgets stay), else 0 with the budgets of the layers that are over
// lowered -- the single-rate step, per layer -- floored at 0 and clamped so
// that they never decrease with l.
#if defined(__HIP__) || defined(__HIPCC__)
#define JP2HIP_RATE_HD __host__ __device__
#else
#define JP2HIP_RATE_HD
#endif
constexpr int64_t kRateNoBudget = INT64_MAX;
JP2HIP_RATE_HD inline int layer_rate_step(int L, int it, int64_t fixed, int64_t part_bytes,
                                          const int64_t *layer_bytes, const int64_t *target, int64_t *budget) {
    bool fits = true;
    int64_t S = fixed + part_bytes;
    for (int l = L - 1; l >= 0; l--) {
        if (target[l] >= 0 && S > target[l]) fits = false;
        S -= layer_bytes[l];
    }
    if (fits || it >= 7) return 1;
    S = fixed + part_bytes;
    for (int l = L - 1; l >= 0; l--) {
        if (target[l] >= 0 && S > target[l]) {
            // exponential back-off + 1/16 of the overshoot + 64 B, as the oracle
            const int64_t over = S - target[l];
            budget[l] -= (over << it) + (over >> 4) + 64;
            if (budget[l] < 0) budget[l] = 0;
        }
        S -= layer_bytes[l];
    }
    for (int l = L - 2; l >= 0; l--)
        if (budget[l] > budget[l + 1]) budget[l] = budget[l + 1];
    return 0;
}
// The targets and first budgets of `L` rates for a w x h image (P's tile-part
// and packet counts are the header estimate's; org = T + E, what the TLM and
// the tile-part divisions take from every layer); a last rate of 0 under
// rate_bpp <= 0 is the lossless top layer: no target, kRateNoBudget.
void layer_rate_targets(const Plan &P, const double *rates, int L, int64_t org, int64_t *target, int64_t *budget);

// Main header (SOC .. COM) for the Kdu-Layer-Info values (nullptr: zeros;
// the length does not depend on them).
void main_header(const Plan &P, std::vector<uint8_t> &v, const uint64_t *K, const int64_t *layer_end);

// What the source file states about its pixels (jp2hip_layout's metadata
// fields): it differs from file to file, so it is passed per encode and is
// never part of a cached Plan.  `icc` is the caller's host memory.
struct SourceMeta {
    int32_t extra_samples = 0, res_unit = 0;
    uint32_t xres_num = 0, xres_den = 0, yres_num = 0, yres_den = 0;
    const uint8_t *icc = nullptr;
    uint64_t icc_bytes = 0;
};
SourceMeta source_meta(const jp2hip_layout &lay);

// An ICC profile for an image of `nc` channels: 0 unusable, 1 restricted
// (matrix / TRC input or display profile: JP2 METH 2), 2 any other usable
// profile (JPX METH 3); *embed = the bytes to embed (the profile's own size).
int classify_icc(const uint8_t *icc, uint64_t n, int nc, uint32_t *embed);

// JP2 / JPX boxes in front of the code-stream (0 bytes for raw J2K); only
// plan.rc.format, w, h, nc and bits are read.
size_t file_header_bytes(const Plan &plan, const SourceMeta &meta);
void write_file_header(const Plan &plan, const SourceMeta &meta, uint64_t cs_bytes, uint8_t *dst);

}  // namespace jp2hip
