// front.hip -- the front of an encode on the GPU: stand-alone ingest, the
// quantiser, slope prediction, and GpuEncoder::run_front, which enqueues every
// stage up to the PCRD hulls.
//
// Stage map of libjp2hip (reference stage: kdu_compress
// invoked at KakaduConverter.java:61-71):
//   unpack.hip, lzw.hip  S1a  compressed TIFF strips / tiles -> an
//                             uncompressed staging copy in HBM
//   dwt.hip       S1-S3  TIFF strips in HBM -> level shift, RCT (int) / ICT
//                        (fp32) fused into DWT level 1; LDS-staged levels
//   k_ingest      S1+S2  stand-alone ingest, used only when levels == 0
//   k_quant       S4     deadzone quantiser + bit-plane masks via wave ballot
//   k_plane_*     S4b    slope prediction (rate-driven encodes)
//   t1.hip        S5     EBCOT tier-1: context modelling + MQ coder
//   pcrd.hip      S6     PCRD-opt convex hulls + slope thresholds per layer
//   t2_device.hip S7/S8  tier-2 and the code-stream, written in HBM and
//                        copied to the host by a DMA engine
//
// Floating point: built with -ffp-contract=off; every 9/7 / ICT expression is
// written in the same order as the oracle so the lossy path is bit-exact.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_common.h"
#include "dwt_fetch.h"
#include "gpu_encoder.h"
#include "hip_check.h"
#include "stage_repeat.h"

namespace jp2hip {

// --------------------------------------------------------------------------
// S1 + S2: ingest
// --------------------------------------------------------------------------
struct IngestArgs {
    const uint8_t *src;
    const uint64_t *strip_off;
    int rps, w, h, nc, bits, planar, big_endian, mct, reversible;
    int ntx, tile_w, tile_h, plane_w, plane_h, spp_strips;  // strips per plane
    int row0;  // image row of local row 0 (tile-split bands)
    void *coef;
    float inv;     // no decomposition: the one band's quantiser (QuantTab [0][0])
    uint32_t lim;
    int q16;
};

__device__ __forceinline__ int32_t read_sample(const IngestArgs &a, int x, int y, int c) {
    int strip = y / a.rps;
    size_t off;
    if (a.planar == 2) {
        off = a.strip_off[(size_t)c * a.spp_strips + strip] +
              ((size_t)(y - strip * a.rps) * a.w + x) * (a.bits >> 3);
    } else {
        off = a.strip_off[strip] + (((size_t)(y - strip * a.rps) * a.w + x) * a.nc + c) * (a.bits >> 3);
    }
    if (a.bits == 8) return (int32_t)a.src[off];
    uint32_t b0 = a.src[off], b1 = a.src[off + 1];
    return (int32_t)(a.big_endian ? ((b0 << 8) | b1) : (b0 | (b1 << 8)));
}

__global__ void __launch_bounds__(256) k_ingest(IngestArgs a) {
    int x = blockIdx.x * 64 + (threadIdx.x & 63);
    int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.w || y >= a.h) return;
    int32_t off = 1 << (a.bits - 1);
    int32_t s[4];
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] = (c < a.nc) ? read_sample(a, x, a.row0 + y, c) - off : 0;
    int tx = x / a.tile_w, ty = y / a.tile_h;
    size_t plane = (size_t)a.plane_w * a.plane_h;
    size_t base = ((size_t)(ty * a.ntx + tx) * a.nc) * plane + (size_t)(y - ty * a.tile_h) * a.plane_w +
                  (x - tx * a.tile_w);
    bool domct = a.mct && a.nc >= 3;
    // the samples are the final coefficients: quantisation indices, as the
    // DWT writes them (dwt.hip)
    auto put = [&](int c, uint32_t q) {
        if (a.q16) ((uint16_t *)a.coef)[base + (size_t)c * plane] = (uint16_t)q;
        else ((uint32_t *)a.coef)[base + (size_t)c * plane] = q;
    };
    if (a.reversible) {
        int32_t v[4] = {s[0], s[1], s[2], s[3]};
        if (domct) {
            v[0] = (s[0] + 2 * s[1] + s[2]) >> 2;
            v[1] = s[2] - s[1];
            v[2] = s[0] - s[1];
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c < a.nc) put(c, quant_sm<true>(v[c], a.inv, a.lim, a.q16 ? 15 : 31));
    } else {
        float f[4] = {(float)s[0], (float)s[1], (float)s[2], (float)s[3]};
        if (domct) {
            float R = f[0], G = f[1], B = f[2];
            float y0 = 0.299f * R; y0 = y0 + 0.587f * G; y0 = y0 + 0.114f * B;
            float cb = -0.16875f * R; cb = cb - 0.33126f * G; cb = cb + 0.5f * B;
            float cr = 0.5f * R; cr = cr - 0.41869f * G; cr = cr - 0.08131f * B;
            f[0] = y0; f[1] = cb; f[2] = cr;
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c < a.nc) put(c, quant_sm<false>(__float_as_int(f[c]), a.inv, a.lim, a.q16 ? 15 : 31));
    }
}

// --------------------------------------------------------------------------
// S4: quantisation + bit-planes.  One wavefront per code-block; lane = column.
// Layout per block (uint64 words, lane c = column c, bit y = row y): B[p][64]
// for p < Mb, then sign[64].  (S[p] = OR_{q>=p} B[q], the significance state
// after plane p, is not stored: k_t1_cm3 walks the planes top-down and builds
// it as it goes.)
// --------------------------------------------------------------------------
constexpr int kZeroSpans = 9;
struct QuantArgs {
    const BlockDesc *blocks;
    const void *coef;
    int plane_w, plane_h, reversible;
    uint64_t *bp;
    int32_t *sm;
    uint8_t *P;
    int64_t *dref, *dsig;  // [block][32]
    uint32_t *est;         // [block][32] predicted coded size of plane p, 1/16 bit
    int max_mb;            // largest Mb of the plan (LDS: max_mb * 512 bytes per wave)
    int keep_sm;           // write the sign-magnitude copy of every block (debug dumps)
    int nblocks;
    // per-encode counters of later kernels, zeroed here (no memset launch):
    // dword spans, spread over the workgroups
    uint32_t *zero[kZeroSpans];
    uint32_t nzero[kZeroSpans];
};

constexpr int kQuantWaves = 2;  // code-blocks (waves) per workgroup

// The bit-plane masks of a column whose magnitudes fit BITS (8 or 16) bits,
// by a bit-matrix transpose in registers; its cost does not depend on the
// number of planes.  Word i of W packs rows i, i + NW, ... (32 / BITS fields
// of BITS bits, NW = ROWS * BITS / 32 words).  log2(BITS) rounds of masked
// swaps between words i and i + s exchange bit s of the word index with bit s
// of the bit position; then word b (and, with 64 rows, word BITS + b) holds
// plane b: field k, bit i of word b + BITS * j = row i + BITS * j + NW * k.
// Two v_perm_b32 order the fields by row.
template <int ROWS, int BITS>
__device__ __forceinline__ void quant_transpose(uint32_t (&W)[ROWS * BITS / 32], int P, uint64_t valid, uint64_t *planes,
                                                uint64_t *BT, int lane) {
    constexpr int NW = ROWS * BITS / 32;
    static_assert((BITS == 8 || BITS == 16) && (ROWS == 32 || ROWS == 64) && NW >= BITS, "quant_transpose");
#pragma unroll
    for (int s = 1; s < BITS; s <<= 1) {
        const uint32_t m = s == 1 ? 0x55555555u : s == 2 ? 0x33333333u : s == 4 ? 0x0F0F0F0Fu : 0x00FF00FFu;
#pragma unroll
        for (int i = 0; i < NW; i++) {
            if (i & s) continue;
            const uint32_t x = W[i], y = W[i + s];
            W[i] = (x & m) | ((y << s) & ~m);
            W[i + s] = ((x >> s) & m) | (y & ~m);
        }
    }
#pragma unroll
    for (int b = 0; b < BITS; b++) {
        if (b >= P) break;
        uint32_t lo = W[b], hi = 0;
        if constexpr (ROWS == 64) {
            // fields of word b: rows 0.., 2 BITS..; of word BITS + b: rows BITS.., 3 BITS..
            constexpr uint32_t sel_lo = BITS == 8 ? 0x05010400u : 0x05040100u;
            constexpr uint32_t sel_hi = BITS == 8 ? 0x07030602u : 0x07060302u;
            lo = __builtin_amdgcn_perm(W[BITS + b], W[b], sel_lo);
            hi = __builtin_amdgcn_perm(W[BITS + b], W[b], sel_hi);
        }
        const uint64_t m = (((uint64_t)hi << 32) | lo) & valid;
        planes[b * 64 + lane] = m;
        BT[(size_t)b * 64 + lane] = m;
    }
}

// What the two front halves below share once the column's magnitudes are
// OR-ed into vor and its signs are in sgcol: the block's number of magnitude
// bits (uniform: P and the plane loop stay scalar) and the sign column.
// Column masks (lane c, bit y = row y): BT[p][c] = bit p of the column, then
// the sign column SGT[c] -- the layout the tier-1 context modelling reads
// (t1.hip k_t1_cm3)
__device__ __forceinline__ int quant_planes_and_signs(const QuantArgs &a, const BlockDesc &d, int b, int lane, uint32_t vor,
                                                      uint64_t sgcol, uint64_t *BT) {
    vor = wave_or_u32(vor);  // a DPP reduction
    const int P = __builtin_amdgcn_readfirstlane(vor ? 32 - __clz(vor) : 0);
    if (lane == 0) a.P[b] = (uint8_t)P;
    uint64_t *SGT = BT + (size_t)d.Mb * 64;
    SGT[lane] = sgcol;
    return P;
}

// The front half of k_quant for a block of at most ROWS rows (64 or 32): the
// column load, the sign / magnitude split, the bit-plane masks (to LDS, for
// the distortion sums, and to HBM) and the sign column.  Returns the block's
// number of magnitude bits.  The coefficient plane holds the quantisation
// indices the DWT wrote, sign-magnitude.
//
// The lane's column stays in registers for the bit-plane passes: the indices
// are read from HBM once, all ROWS row loads in flight at once; rows past
// the block end re-read its last row and lanes past its width read column 0
// -- values of the block, so its magnitude bits are unchanged -- and are
// cleared from the masks (`valid`), not row by row.  The sign bit is taken as
// stored: a -0.0 quantises to 0, and a zero's sign is never coded.
//
// 16-bit index plane (QuantTab::q16): rows i and i + ROWS / 2 share a word from
// the start, which is the packing of the 16-bit transpose and one v_perm_b32
// away from that of the 8-bit one.
template <int ROWS>
__device__ __forceinline__ int quant_columns16(const QuantArgs &a, const BlockDesc &d, int b, int lane, bool act, bool keep_sm,
                                               uint64_t valid, int32_t *sm, uint64_t *planes) {
    static_assert(ROWS == 64 || ROWS == 32, "quant_columns16: 64 or 32 rows");
    constexpr int H = ROWS / 2;
    const size_t e0 = (size_t)d.tc * a.plane_w * a.plane_h + (size_t)d.y0 * a.plane_w + d.x0;
    const uint16_t *src = (const uint16_t *)a.coef + e0;
    const int cl = act ? lane : 0;
    const int hm1 = d.h - 1;
    uint32_t W[H];
#pragma unroll
    for (int i = 0; i < H; i++) {
        // the two rows as the elements of a 2 x 16-bit vector: packed as they
        // arrive, so the column never takes a register per row
        typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
        u16x2 w;
        w.x = src[(size_t)min(i, hm1) * a.plane_w + cl];
        w.y = src[(size_t)min(i + H, hm1) * a.plane_w + cl];
        W[i] = __builtin_bit_cast(uint32_t, w);
    }
    // The sign bits, 15 and 31 of every word, two ops a word: word i < 16
    // shifted right by 15 - i drops them at bits i and 16 + i of s0; word i
    // >= 16 shifted by 31 - i at bits i - 16 and i of s1.  So the low halves
    // of (s0, s1) are the signs of rows 0..31 and the high halves those of
    // rows H.. .  The magnitudes keep their sign bits for now.
    uint32_t s0 = 0, s1 = 0, vor = 0;
#pragma unroll
    for (int i = 0; i < H; i++) {
        if (i < 16) s0 |= (W[i] >> (15 - i)) & (0x00010001u << i);
        else s1 |= (W[i] >> (31 - i)) & (0x00010001u << (i - 16));
        vor |= W[i];
    }
    uint64_t sgcol = s0;  // 32 rows: bits i and 16 + i are rows i and H + i
    if constexpr (ROWS == 64)
        sgcol = ((uint64_t)__builtin_amdgcn_perm(s1, s0, 0x07060302u) << 32) | __builtin_amdgcn_perm(s1, s0, 0x05040100u);
    sgcol &= valid;
    uint64_t *BT = a.bp + d.bp_off;
    const int P = quant_planes_and_signs(a, d, b, lane, (vor | (vor >> 16)) & 0x7FFFu, sgcol, BT);
    if (keep_sm) {  // debug dumps only (Mb <= 15 here): the rows read again, not held in registers for this
        for (int y = 0; y < d.h; y++) {
            const uint32_t raw = src[(size_t)y * a.plane_w + cl];
            sm[y * 64] = act ? (int32_t)((raw & 0x7FFFu) | (raw >> 15) << 31) : 0;
        }
    }
    if (P > 8) {
#pragma unroll
        for (int i = 0; i < H; i++) W[i] &= 0x7FFF7FFFu;
        quant_transpose<ROWS, 16>(W, P, valid, planes, BT, lane);
    } else if (P > 0) {
        // bytes of rows i, i + Q, i + 2Q, i + 3Q (Q = ROWS / 4) from the words
        // of rows (i, i + 2Q) and (i + Q, i + 3Q): the low bytes of their
        // halves, which leaves the sign bits behind
        constexpr int Q = ROWS / 4;
        uint32_t B[Q];
#pragma unroll
        for (int i = 0; i < Q; i++) B[i] = __builtin_amdgcn_perm(W[i + Q], W[i], 0x06020400u);
        quant_transpose<ROWS, 8>(B, P, valid, planes, BT, lane);
    }
    return P;
}

// 32-bit index plane (sources deeper than 8 bits, small quantiser steps): up
// to 31 planes, by the nibble spread.
template <int ROWS>
__device__ __forceinline__ int quant_columns32(const QuantArgs &a, const BlockDesc &d, int b, int lane, bool act, bool keep_sm,
                                               uint64_t valid, int32_t *sm, uint64_t *planes) {
    static_assert(ROWS == 64 || ROWS == 32, "quant_columns32: 64 or 32 rows");
    const size_t e0 = (size_t)d.tc * a.plane_w * a.plane_h + (size_t)d.y0 * a.plane_w + d.x0;
    const uint32_t *src = (const uint32_t *)a.coef + e0;
    const int cl = act ? lane : 0;
    const int hm1 = d.h - 1;
    uint32_t col[ROWS];
#pragma unroll
    for (int y = 0; y < ROWS; y++) col[y] = src[(size_t)min(y, hm1) * a.plane_w + cl];
    // magnitudes in col[], the signs straight into the sign column
    uint32_t sg_lo = 0, sg_hi = 0, vor = 0;
#pragma unroll
    for (int y = 0; y < ROWS; y++) {
        const uint32_t raw = col[y];
        if (y < 32) sg_lo |= (raw >> 31) << y;
        else sg_hi |= (raw >> 31) << (y - 32);
        col[y] = raw & 0x7FFFFFFFu;
        vor |= col[y];
    }
    const uint64_t sgcol = (((uint64_t)sg_hi << 32) | sg_lo) & valid;
    if (keep_sm) {
#pragma unroll
        for (int y = 0; y < ROWS; y++)
            if (y < d.h) sm[y * 64] = act ? (int32_t)(col[y] | (uint32_t)((sgcol >> y) & 1u) << 31) : 0;
    }
    uint64_t *BT = a.bp + d.bp_off;
    const int P = quant_planes_and_signs(a, d, b, lane, vor, sgcol, BT);
    // Four planes at a time: a row's 4 bits are spread to the 4 bytes of a
    // word by one multiply (nib * 0x204081 & 0x01010101), so G[g] collects
    // rows 8g..8g+7 with plane p0+k in byte k; each plane's 64-bit mask is
    // then byte k of G[0..7], gathered by v_perm_b32 (4 ops per row group of
    // 4 planes instead of 2 per row and plane)
    for (int p0 = 0; p0 < P; p0 += 4) {
        uint32_t G[ROWS / 8];
#pragma unroll
        for (int g = 0; g < ROWS / 8; g++) {
            uint32_t acc = 0;
#pragma unroll
            for (int i = 0; i < 8; i++)
                acc |= (__umul24(__builtin_amdgcn_ubfe(col[8 * g + i], (uint32_t)p0, 4u), 0x00204081u) & 0x01010101u) << i;
            G[g] = acc;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int p = p0 + k;
            if (p >= P) break;
            // bytes k of (G0, G1) and (G2, G3) -> low halves; the pair merged
            const uint32_t sel = (uint32_t)k | ((uint32_t)(k + 4) << 8) | 0x0C0C0000u;
            const uint32_t lo = __builtin_amdgcn_perm(G[1], G[0], sel) | (__builtin_amdgcn_perm(G[3], G[2], sel) << 16);
            uint32_t hi = 0;
            if constexpr (ROWS == 64)
                hi = __builtin_amdgcn_perm(G[5], G[4], sel) | (__builtin_amdgcn_perm(G[7], G[6], sel) << 16);
            const uint64_t m = (((uint64_t)hi << 32) | lo) & valid;
            planes[p * 64 + lane] = m;
            BT[(size_t)p * 64 + lane] = m;
        }
    }
    return P;
}

// The sum over the wave of one row of the plane loop's per-lane partials: row
// rho = 2 * plane + k (k = 0: sv, 1: sl), the 64 dwords w32[128 plane + 2 j +
// k], int32 each, added up in 64 bits.  R = 2^lgR >= the number of rows (4..64)
// lanes take a row each, 64 / R lanes per row; a lane walks R entries of its
// row, starting R entries apart from the row's other lanes and one entry
// further for every lane, so that the reads of a step spread over the banks;
// the row's lanes then add their parts (every lane of a row returns the row's
// total).  Rows past `rows` read row 0 and return nothing of use.
__device__ __forceinline__ int64_t quant_row_sum(const int32_t *w32, int rows, int lgR, int lane) {
    const int R = 1 << lgR;
    const int rho = lane & (R - 1);
    const int r = rho < rows ? rho : 0;
    const int base = (r >> 1) * 128 + (r & 1);
    const int j0 = (lane >> lgR) << lgR;
    int64_t acc = 0;
#pragma unroll 4
    for (int t = 0; t < R; t++) {
        const int j = j0 + ((t + lane) & (R - 1));
        acc += w32[base + 2 * j];
    }
    for (int o = R; o < 64; o <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)acc, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)acc >> 32), o, 64);
        acc += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return acc;
}

template <bool REV, bool Q16>
__global__ void __launch_bounds__(64 * kQuantWaves) k_quant(QuantArgs a) {
    extern __shared__ uint64_t lds_planes[];  // [wave][plane][lane], a.max_mb planes per wave
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * kQuantWaves + wv;
#pragma unroll
    for (int z = 0; z < kZeroSpans; z++)
        for (uint32_t i = blockIdx.x * 64 * kQuantWaves + threadIdx.x; i < a.nzero[z]; i += gridDim.x * 64 * kQuantWaves)
            a.zero[z][i] = 0u;
    if (b >= a.nblocks) return;
    uint64_t *planes = lds_planes + (size_t)wv * a.max_mb * 64;
    BlockDesc d = a.blocks[b];
    int lane = threadIdx.x & 63;
    bool act = lane < d.w;
    int32_t *sm = a.sm + d.sm_off + lane;
    // the sign-magnitude copy is read only by the 64-bit distortion path of
    // planes above 23 (below) and by the debug dumps
    const bool keep_sm = a.keep_sm || d.Mb > 24;
    const uint64_t hmask = d.h >= 64 ? ~0ull : ((1ull << d.h) - 1ull);
    const uint64_t valid = act ? hmask : 0ull;  // rows < h of columns < w
    // short blocks (the deep levels' bands) load and transpose only 32 rows
    int P;
    if constexpr (Q16)
        P = d.h > 32 ? quant_columns16<64>(a, d, b, lane, act, keep_sm, valid, sm, planes)
                     : quant_columns16<32>(a, d, b, lane, act, keep_sm, valid, sm, planes);
    else
        P = d.h > 32 ? quant_columns32<64>(a, d, b, lane, act, keep_sm, valid, sm, planes)
                     : quant_columns32<32>(a, d, b, lane, act, keep_sm, valid, sm, planes);
    constexpr bool lossless = REV;
    constexpr int dd = lossless ? 0 : 1;  // reconstruction offset, half-units
    const bool wcol = lane < d.w;
    uint64_t colS = 0;       // S[p+1] of this column
    uint32_t cnt_above = 0;  // |S[p+1]| over the block
    // Planes top-down.  Distortion decreases of plane p (oracle dist_gain,
    // half-units, d = reconstruction offset): a sample whose top bit is p
    // gains 2^p (12 v + 6d - 9 2^p); one significant above p, with l = v mod
    // 2^p, gains 2^p (4l + 2d - 2^p) if bit p is set, else 2^p (3 2^p - 4l -
    // 2d); lossless p = 0 gains 4 for a new sample and for a refined 0 bit,
    // nothing else.  The sums of v over new samples (N) and of +-l over
    // refined ones (R1: bit p set, R0: clear) come from the column masks:
    // sum_N v = sum_{q<=p} 2^q |N & B[q]|, sum_R +-l = sum_{q<p} 2^q (|R1 &
    // B[q]| - |R0 & B[q]|), int32 per lane up to p = 23.  The slope-prediction
    // counts (oracle plane_stats): significant samples, and insignificant
    // samples with a significant 8-neighbour; their wave totals by DPP scans,
    // cS and cN (<= 4096 each) sharing one scan.
    uint32_t cS, cN, nb1;
    auto plane_counts = [&]() {
        // insignificant samples with a significant 8-neighbour (rows < h,
        // columns < w)
        // (DPP whole-wave shifts on every lane: lanes 0 / 63 receive 0)
        const uint64_t Lc = wave_shr1(colS), Rc = wave_shl1(colS);
        const uint64_t H = colS | Lc | Rc;
        const uint32_t n = wcol ? (uint32_t)__popcll((H | (H << 1) | (H >> 1)) & ~colS & hmask) : 0u;
        const uint32_t both = wave_sum_u32((uint32_t)__popcll(colS) | (n << 16));
        cS = both & 0xFFFFu;
        cN = both >> 16;
        nb1 = wave_sum_u32(nb1);
    };
    int p = P - 1;
    // Planes above 23 (never for <= 16-bit sources): 64-bit gains per row,
    // the column re-read from the sign-magnitude copy, summed over the wave
    // plane by plane.
    for (; p > 23; p--) {
        const uint64_t Bp = planes[p * 64 + lane];
        nb1 = (uint32_t)__popcll(colS & Bp);
        int64_t ref = 0, sig = 0;
        for (int y = 0; y < d.h; y++) {
            const uint32_t v = (uint32_t)sm[y * 64] & 0x7FFFFFFFu;
            const uint32_t hi = v >> p;
            if (hi == 0) continue;
            const int64_t g = dist_gain(v, p, lossless);
            if (hi == 1) sig += g;
            else ref += g;
        }
        colS |= Bp;
        plane_counts();
        ref = wave_sum64(ref);
        sig = wave_sum64(sig);
        if (lane == 0) {
            a.est[(size_t)b * 32 + p] = 16u * cnt_above + 56u * (cS - cnt_above) + 5u * cN;
            a.dref[(size_t)b * 32 + p] = ref;
            a.dsig[(size_t)b * 32 + p] = sig;
        }
        cnt_above = cS;
    }
    // Planes 23 and below.  The lane's sv and sl are not summed over the wave
    // here: they go to planes[p][lane], which is dead once plane p is done
    // (lower planes read only planes[q], q < p), and one reduction per block
    // follows the loop.  Lane p keeps plane p's three counts for it.
    const int Pn = p + 1;  // min(P, 24)
    uint32_t my_cS = 0, my_nb1 = 0, my_above = 0;
    for (; p >= 0; p--) {
        const uint64_t Bp = planes[p * 64 + lane];
        const uint64_t N = Bp & ~colS, R1 = colS & Bp;
        nb1 = (uint32_t)__popcll(R1);  // refined samples with bit p set
        int32_t sv = __popcll(N) << p, sl = 0;
        for (int q = 0; q < p; q++) {
            const uint64_t Bq = planes[q * 64 + lane];
            sv += __popcll(N & Bq) << q;
            sl += (2 * __popcll(R1 & Bq) - __popcll(colS & Bq)) * (1 << q);
        }
        colS |= Bp;
        planes[p * 64 + lane] = (uint64_t)(uint32_t)sv | ((uint64_t)(uint32_t)sl << 32);
        plane_counts();
        if (lane == 0) a.est[(size_t)b * 32 + p] = 16u * cnt_above + 56u * (cS - cnt_above) + 5u * cN;
        if (lane == p) {
            my_cS = cS;
            my_nb1 = nb1;
            my_above = cnt_above;
        }
        cnt_above = cS;
    }
    // The block's sums: rows 2p (sv) and 2p + 1 (sl), a lane or several a row
    const int rows = 2 * Pn;
    if (rows == 0) return;
    int lgR = 2;
    while ((1 << lgR) < rows) lgR++;  // rows <= 48
    const int64_t tot = quant_row_sum((const int32_t *)planes, rows, lgR, lane);
    // the row totals go through LDS to the lane of their plane (every partial
    // has been read: the wave's LDS operations complete in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < rows) planes[lane] = (uint64_t)tot;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < Pn) {
        p = lane;
        const int64_t SV = (int64_t)planes[2 * p], SL = (int64_t)planes[2 * p + 1];
        const int64_t n1 = my_cS - my_above, nr1 = my_nb1, nr0 = my_above - my_nb1, q = (int64_t)1 << p;
        int64_t ref, sig;
        if (lossless && p == 0) {
            sig = 4 * n1;
            ref = 4 * nr0;
        } else {
            sig = q * (12 * SV + (6 * dd - 9 * q) * n1);
            ref = q * (4 * SL + nr1 * (2 * dd - q) + nr0 * (3 * q - 2 * dd));
        }
        a.dref[(size_t)b * 32 + p] = ref;
        a.dsig[(size_t)b * 32 + p] = sig;
    }
}

// --------------------------------------------------------------------------
// S4b: slope prediction (rate-driven encodes; oracle/jp2_oracle.c
// predict_and_code).  kdu_compress "-rate" (KakaduConverter.java:44) stops
// its block coder at a predicted slope threshold instead of coding passes
// PCRD-opt will discard.  Plane p of a block has predicted slope
// pd * weight / est; est is histogrammed over 1/8-octave slope bins, the bin
// where the predicted size reaches the target fixes the cut, and planes more
// than kSkipMargin bins below it are not coded (pmin = lowest coded plane).
// All integer after the one IEEE division, so the oracle agrees bit for bit.
// --------------------------------------------------------------------------
__device__ __forceinline__ int slope_bin(double s) {
    if (!(s > 0.0)) return -1;
    const uint64_t k = (uint64_t)__double_as_longlong(s);
    const int b = (int)(k >> 49) - kSlopeBinBase;
    return b < 0 ? 0 : (b >= kSlopeBins ? kSlopeBins - 1 : b);
}
__device__ __forceinline__ int plane_bin(int64_t pd, double wgt, uint32_t est) {
    if (est == 0) return pd > 0 ? kSlopeBins - 1 : -1;
    return slope_bin((double)pd * wgt / (double)est);
}

struct PredictArgs {
    int nblocks;
    const uint8_t *P;
    const int64_t *dref, *dsig;
    const uint32_t *est;
    const double *weight;
    unsigned long long *hist;  // [kSlopeBins]
    uint8_t *pmin;
};

// Thread per block, its planes in a loop (a thread per (block, plane) slot
// left most lanes idle: 32 slots for ~12 planes); a workgroup covers
// kHistBlocks consecutive blocks, whose planes land in few bins, so it sums
// into an LDS histogram and flushes only the bins it touched.
constexpr int kHistBlocks = 1024;
__global__ void __launch_bounds__(256) k_plane_hist(PredictArgs a) {
    __shared__ unsigned long long lh[kSlopeBins];
    for (int i = threadIdx.x; i < kSlopeBins; i += 256) lh[i] = 0;
    __syncthreads();
    const int b0 = blockIdx.x * kHistBlocks;
    const int b1 = min(a.nblocks, b0 + kHistBlocks);
    for (int b = b0 + (int)threadIdx.x; b < b1; b += 256) {
        const int Pb = a.P[b];
        const double wb = a.weight[b];
        const size_t i0 = (size_t)b * 32;
        // the next plane's three loads in flight while this one is binned
        int64_t dd = Pb > 0 ? a.dref[i0] + a.dsig[i0] : 0;
        uint32_t e = Pb > 0 ? a.est[i0] : 0u;
        for (int p = 0; p < Pb; p++) {
            const int pn = min(p + 1, 31);
            const int64_t ddn = a.dref[i0 + pn] + a.dsig[i0 + pn];
            const uint32_t en = a.est[i0 + pn];
            const int k = plane_bin(dd, wb, e);
            if (k >= 0) atomicAdd(&lh[k], (unsigned long long)e);
            dd = ddn;
            e = en;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kSlopeBins; k += 256)
        if (lh[k]) atomicAdd(&a.hist[k], lh[k]);
}

// kstar = #{k in [1, kSlopeBins) : sum_{j >= k} hist[j] >= goal} (the
// oracle's downward scan), kcut = kstar - kSkipMargin.  One wave; lane l owns
// bins [16 l, 16 l + 16).
__device__ __forceinline__ int plane_cut(const unsigned long long *hist, int64_t goal) {
    const int lane = threadIdx.x & 63;
    constexpr int kPer = kSlopeBins / 64;
    unsigned long long h[kPer], part = 0;
#pragma unroll
    for (int i = 0; i < kPer; i++) { h[i] = hist[lane * kPer + i]; part += h[i]; }
    // exclusive suffix sum over lanes: bins above this lane's range
    const uint64_t inc = wave_incl_scan64(part);
    const unsigned long long above =
        (uint64_t)__shfl((long long)inc, 63, 64) - inc;
    int cnt = 0;
    unsigned long long acc = above;
#pragma unroll
    for (int i = kPer - 1; i >= 0; i--) {
        acc += h[i];
        const int k = lane * kPer + i;
        cnt += (k >= 1 && acc >= (unsigned long long)goal) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    return cnt - kSkipMargin;
}

// the lowest coded plane of each block, then its items in tier-1's work lists
// (every workgroup finds the cut from the histogram itself: no launch for it)
__global__ void __launch_bounds__(256) k_plane_pmin(PredictArgs a, T1ItemArgs ia, int64_t goal) {
    __shared__ int kcut;
    __shared__ ItemScratch sc;
    if (threadIdx.x < 64) {
        const int kc = plane_cut(a.hist, goal);
        if (threadIdx.x == 0) kcut = kc;
    }
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = b < a.nblocks;
    const int P = in ? a.P[b] : 0;
    int pmin = P > 0 ? P - 1 : 0;
    if (in) {
        const int kc = kcut;
        const double wgt = a.weight[b];
        // planes 8 at a time: their loads in flight together
        bool found = false;
        for (int p0 = 0; p0 < P && !found; p0 += 8) {
            int64_t dd[8];
            uint32_t e[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const size_t i = (size_t)b * 32 + min(p0 + j, 31);
                dd[j] = a.dref[i] + a.dsig[i];
                e[j] = a.est[i];
            }
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (!found && p0 + j < P && plane_bin(dd[j], wgt, e[j]) >= kc) {
                    pmin = p0 + j;
                    found = true;
                }
        }
        a.pmin[b] = (uint8_t)pmin;
    }
    emit_t1_items<256>(ia, b, in, P, pmin, sc);
}

// --------------------------------------------------------------------------
// run_front: the stages above (and dwt.hip, t1.hip, pcrd.hip's k_hull)
// enqueued on the context's stream, one member function per stage
// --------------------------------------------------------------------------
// what the steps of one run_front share
struct FrontJob {
    const void *d_src;
    const jp2hip_layout &lay;
    const Plan &plan;
    int64_t skip_target;
    const GpuEncoder::HistReduce *reduce;
    bool pool_worst;
    int nb, G;       // code-blocks, rate-control groups
    size_t plane;    // samples of a tile-component plane
    const char *dd;  // debug builds: JP2HIP_DUMP_DIR (every stage's buffer written to files)
    QuantTab qt;     // the final coefficients are written as quantisation indices
    int kmax;        // largest Mb of the plan (front_reserve)
    size_t nflags;   // nb * kmax: bound on the tier-1 items
    IngestArgs ing;  // the first stage's arguments (front_first_args): k_ingest,
    DwtLaunch dl;    // or the fused ingest + DWT
};

bool GpuEncoder::front_reserve(FrontJob &j, std::string &err) {
    const Plan &plan = j.plan;
    const jp2hip_layout &lay = j.lay;
    const int nb = j.nb, G = j.G;
    const size_t plane = j.plane;
    if (!ensure<int32_t>(coef, plane * plan.ntc, err)) return false;
    if (!ensure<BlockDesc>(blocks, nb, err)) return false;
    // MQ lane-order buckets (k_t1_cm3's bslots)
    if (!ensure<int32_t>(order, (size_t)kOrderBuckets * std::max(nb, 1), err)) return false;
    if (!ensure<uint64_t>(bp, plan.bp_words, err)) return false;
    if (!ensure<int32_t>(sm, plan.sm_words, err)) return false;
    if (!ensure<uint8_t>(P, nb, err)) return false;
    if (!ensure<int64_t>(dref, (size_t)nb * 32, err)) return false;
    if (!ensure<int64_t>(dsig, (size_t)nb * 32, err)) return false;
    if (!ensure<uint32_t>(est, (size_t)nb * 32, err)) return false;
    if (!ensure<uint8_t>(pmin, nb, err)) return false;
    if (!ensure<unsigned long long>(hist, kSlopeBins, err)) return false;
    if (!ensure<uint8_t>(t1out, plan.out_bytes + 64, err)) return false;  // + k_t2_copy's dword over-read
    if (!ensure<int32_t>(rates, (size_t)nb * kMaxPasses, err)) return false;
    if (!ensure<int64_t>(dists, (size_t)nb * kMaxPasses, err)) return false;
    if (!ensure<uint8_t>(npasses, nb, err)) return false;
    if (!ensure<int32_t>(lengths, nb, err)) return false;
    if (!ensure<double>(weight, nb, err)) return false;
    if (!ensure<uint8_t>(nhull, nb, err)) return false;
    if (!ensure<uint8_t>(hpass, (size_t)nb * (kMaxPasses + 1), err)) return false;
    if (!ensure<uint64_t>(hkey, (size_t)nb * (kMaxPasses + 1), err)) return false;
    if (!ensure<int64_t>(hdist, (size_t)nb * (kMaxPasses + 1) * 2, err)) return false;  // HullPt
    if (!ensure<int64_t>(budget, (size_t)G * kMaxLayers, err)) return false;
    if (!ensure<uint8_t>(nl, (size_t)nb * plan.rc.layers, err)) return false;
    if (!ensure<int32_t>(lrate, (size_t)nb * plan.rc.layers, err)) return false;
    if (!ensure<int>(this->err, 4, err)) return false;
    if (!ensure<int32_t>(tcw, plan.ntc, err)) return false;
    if (!ensure<int32_t>(tch, plan.ntc, err)) return false;
    if (!ensure<uint64_t>(strips, lay.nstrips, err)) return false;

    // tier-1 decision streams: one pool, carved on the device once the coded
    // planes are known (emit_t1_items: c planes x plane_stream_cap per
    // block).  Sized at a fraction of the every-plane bound -- or at what an
    // encode of this context last needed, when that is more -- and grown
    // after an encode that did not fit (the host re-encodes: pool_grow).
    // The tile-split path asks for the whole bound (its ranks cannot repeat
    // an exchange).
    uint64_t stream_bound = 0;
    j.kmax = 0;
    for (int i = 0; i < nb; i++) {
        stream_bound += (uint64_t)plan.blocks[i].Mb * t1_plane_stream_cap(plan.blocks[i].w, plan.blocks[i].h);
        j.kmax = std::max(j.kmax, (int)plan.blocks[i].Mb);
    }
    j.nflags = (size_t)nb * j.kmax;
    const double pool_frac = j.pool_worst           ? 1.0
                             : pool_frac_test >= 0.0 ? pool_frac_test
                             : (plan.rc.reversible ? kPoolFracLossless : kPoolFracLossy);
    const uint64_t pool_want = std::min<uint64_t>(
        stream_bound, std::max<uint64_t>(pool_hint, (uint64_t)((double)stream_bound * pool_frac)));
    return ensure<uint64_t>(slotoff, nb, err) && ensure<uint8_t>(stream_buf, std::max<uint64_t>(pool_want, 1), err);
}

// the strip offsets, the plan's tables and the rate-control group table
bool GpuEncoder::front_upload(const FrontJob &j, std::string &err) {
    const Plan &plan = j.plan;
    const jp2hip_layout &lay = j.lay;
    const int nb = j.nb, G = j.G;
    // the strip offsets: uploaded only when they differ from the last upload
    // (repeat encodes of one layout skip the copy)
    if (strips.ptr != strips_dev || strips_host.size() != (size_t)lay.nstrips ||
        std::memcmp(strips_host.data(), lay.strip_offsets, sizeof(uint64_t) * lay.nstrips) != 0) {
        if (!h2d(strips.ptr, lay.strip_offsets, sizeof(uint64_t) * lay.nstrips, err)) return false;
        strips_host.assign(lay.strip_offsets, lay.strip_offsets + lay.nstrips);
        strips_dev = strips.ptr;
    } else if (!reuse_front_noted) {
        reuse |= JP2HIP_REUSED_STRIPS;
    }
    // the plan's tables stay resident while the context encodes the same
    // geometry (plan.gen; buffers only grow, so they are still in place)
    if (!plan.gen || plan.gen != front_gen) {
        front_gen = 0;
        if (!h2d(blocks.ptr, plan.blocks.data(), sizeof(BlockDesc) * nb, err) ||
            !h2d(weight.ptr, plan.weight.data(), sizeof(double) * nb, err) ||
            !h2d(tcw.ptr, plan.tc_w.data(), sizeof(int32_t) * plan.ntc, err) ||
            !h2d(tch.ptr, plan.tc_h.data(), sizeof(int32_t) * plan.ntc, err))
            return false;
        // rate-control groups: block ranges and each group's first
        // candidate slot (the bound sum(3 Mb - 2) over the groups before)
        std::vector<int32_t> gtab(2 * ((size_t)G + 1));
        int64_t sb = 0;
        for (int g = 0; g <= G; g++) {
            gtab[(size_t)g] = plan.grp_b0[(size_t)g];
            gtab[(size_t)G + 1 + g] = (int32_t)sb;
            if (g < G)
                for (int i = plan.grp_b0[(size_t)g]; i < plan.grp_b0[(size_t)g + 1]; i++)
                    sb += std::max(0, 3 * (int)plan.blocks[i].Mb - 2);
        }
        if (!ensure<int32_t>(grptab, gtab.size(), err) || !h2d(grptab.ptr, gtab.data(), sizeof(int32_t) * gtab.size(), err))
            return false;
        front_gen = plan.gen;
    } else if (!reuse_front_noted) {
        reuse |= JP2HIP_REUSED_FRONT_TABLES;
    }
    reuse_front_noted = true;
    // (the error word is zeroed by k_quant, which every encode with blocks runs)
    if (!nb) {
        HIPCHECK(hipMemsetAsync(this->err.ptr, 0, sizeof(int), stream));
        if (!ensure<T2Summary>(t2sum, 1, err)) return false;
        HIPCHECK(hipMemsetAsync(t2sum.ptr, 0, sizeof(T2Summary), stream));  // (k_hull's totals: none)
    }
    return true;
}

// S1-S3: the arguments of k_ingest (no decomposition) or of the fused ingest +
// DWT, and the DWT's scratch planes
bool GpuEncoder::front_first_args(FrontJob &j, std::string &err) {
    const Plan &plan = j.plan;
    const jp2hip_layout &lay = j.lay;
    const void *d_src = j.d_src;
    const QuantTab &qt = j.qt;
    IngestArgs &ing = j.ing;
    DwtLaunch &dl = j.dl;
    if (plan.rc.levels == 0) {
        // S1+S2 only: no decomposition
        ing.src = (const uint8_t *)d_src;
        ing.strip_off = (const uint64_t *)strips.ptr;
        ing.rps = lay.rows_per_strip;
        ing.w = plan.w; ing.h = plan.band_h; ing.nc = plan.nc; ing.bits = plan.bits;
        ing.row0 = plan.row0;
        ing.planar = lay.planar; ing.big_endian = lay.big_endian;
        ing.mct = plan.rc.mct; ing.reversible = plan.rc.reversible;
        ing.ntx = plan.ntx; ing.tile_w = plan.rc.tile_w; ing.tile_h = plan.rc.tile_h;
        ing.plane_w = plan.plane_w; ing.plane_h = plan.plane_h;
        ing.spp_strips = (plan.h + lay.rows_per_strip - 1) / lay.rows_per_strip;
        ing.coef = coef.ptr;
        ing.inv = qt.inv[0][0]; ing.lim = qt.lim[0][0]; ing.q16 = qt.q16;
    } else {
        // S1+S2+S3 fused: ingest inside DWT level 1 (dwt.hip)
        const size_t llw = (size_t)((plan.plane_w + 1) / 2) * ((plan.plane_h + 1) / 2) * plan.ntc;
        if (!ensure<int32_t>(llbuf0, llw, err) || !ensure<int32_t>(llbuf1, llw, err)) return false;
        dl.tif = d_src;
        dl.strip_off = (const uint64_t *)strips.ptr;
        dl.rps = lay.rows_per_strip;
        dl.img_w = plan.w; dl.nc = plan.nc; dl.bits = plan.bits;
        dl.planar = lay.planar; dl.big_endian = lay.big_endian; dl.mct = plan.rc.mct;
        dl.spp_strips = (plan.h + lay.rows_per_strip - 1) / lay.rows_per_strip;
        dl.ntx = plan.ntx; dl.tile_w = plan.rc.tile_w; dl.tile_h = plan.rc.tile_h; dl.row0 = plan.row0;
        dl.last_tile_w = plan.w - (plan.ntx - 1) * plan.rc.tile_w;
        dl.src_end = source_end(lay.strip_offsets, lay.rows_per_strip, dl.spp_strips, lay.planar == 2 ? plan.nc : 1,
                                plan.row0, plan.row0 + plan.band_h,
                                (uint64_t)plan.w * (lay.planar == 2 ? 1 : plan.nc) * (plan.bits >> 3));
        dl.plane_w = plan.plane_w; dl.plane_h = plan.plane_h; dl.ntc = plan.ntc;
        dl.levels = plan.rc.levels; dl.reversible = plan.rc.reversible;
        dl.tc_w = (const int32_t *)tcw.ptr; dl.tc_h = (const int32_t *)tch.ptr;
        dl.coef = coef.ptr; dl.scratch0 = llbuf0.ptr; dl.scratch1 = llbuf1.ptr;
        dl.qt = qt;
    }
    return true;
}

bool GpuEncoder::front_ingest_dwt(const FrontJob &j, std::string &err) {
    const Plan &plan = j.plan;
    if (plan.rc.levels == 0) {
        dim3 gi((plan.w + 63) / 64, (plan.band_h + 3) / 4);
        hipLaunchKernelGGL(k_ingest, gi, dim3(256), 0, stream, j.ing);
        HIPCHECK(hipGetLastError());
    } else {
        bool dwt_ok = true;
        const char *why = nullptr;
        REPEAT_IF(1) dwt_ok = dwt_ok && launch_dwt(j.dl, stream, &why);
        if (!dwt_ok) {
            err = why ? std::string(why) : std::string("DWT launch failed: ") + hipGetErrorString(hipGetLastError());
            return false;
        }
    }
    return true;
}

// S4: the quantiser, which also zeroes the per-encode counters of the later
// kernels (tier-1 work lists and lane order, slope prediction, PCRD: spans
// spread over its workgroups, no memset launches)
bool GpuEncoder::front_quant(const FrontJob &j, std::string &err) {
    const Plan &plan = j.plan;
    const int nb = j.nb, G = j.G, kmax = j.kmax;
    const size_t nflags = j.nflags;
    const QuantTab &qt = j.qt;
    const char *dd = j.dd;
    QuantArgs qa;
    qa.blocks = (const BlockDesc *)blocks.ptr;
    qa.coef = coef.ptr;
    qa.plane_w = plan.plane_w; qa.plane_h = plan.plane_h;
    qa.reversible = plan.rc.reversible;
    qa.bp = (uint64_t *)bp.ptr;
    qa.sm = (int32_t *)sm.ptr;
    qa.P = (uint8_t *)P.ptr;
    qa.dref = (int64_t *)dref.ptr;
    qa.dsig = (int64_t *)dsig.ptr;
    qa.est = (uint32_t *)est.ptr;
    qa.nblocks = nb;
    qa.keep_sm = dd != nullptr;
    if (!ensure<unsigned long long>(pcrd_hb, (size_t)G * kPcrdBins, err) ||
        !ensure<uint32_t>(pcrd_hc, (size_t)G * kPcrdBins, err) ||
        !ensure<uint32_t>(sel_ctl, (size_t)G * (kMaxLayers + 1), err) ||
        !ensure<unsigned long long>(gtot, G, err) || !ensure<uint32_t>(t1fill, 64 + kOrderBuckets, err) ||
        !ensure<int32_t>(items, std::max<size_t>(nflags, 1), err) ||
        !ensure<uint4>(counts, (size_t)nb * 32, err) || !ensure<int64_t>(dspp, (size_t)nb * 32, err) ||
        !ensure<unsigned long long>(ordkey, std::max(nb, 1), err) || !ensure<unsigned long long>(mqspan, 3, err))
        return false;
    std::memset(qa.zero, 0, sizeof qa.zero);
    std::memset(qa.nzero, 0, sizeof qa.nzero);
    qa.zero[0] = (uint32_t *)pcrd_hb.ptr;
    qa.nzero[0] = 2 * kPcrdBins * G;
    qa.zero[1] = (uint32_t *)pcrd_hc.ptr;
    qa.nzero[1] = kPcrdBins * G;
    qa.zero[2] = (uint32_t *)sel_ctl.ptr;
    qa.nzero[2] = (kMaxLayers + 1) * G;
    qa.zero[3] = (uint32_t *)t1fill.ptr;  // tier-1 list fills [64], then the lane-order bucket fills
    qa.nzero[3] = 64 + kOrderBuckets;
    qa.zero[4] = (uint32_t *)mqspan.ptr;  // k_t1_mq's span[2], then the stream pool's fill
    qa.nzero[4] = 6;
    // (span 5: the error word; span 6: the slope histogram; span 7: tier-1
    // totals; span 8: the rate-control groups' tier-1 bytes)
    qa.zero[8] = (uint32_t *)gtot.ptr;
    qa.nzero[8] = 2 * G;
    qa.zero[5] = (uint32_t *)this->err.ptr;
    qa.nzero[5] = 1;
    // the tier-1 totals k_hull sums (t1_bytes .. skipped: contiguous)
    if (!ensure<T2Summary>(t2sum, 1, err)) return false;
    qa.zero[7] = (uint32_t *)&((T2Summary *)t2sum.ptr)->t1_bytes;
    qa.nzero[7] = (uint32_t)((offsetof(T2Summary, skipped) + sizeof(int32_t) - offsetof(T2Summary, t1_bytes)) / 4);
    if (j.skip_target >= 0) {
        qa.zero[6] = (uint32_t *)hist.ptr;
        qa.nzero[6] = 2 * kSlopeBins;
    }
    qa.max_mb = std::max(1, kmax);
    const size_t qlds = (size_t)qa.max_mb * 64 * sizeof(uint64_t);
    if (nb) {
        const dim3 gq((nb + kQuantWaves - 1) / kQuantWaves), bq(64 * kQuantWaves);
        REPEAT_IF(2) {
            const size_t ql = qlds * kQuantWaves;
            if (plan.rc.reversible) {
                if (qt.q16) hipLaunchKernelGGL((k_quant<true, true>), gq, bq, ql, stream, qa);
                else hipLaunchKernelGGL((k_quant<true, false>), gq, bq, ql, stream, qa);
            } else {
                if (qt.q16) hipLaunchKernelGGL((k_quant<false, true>), gq, bq, ql, stream, qa);
                else hipLaunchKernelGGL((k_quant<false, false>), gq, bq, ql, stream, qa);
            }
        }
    }
    HIPCHECK(hipGetLastError());
    return true;
}

// S4b: slope prediction -> lowest coded plane per block, and the tier-1
// work lists: list k = the blocks with more than k coded planes
bool GpuEncoder::front_predict_items(const FrontJob &j, std::string &err) {
    const int nb = j.nb;
    const int64_t skip_target = j.skip_target;
    const HistReduce *reduce = j.reduce;
    T1ItemArgs ia;
    ia.nb = nb;
    ia.kmax = j.kmax;
    ia.P = (const uint8_t *)P.ptr;
    ia.pmin = (uint8_t *)pmin.ptr;
    ia.dfill = (uint32_t *)t1fill.ptr;
    ia.dlist = (int32_t *)items.ptr;
    ia.acc = (unsigned long long *)ordkey.ptr;
    ia.npasses = (uint8_t *)npasses.ptr;
    ia.lengths = (int32_t *)lengths.ptr;
    ia.blocks = (const BlockDesc *)blocks.ptr;
    ia.pool_used = (unsigned long long *)mqspan.ptr + 2;
    ia.pool_cap = stream_buf.bytes;
    ia.slot_off = (uint64_t *)slotoff.ptr;
    ia.err = (int *)this->err.ptr;
    if (skip_target >= 0 && nb) {
        PredictArgs pa;
        pa.nblocks = nb;
        pa.P = (const uint8_t *)P.ptr;
        pa.dref = (const int64_t *)dref.ptr;
        pa.dsig = (const int64_t *)dsig.ptr;
        pa.est = (const uint32_t *)est.ptr;
        pa.weight = (const double *)weight.ptr;
        pa.hist = (unsigned long long *)hist.ptr;
        pa.pmin = (uint8_t *)pmin.ptr;
        hipLaunchKernelGGL(k_plane_hist, dim3((nb + kHistBlocks - 1) / kHistBlocks), dim3(256), 0, stream, pa);
        HIPCHECK(hipGetLastError());
        if (reduce) {
            h_hist.resize(kSlopeBins);
            if (!host_wait(err)) return false;  // (a pageable copy waits for the stream holding a shared lock)
            HIPCHECK(hipMemcpyAsync(h_hist.data(), hist.ptr, sizeof(int64_t) * kSlopeBins, hipMemcpyDeviceToHost,
                                    stream));
            if (!host_wait(err)) return false;
            if (!(*reduce)(h_hist)) {
                err = "split: slope-prediction exchange failed";
                return false;
            }
            if (!h2d(hist.ptr, h_hist.data(), sizeof(int64_t) * kSlopeBins, err)) return false;
        }
        hipLaunchKernelGGL(k_plane_pmin, dim3((nb + 255) / 256), dim3(256), 0, stream, pa, ia, skip_target * 128);
        HIPCHECK(hipGetLastError());
    } else {
        launch_t1_items(ia, stream);
        HIPCHECK(hipGetLastError());
    }
    return true;
}

// S5: tier-1.  k_t1_cm3 takes the items depth by depth; each block's last
// plane files it in its MQ lane-order bucket (decision count), which
// k_t1_mq reads.  Buffers and the grid are sized by the plan's bound
// (every plane of every block coded).
bool GpuEncoder::front_t1(const FrontJob &j, std::string &err) {
    const Plan &plan = j.plan;
    const int nb = j.nb;
    uint32_t *dfill = (uint32_t *)t1fill.ptr, *bfill = dfill + 64;
    T1CmArgs ca;
    ca.dfill = dfill;
    ca.dlist = (const int32_t *)items.ptr;
    ca.nb = nb;
    ca.kmax = j.kmax;
    ca.max_items = (int)j.nflags;
    ca.blocks = (const BlockDesc *)blocks.ptr;
    ca.bp = (const uint64_t *)bp.ptr;
    ca.sm = (const int32_t *)sm.ptr;
    ca.P = (const uint8_t *)P.ptr;
    ca.stream = (uint8_t *)stream_buf.ptr;
    ca.slot_off = (const uint64_t *)slotoff.ptr;
    ca.counts = (uint4 *)counts.ptr;
    ca.dspp = (int64_t *)dspp.ptr;
    ca.acc = (unsigned long long *)ordkey.ptr;
    ca.bfill = bfill;
    ca.bslots = (int32_t *)order.ptr;
    ca.lossless = plan.rc.reversible;
    launch_t1_cm(ca, stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(ev[kEvCmEnd], stream));
    T1MqArgs ma;
    ma.blocks = (const BlockDesc *)blocks.ptr;
    ma.bfill = bfill;
    ma.bslots = (const int32_t *)order.ptr;
    ma.nblocks = nb;
    ma.P = (const uint8_t *)P.ptr;
    ma.pmin = (const uint8_t *)pmin.ptr;
    ma.stream = (const uint8_t *)stream_buf.ptr;
    ma.slot_off = (const uint64_t *)slotoff.ptr;
    ma.counts = (const uint4 *)counts.ptr;
    ma.dspp = (const int64_t *)dspp.ptr;
    ma.dref = (const int64_t *)dref.ptr;
    ma.dsig = (const int64_t *)dsig.ptr;
    ma.out = (uint8_t *)t1out.ptr;
    ma.rates = (int32_t *)rates.ptr;
    ma.dists = (int64_t *)dists.ptr;
    ma.npasses = (uint8_t *)npasses.ptr;
    ma.lengths = (int32_t *)lengths.ptr;
    ma.err = (int *)this->err.ptr;
    ma.dbg = nullptr;
    ma.span = (unsigned long long *)mqspan.ptr;
    if (j.dd) {
        if (!ensure<int64_t>(dbgbuf, (size_t)nb * 6, err)) return false;
        ma.dbg = (int64_t *)dbgbuf.ptr;
    }
    REPEAT_IF(3) launch_t1_mq(ma, stream);
    HIPCHECK(hipGetLastError());
    return true;
}

// every stage's device buffer written to files: a debug build only
// (make JP2HIP_DEBUG=1), for the tools in tests/tools
bool GpuEncoder::front_dumps(const FrontJob &j, std::string &err) {
    const Plan &plan = j.plan;
    const size_t nb = (size_t)j.nb;
    const struct { const char *name; const DevBuf &b; size_t bytes; } files[] = {
        {"blocks.bin", blocks, sizeof(BlockDesc) * nb}, {"sm.bin", sm, plan.sm_words * 4}, {"P.bin", P, nb},
        {"t1out.bin", t1out, plan.out_bytes}, {"lengths.bin", lengths, nb * 4}, {"npasses.bin", npasses, nb},
        {"rates.bin", rates, nb * kMaxPasses * 4}, {"dists.bin", dists, nb * kMaxPasses * 8},
        {"dref.bin", dref, nb * 32 * 8}, {"dsig.bin", dsig, nb * 32 * 8}, {"est.bin", est, nb * 32 * 4},
        {"pmin.bin", pmin, nb}, {"bp.bin", bp, plan.bp_words * 8}, {"mqdbg.bin", dbgbuf, nb * 6 * 8}};
    for (const auto &f : files)
        if (!dump(j.dd, f.name, f.b, f.bytes, err)) return false;
    return true;
}

bool GpuEncoder::run_front(const void *d_src, const jp2hip_layout &lay, const Plan &plan,
                           bool profile, StageTimes &st, std::string &err, int64_t skip_target,
                           const HistReduce *reduce, bool pool_worst) {
    HIPCHECK(hipSetDevice(device));
#ifdef JP2HIP_DEBUG_DUMPS
    const char *dd = getenv("JP2HIP_DUMP_DIR");
#else
    const char *dd = nullptr;
#endif
    FrontJob j{d_src, lay, plan, skip_target, reduce, pool_worst, (int)plan.blocks.size(), plan.ngroups(),
               (size_t)plan.plane_w * plan.plane_h, dd, quant_tab(plan.rc, plan.bits)};
    if (!front_reserve(j, err) || !front_upload(j, err)) return false;
    // the first stage's arguments are prepared before its events: on an idle
    // stream the GPU waits from the event to the first launch, so host work
    // placed there was timed as DWT (≈80 us of a 310 us C2 stage alone,
    // against 232 us of DWT kernels in the rocprofv3 trace of the same run,
    // profiles/r06/dwt_stage_events.txt)
    if (!front_first_args(j, err)) return false;
    HIPCHECK(hipEventRecord(ev[kEvFrontBegin], stream));
    HIPCHECK(hipEventRecord(ev[kEvDwtBegin], stream));
    if (!front_ingest_dwt(j, err)) return false;  // S1-S3
    HIPCHECK(hipEventRecord(ev[kEvDwtEnd], stream));
    if (dd && !dump(dd, "dwt.bin", coef, j.plane * plan.ntc * (j.qt.q16 ? 2 : 4), err)) return false;
    if (!front_quant(j, err)) return false;          // S4
    if (!front_predict_items(j, err)) return false;  // S4b
    HIPCHECK(hipEventRecord(ev[kEvQuantEnd], stream));
    HIPCHECK(hipEventRecord(ev[kEvCmBegin], stream));
    if (!front_t1(j, err)) return false;  // S5 (records kEvCmEnd between the modeller and the coder)
    HIPCHECK(hipEventRecord(ev[kEvMqEnd], stream));
    if (!hull_launch(plan, err)) return false;  // S6a (pcrd.hip)
    HIPCHECK(hipEventRecord(ev[kEvHullEnd], stream));
    profiled = profile;
    if (dd && !front_dumps(j, err)) return false;
    // no host wait: tier-1 totals and the overflow flag reach the host with
    // the first tier-2 summary (t2_size), stage times via collect_profile()
    return true;
}

}  // namespace jp2hip
