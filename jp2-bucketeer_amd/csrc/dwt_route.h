// dwt_route.h -- which kernel form lifts each DWT level of an encode, on what
// grid and with how much LDS, and the staging geometry that decision rests on.
// GPU-free (host and device): the kernels and launch_dwt (dwt.hip) and the CPU
// test (tests/host/test_dwt_route.cpp, under ASan / UBSan) share this file.
//
// dwt.hip has eight kernel forms.  Level 1 reads the TIFF: the streaming
// k_dwt_l1s (tiles up to 1024 wide whose components' rows fit in LDS
// together, 1, 2 or 4 columns per thread), the windowed k_dwt_l1 (wider such
// tiles), k_dwt_l1 in column chunks (16 rows of the level do not fit in a
// workgroup's LDS), or k_dwt_band with ingest, one component per workgroup
// (the rest).  Levels >= 2 read the previous level's LL: k_dwt_band on whole
// rows, in workgroups of 256 threads or -- levels at most 128 wide -- of 128,
// or in column chunks; and from the first level of at most 64 x 64 samples on
// k_dwt_tail runs every remaining level in one launch.  dwt_route() decides,
// launch_dwt only dispatches on what it returns.
#pragma once

#include <cstddef>

#include "dwt_chunk.h"

namespace jp2hip {

constexpr int kDwtThreads = 256;
constexpr int kDwtHalo = 4;           // >= lifting steps (9/7: 4, 5/3: 2)
constexpr int kDwtLdsWords = 16384;   // 64 KiB: band workgroups for rows <= 1024, tail
constexpr int kDwtLdsWordsWide = 32768;  // 128 KiB: what the wide instances opt in to (level 1's routes compare with it)
static_assert(kDwtHalo == kDwtChunkHalo, "one halo, rows and columns");

constexpr int kPadL = 4;   // LDS words in front of row 0 (the first segment's left halo)
// LDS row stride for W samples: a multiple of 4 words (16-byte reads), = 4
// mod 64 so consecutive rows start on different banks
JP2HIP_HD constexpr int lds_row_stride(int W) { return ((W + 63) & ~63) + 4; }
constexpr int kPadR = 24;  // LDS words after the last row (the last segment's right halo)
// Skewed staging layout (k_dwt_l1s): 4 words of padding after every 16
// samples.  hlift_seg's lanes read 16-sample segments, 16 bytes at a time;
// in the dense layout the 16 lanes of a ds_read_b128 group sit 16 words
// apart, so only 4 distinct bank windows serve them (4-way conflicts); at 20
// words apart every lane of the group has its own 4 banks.
JP2HIP_HD constexpr int skew_x(int x) { return x + ((x >> 4) << 2); }
JP2HIP_HD constexpr int lds_row_stride_skew(int W) { return ((W + 15) >> 4) * 20 + 4; }
constexpr int kPadLs = 8;  // ... words in front of row 0: segment 0 reads 8 words before its samples

// The switches that change a route (make VARIANT=... VARIANT_FLAGS=-D...).
#ifndef JP2HIP_STREAM_BAND
#define JP2HIP_STREAM_BAND 64
#endif
constexpr int kStreamBand = JP2HIP_STREAM_BAND;  // k_dwt_l1s: output rows per workgroup
#ifndef JP2HIP_L1S_SKEW
#define JP2HIP_L1S_SKEW 1  // the skewed staging layout (hlift_seg's reads conflict-free)
#endif
constexpr bool kL1sSkew = JP2HIP_L1S_SKEW != 0;
#ifndef JP2HIP_L1S_R
#define JP2HIP_L1S_R 4  // rows per horizontal batch (4 or 8)
#endif
// (99 VGPRs, 4 waves per SIMD for the C2 variant; a budget for 5 --
// amdgpu_waves_per_eu(5), 5 VGPRs spilled -- measured no faster: 146.7 vs
// 146.4 us, profiles/r05/ab_select_fold.txt)
constexpr int kL1sRows = JP2HIP_L1S_R;
#ifndef JP2HIP_BAND_RB
#define JP2HIP_BAND_RB 16
#endif
#ifndef JP2HIP_BAND_NARROW
#define JP2HIP_BAND_NARROW 128  // levels at most this wide: workgroups of this many threads
#endif
// k_dwt_band's kept rows per workgroup (16: 8 took 2 x 40 us for levels 2-3, 16 70 us, profiles/r04/ab_dwt_band.txt)
constexpr int kBandRb = JP2HIP_BAND_RB;
// (a level of <= 128 columns in 128-thread workgroups: with 256 threads half
// of them had no column)
constexpr int kBandNarrow = JP2HIP_BAND_NARROW < kDwtThreads ? JP2HIP_BAND_NARROW : kDwtThreads;
constexpr int kRb1 = 8;  // k_dwt_l1's kept rows per workgroup

constexpr int kTailThreads = 256;
constexpr int kTailWords = 4096 + 64 * 4 + kPadL + kPadR;    // padded rows of a <= 64 x 64 level
constexpr int kTailLL = 1024;                                // the LL of a <= 64 x 64 level

// What a gfx950 workgroup can be given: 160 KiB of LDS.  A level whose band
// of whole rows asks for no more keeps the whole-row kernels (the runtime
// grants a launch up to the device's limit); a wider one goes to the chunked
// instances, whose LDS does not depend on the width (static_asserts below).
constexpr size_t kLdsPerWorkgroup = 160 * 1024;

// dynamic LDS bytes of `rows` staged whole rows of W samples (k_dwt_band:
// kBandRb rows; k_dwt_l1: kRb1 rows of every component) ...
JP2HIP_HD constexpr size_t dwt_rows_lds(int rows, int W) {
    return ((size_t)rows * lds_row_stride(W) + kPadL + kPadR) * 4;
}
// ... of k_dwt_l1s's horizontal batch: kL1sRows rows of each of nc components
JP2HIP_HD constexpr size_t dwt_stream_lds(int nc, int W) {
    return ((size_t)nc * kL1sRows * (kL1sSkew ? lds_row_stride_skew(W) : lds_row_stride(W)) +
            (kL1sSkew ? kPadLs : kPadL) + kPadR) * 4;
}
// ... of the chunked instances (dwt_chunk.h): a chunk's staged rows, whatever
// the level's width
JP2HIP_HD constexpr size_t band_chunk_lds(int rows, int C) { return dwt_rows_lds(rows, dwt_chunk_staged(C)); }
static_assert(band_chunk_lds(kBandRb, kBandChunkW) <= (size_t)kDwtLdsWords * 4,
              "a chunked band fits the default 64 KiB of dynamic LDS");
static_assert(band_chunk_lds(4 * kRb1, kL1ChunkW) <= (size_t)kDwtLdsWordsWide * 4,
              "a chunked level 1 (4 components, the most) fits the 128 KiB the instance opts in to");

enum class DwtForm {
    L1Stream,    // k_dwt_l1s<REV, NC, CPT, kL1sRows, ALIGNED, PX>
    L1Window,    // k_dwt_l1<REV, NC, kRb1>
    L1Chunk,     // k_dwt_l1<REV, NC, kRb1, CHUNK>
    BandIngest,  // k_dwt_band<REV, INGEST, kBandRb>
    Band,        // k_dwt_band<REV, LL, kBandRb, 256 or kBandNarrow>
    BandChunk,   // k_dwt_band<REV, LL, kBandRb, 256, CHUNK>
    Tail,        // k_dwt_tail<REV>: this level and every later one
};

// output rows a workgroup of the form owns (grid x counts them; Tail: the whole level, 0)
JP2HIP_HD constexpr int dwt_form_rows(DwtForm f) {
    return f == DwtForm::L1Stream ? kStreamBand : (f == DwtForm::L1Window || f == DwtForm::L1Chunk) ? kRb1
         : f == DwtForm::Tail ? 0 : kBandRb;
}

// One launch (k_dwt_l1s: one per instance, aligned and ragged tile widths).
struct DwtLevelRoute {
    DwtForm form;
    int level;
    int W, H;      // the widest / tallest tile-component at this level
    int threads;   // per workgroup
    int cpt;       // L1Stream: columns per thread (1, 2 or 4); 0 otherwise
    int gx, gy, gz;  // grid: row bands (Tail: tile-components) x tiles or tile-components x column chunks
    size_t lds;    // dynamic LDS bytes
};

constexpr int kDwtRouteLevels = 12;  // the plan's kMaxLevels
struct DwtRoute {
    int n;                               // launches, in order
    DwtLevelRoute lv[kDwtRouteLevels];
    const char *refused;                 // or why nothing may be launched: lv[n] is then the level at fault
};

JP2HIP_HD constexpr bool dwt_grid_ok(const DwtLevelRoute &r) {
    return r.gx >= 1 && r.gy >= 1 && r.gy <= 65535 && r.gz >= 1 && r.gz <= 65535;
}

// The launches of a `levels`-level DWT of ntc tile-components (nc per tile) in
// planes of plane_w x plane_h samples (the tile size: every tile-component's
// region at level lv is at most ceil(plane / 2^(lv-1)) on a side).
JP2HIP_HD DwtRoute dwt_route(int plane_w, int plane_h, int nc, int ntc, int levels) {
    DwtRoute out;
    out.n = 0;
    out.refused = nullptr;
    if (levels > kDwtRouteLevels) {
        out.lv[0] = DwtLevelRoute{DwtForm::Tail, kDwtRouteLevels + 1, 0, 0, 0, 0, 0, 0, 0, 0};
        out.refused = "DWT: more decomposition levels than a plan holds";
        return out;
    }
    for (int lv = 1; lv <= levels; lv++) {
        DwtLevelRoute &r = out.lv[out.n];
        r.level = lv;
        r.W = (plane_w + (1 << (lv - 1)) - 1) >> (lv - 1);
        r.H = (plane_h + (1 << (lv - 1)) - 1) >> (lv - 1);
        r.threads = kDwtThreads;
        r.cpt = 0;
        r.gz = 1;
        if (lv >= 2 && ((r.W + 1) / 2) * ((r.H + 1) / 2) <= kTailLL &&
            lds_row_stride(r.W) * r.H + kPadL + kPadR <= kTailWords) {
            r.form = DwtForm::Tail;
            r.threads = kTailThreads;
            r.gx = ntc; r.gy = 1;
            r.lds = 0;  // its LDS is static
            out.n++;
            return out;
        }
        // level 1: every component of a tile in one workgroup when its rows
        // fit in LDS (each TIFF pixel read once)
        const bool l1_fits = lv == 1 && dwt_rows_lds(nc * kRb1, r.W) <= (size_t)kDwtLdsWordsWide * 4;
        const bool chunked = !l1_fits && dwt_rows_lds(kBandRb, r.W) > kLdsPerWorkgroup;
        if (l1_fits && r.W <= 4 * kDwtThreads) {
            // streaming vertical pass, bands of kStreamBand rows, horizontal
            // batches of kL1sRows rows
            r.form = DwtForm::L1Stream;
            r.cpt = r.W <= kDwtThreads ? 1 : (r.W <= 2 * kDwtThreads ? 2 : 4);
            r.lds = dwt_stream_lds(nc, r.W);
        } else if (l1_fits) {
            r.form = DwtForm::L1Window;
            r.lds = dwt_rows_lds(nc * kRb1, r.W);
        } else if (chunked) {
            // whole rows of this level do not fit in a workgroup's LDS: column
            // chunks (level 1: every component of a tile per workgroup); grid
            // z = chunks of the widest tile-component
            r.form = lv == 1 ? DwtForm::L1Chunk : DwtForm::BandChunk;
            r.lds = lv == 1 ? band_chunk_lds(nc * kRb1, kL1ChunkW) : band_chunk_lds(kBandRb, kBandChunkW);
            r.gz = dwt_chunk_count(r.W, lv == 1 ? kL1ChunkW : kBandChunkW);
        } else {
            r.form = lv == 1 ? DwtForm::BandIngest : DwtForm::Band;
            if (lv > 1 && r.W <= kBandNarrow) r.threads = kBandNarrow;
            r.lds = dwt_rows_lds(kBandRb, r.W);
        }
        const int rows = dwt_form_rows(r.form);
        r.gx = (r.H + rows - 1) / rows;
        // level 1's own kernels take a tile per workgroup, k_dwt_band a tile-component
        r.gy = (r.form == DwtForm::L1Stream || r.form == DwtForm::L1Window || r.form == DwtForm::L1Chunk) ? ntc / nc : ntc;
        if (chunked && !dwt_grid_ok(r)) {
            out.refused = "DWT: the tile needs more workgroups than a launch takes";
            return out;
        }
        out.n++;
    }
    return out;
}

}  // namespace jp2hip
