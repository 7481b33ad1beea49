// stages.h -- what the stage files export to GpuEncoder's members: argument
// structs and launchers of the strip decoders (unpack.hip, lzw.hip), the
// sample expansion (expand.hip), the orientation (orient.hip), the fused
// ingest + DWT (dwt.hip) and tier-1 (t1.hip).  Argument structs that only one file uses stay in that file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "jp2hip_internal.h"

namespace jp2hip {

#include "unpack_args.h"
// LZW strips, segment-parallel (lzw.hip): lzw_slices() lays out each
// strip's segment slots (returns their total), the caller uploads `slice` to
// the start of `scratch` (lzw_scratch_bytes); false on a launch error
uint64_t lzw_slices(const uint64_t *strip_bytes, int nstrips, std::vector<uint64_t> &slice);
size_t lzw_scratch_bytes(int nstrips, uint64_t segs);
bool launch_lzw(const UnpackArgs &u, uint64_t segs, void *scratch, hipStream_t st);

// S1b sample expansion (expand.hip): packed 1-, 2-, 4-bit samples or palette
// indices (1, 2, 4, 8 bits), one sample per pixel, in strips or tiles ->
// row-major 8-bit samples, grey or chunky RGB.  Unit u (strip, or tile in
// row-major tile order) starts at src + off[u]; its rows are row_bytes apart.
struct ExpandArgs {
    const uint8_t *src;
    const uint64_t *off;   // [units] device table
    int w, rows;           // pixels per output row, output rows
    int unit_w, unit_h;    // pixels per unit row (w for strips), rows per unit
    int across;            // units side by side (1 for strips)
    uint32_t row_bytes;    // ceil(unit_w * bits / 8)
    int lsb_first;         // FillOrder 2: the bits of every source byte reversed first
    uint32_t invert;       // WhiteIsZero: 0xFFFFFFFF, XORed onto every output dword (else 0)
    const uint32_t *lut;   // palette: [2^bits] dwords R | G << 8 | B << 16
    uint8_t *dst;          // rows * w bytes (grey), rows * w * 3 (palette)
};
// false: bits is not 1, 2, 4 (or 8 with a palette), or a launch error
bool launch_expand(const ExpandArgs &a, int bits, bool palette, hipStream_t st);

// S1c orientation (orient.hip): uncompressed strips of whole-byte elements (a
// pixel of a chunky source, a sample of a planar one) -> upright rows [row0,
// row1) of the image under TIFF Orientation o (orient_map.h), row-major, one
// run of rows per plane.  Row y of plane p starts at
// src + off[p * spp_strips + y / rps] + (y % rps) * w * es.
struct OrientArgs {
    const uint8_t *src;
    const uint64_t *off;   // [planes * spp_strips] device table
    int w, h;              // the stored image: elements per row, rows
    int o;                 // 2..8
    int rps, spp_strips, planes;
    int row0, row1;        // upright rows written: dst row 0 is upright row row0
    uint8_t *dst;          // planes * (row1 - row0) * upright width * es bytes
};
constexpr int kOrientTile = 64;  // the transposing form's tile: 64 x 64 elements
// false: es is not 1, 2, 3, 4, 6 or 8, o is not 2..8, a grid dimension is out
// of range, or a launch error
bool launch_orient(const OrientArgs &a, int es, hipStream_t st);

// the SDMA engines chosen per GPU and their probed rates (t2_device.hip)
std::string dma_engine_report();

// tier-1 kernels (t1.hip)
#ifndef JP2HIP_ORDER_SUB
#define JP2HIP_ORDER_SUB 16  // MQ lane-order buckets per octave of decision count
#endif
constexpr int kOrderSub = JP2HIP_ORDER_SUB;
constexpr int kOrderBuckets = 32 * kOrderSub;  // MQ lane-order buckets (decision count, 6.25 % wide)
// Work lists of k_t1_cm3, filled once the coded planes are known
// (emit_t1_items: k_plane_pmin, or k_t1_items without slope prediction):
// list k holds the blocks with more than k coded planes (item = plane k from
// the top of that block), in no particular order.
struct T1ItemArgs {
    int nb, kmax;               // kmax: largest Mb of the plan (<= 64)
    const uint8_t *P;
    uint8_t *pmin;              // k_t1_items writes 0 (every plane coded)
    uint32_t *dfill;            // [64] list fills (zeroed by k_quant)
    int32_t *dlist;             // [kmax][nb]
    unsigned long long *acc;    // [nb] (coded planes << 40): k_t1_cm3 counts planes down, decisions up
    uint8_t *npasses;           // blocks without a coded plane: 0 passes, 0 bytes (k_t1_mq never sees them)
    int32_t *lengths;
    // decision-stream slots, placed here (emit_t1_items)
    const BlockDesc *blocks;
    unsigned long long *pool_used;  // zeroed by k_quant; ends at the bytes needed
    unsigned long long pool_cap;    // bytes in the pool (stream_buf)
    uint64_t *slot_off;             // [nb]
    int *err;                       // kErrSlotPool when a block did not fit
};
struct T1CmArgs {
    const uint32_t *dfill;  // per-depth list fills
    const int32_t *dlist;
    int nb, kmax;
    int max_items;          // bound on the items (nb * kmax): the grid
    const BlockDesc *blocks;
    const uint64_t *bp;
    const int32_t *sm;
    const uint8_t *P;
    uint8_t *stream;
    const uint64_t *slot_off;
    uint4 *counts;    // [block][32] (end of SPP, end of MRP, end of CUP)
    int64_t *dspp;    // [block][32]
    unsigned long long *acc;  // [block] (planes left << 40) | decisions so far
    uint32_t *bfill;          // [256] MQ lane-order bucket fills (zeroed by k_quant)
    int32_t *bslots;          // [256][nb] blocks per bucket
    int lossless;
};
struct T1MqArgs {
    const BlockDesc *blocks;
    const uint32_t *bfill;   // lane order: bucket fills and members (k_t1_cm3)
    const int32_t *bslots;
    int nblocks;
    const uint8_t *P;
    const uint8_t *pmin;  // lowest coded plane (slope prediction; 0 = all)
    const uint8_t *stream;
    const uint64_t *slot_off;
    const uint4 *counts;
    const int64_t *dspp, *dref, *dsig;
    uint8_t *out;
    int32_t *rates;
    int64_t *dists;
    uint8_t *npasses;
    int32_t *lengths;
    int *err;
    unsigned long long *span;  // [2] execution span in 100 MHz ticks (~min start, max end)
    int64_t *dbg;  // optional per-block census [block][6] (debug builds: decisions, modeller cycles
                   // and barrier cycles, coder cycles and barrier cycles, lane position)
};
// fused ingest + DWT (dwt.hip)
struct DwtLaunch {
    const void *tif;
    const uint64_t *strip_off;
    int rps, img_w, nc, bits, planar, big_endian, mct, spp_strips;
    int ntx, tile_w, tile_h, row0, plane_w, plane_h, ntc, levels, reversible;
    int last_tile_w;  // width of the last tile column (the others are tile_w)
    uint64_t src_end;  // end of the last source byte the plan's rows hold (dwt_fetch.h: no access ends beyond it)
    const int32_t *tc_w, *tc_h;
    void *coef, *scratch0, *scratch1;  // scratch: ntc * ceil(plane_w/2) * ceil(plane_h/2) words each
    QuantTab qt;                       // final coefficients are written as quantisation indices
};
// false: a launch failed, or (*why set) one was refused before it was made
bool launch_dwt(const DwtLaunch &p, hipStream_t st, const char **why = nullptr);

void launch_t1_cm(const T1CmArgs &a, hipStream_t st);
void launch_t1_items(const T1ItemArgs &a, hipStream_t st);
void launch_t1_mq(const T1MqArgs &a, hipStream_t st);
uint32_t t1_plane_stream_cap(int w, int h);
}  // namespace jp2hip
