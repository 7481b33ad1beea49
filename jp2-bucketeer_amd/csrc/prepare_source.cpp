// prepare_source.cpp -- the source of an encode, brought to what ingest reads.
#include <string>
#include <vector>

#include "context.h"
#include "encode.h"
#include "orient_map.h"
#include "source_layout.h"

namespace jp2hip {

namespace {

// S1c: (d_src, lay) -- the whole stored image as uncompressed strips of whole
// samples, the entries of the stored rows behind upright rows [row0, row1)
// valid -- becomes the upright image of TIFF Orientation `orient` (2..8):
// those rows in the context's `oriented` buffer, and a layout of the upright
// width and height over them whose resolution follows the axes.  A plane is
// one strip; a band that starts at row0 > 0 is described by strips of row0
// rows, so that it starts on a strip and no offset lies in front of the copy.
bool orient_source(jp2hip_ctx *ctx, const void *&d_src, const jp2hip_layout *&lay, int row0, int row1, int orient,
                   jp2hip_layout &ulay, std::vector<uint64_t> &uoffs, std::string &err) {
    const jp2hip_layout in = *lay;  // (may be ulay, whose table is uoffs: read before either changes)
    const void *d = nullptr;
    if (!ctx->gpu.orient_samples(d_src, in, orient, row0, row1, ctx->cfg.profile != 0, &d, err)) return false;
    const int64_t planes = in.planar == 2 ? in.components : 1;
    ulay = in;
    oriented_header(ulay, orient);
    const uint64_t row_bytes = (uint64_t)ulay.width * (in.planar == 2 ? 1 : in.components) * (in.bits >> 3);
    const int64_t rps = row0 > 0 ? row0 : ulay.height, per_plane = (ulay.height + rps - 1) / rps;
    uoffs.assign((size_t)(per_plane * planes), 0);
    for (int64_t p = 0; p < planes; p++)
        for (int64_t s = row0 / rps; s <= (row1 - 1) / rps; s++)
            uoffs[(size_t)(p * per_plane + s)] =
                (uint64_t)p * (uint64_t)(row1 - row0) * row_bytes + (uint64_t)(s * rps - row0) * row_bytes;
    ulay.rows_per_strip = (int32_t)rps;
    ulay.nstrips = (int32_t)(per_plane * planes);
    ulay.strip_offsets = uoffs.data();
    ulay.strip_bytes = nullptr;
    d_src = d;
    lay = &ulay;
    return true;
}

}  // namespace

// What every encode does to its source before the front: the units (strips
// or tiles; source_layout.h) that image rows [row0, row1) touch are checked
// against src_len -- they alone must lie inside d_src, so a tile-split rank
// passes its band -- and, unless they are uncompressed strips of whole
// samples, which ingest reads in place, brought to that form in HBM as a
// stand-alone image of the band's rows: decoded (S1a: LZW / Deflate /
// PackBits, tiles untiled), then, for 1-, 2-, 4-bit samples and palette
// indices, expanded to 8 bits (S1b; such tiles stay tiles when decoded, the
// expansion untiles).  Afterwards (d_src, lay) describe the whole image as
// uncompressed strips whose entries outside the band are never read (the
// plan, or a rank's sub-plan, reads only its rows).
// orient = 2..8 (TIFF Orientation; 0 and 1: nothing more is done): [row0,
// row1) are rows of the upright image, the units walked, checked and decoded
// are those of the stored rows behind them (orient_map.h: the mirrored range
// for 3 and 4, every row for 5..8), and S1c runs last (k_orient, orient.hip):
// (d_src, lay) then describe the upright image, its width and height, one
// strip per plane.
bool prepare_source(jp2hip_ctx *ctx, const UnitGrid &g, const void *&d_src, size_t src_len, const jp2hip_layout *&lay,
                    int row0, int row1, jp2hip_layout &ulay, std::vector<uint64_t> &uoffs, std::string &err, int orient) {
    const bool turn = orient >= 2;
    int64_t s0 = row0, s1 = row1;
    if (turn) orient_source_rows(lay->height, lay->width, orient, row0, row1, s0, s1);
    Band band;
    if (!band_walk(*lay, g, s0, s1, src_len, band, err)) return false;
    const bool expand = needs_expand(*lay);
    if (!g.tiled && !g.coded && !expand) {
        if (!turn) return true;
        return orient_source(ctx, d_src, lay, row0, row1, orient, ulay, uoffs, err);
    }
    std::vector<uint64_t> voff, vcnt;
    for (const BandUnit &u : band.units) {
        voff.push_back(u.off);
        vcnt.push_back(u.bytes);
    }
    jp2hip_layout v = *lay;
    v.height = (int32_t)(band.row1 - band.row0);
    v.nstrips = (int32_t)voff.size();
    v.strip_offsets = voff.data();
    v.strip_bytes = vcnt.data();
    UnitGrid gv;
    if (!unit_grid(v, gv, err)) return false;
    jp2hip_layout vu;
    std::vector<uint64_t> vuoffs;
    const jp2hip_layout *cur = &v;
    const void *d = d_src;
    if (g.coded || !expand) {
        if (!ctx->gpu.unpack_strips(d_src, v, gv, vu, vuoffs, &d, err, !expand)) return false;
        cur = &vu;
    }
    int nc, bits;
    encoded_format(*lay, nc, bits);
    if (expand) {
        // the colour table: per encode, never with the cached plan (two files
        // of one geometry have their own maps)
        uint32_t lut[256];
        const bool palette = lay->photometric == JP2HIP_PHOTO_PALETTE;
        if (palette) palette_lut(*lay, lut);
        if (!ctx->gpu.expand_samples(d, *cur, gv, palette ? lut : nullptr, ctx->cfg.profile != 0, &d, err)) return false;
    }
    // the full-image view: unit row u of plane p at its place in the copy
    // (decoded strips stand one per table entry; untiled or expanded rows
    // are row-major per plane)
    const int64_t nu = band.u1 - band.u0;
    const uint64_t img_row = expand ? (uint64_t)lay->width * nc
                                    : packed_row_bytes(lay->width, lay->planar == 2 ? 1 : lay->components, lay->bits);
    uoffs.assign((size_t)(g.urows * g.planes), 0);
    for (int64_t p = 0; p < g.planes; p++)
        for (int64_t u = band.u0; u < band.u1; u++)
            uoffs[(size_t)(p * g.urows + u)] =
                expand    ? (uint64_t)(u - band.u0) * g.unit_h * img_row
                : g.tiled ? vuoffs[(size_t)p] + (uint64_t)(u - band.u0) * g.unit_h * img_row
                          : vuoffs[(size_t)(p * nu + (u - band.u0))];
    ulay = *lay;
    ulay.rows_per_strip = (int32_t)g.unit_h;
    ulay.nstrips = (int32_t)(g.urows * g.planes);
    ulay.strip_offsets = uoffs.data();
    ulay.compression = 1;
    ulay.predictor = 1;
    ulay.strip_bytes = nullptr;
    ulay.tile_width = ulay.tile_height = 0;
    if (expand) {  // 8-bit grey or chunky RGB
        ulay.components = nc;
        ulay.bits = bits;
        ulay.planar = 1;
        ulay.photometric = JP2HIP_PHOTO_DEFAULT;
        ulay.fill_order = 0;
        ulay.colormap = nullptr;
        ulay.colormap_entries = 0;
    }
    d_src = d;
    lay = &ulay;
    return !turn || orient_source(ctx, d_src, lay, row0, row1, orient, ulay, uoffs, err);
}

}  // namespace jp2hip
