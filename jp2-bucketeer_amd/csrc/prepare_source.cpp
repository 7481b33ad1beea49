// prepare_source.cpp -- the source of an encode, brought to what ingest reads.
#include <string>
#include <vector>

#include "context.h"
#include "encode.h"
#include "source_layout.h"

namespace jp2hip {

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
bool prepare_source(jp2hip_ctx *ctx, const UnitGrid &g, const void *&d_src, size_t src_len, const jp2hip_layout *&lay,
                    int row0, int row1, jp2hip_layout &ulay, std::vector<uint64_t> &uoffs, std::string &err) {
    Band band;
    if (!band_walk(*lay, g, row0, row1, src_len, band, err)) return false;
    const bool expand = needs_expand(*lay);
    if (!g.tiled && !g.coded && !expand) return true;
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
    return true;
}

}  // namespace jp2hip
