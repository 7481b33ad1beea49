// source_layout.h -- which bytes of a source buffer hold the image: the
// baseline TIFF parser, the pixel-format rules, and the one description of a
// layout's unit grid (strips or tiles) and of the units a band of rows reads.
// Every path that hands a jp2hip_layout to a kernel (prepare_source.cpp,
// the encode_file split path, GpuEncoder::unpack_strips / expand_samples)
// takes its geometry and its bounds checks from here.  Host-only: jp2hip.h
// and the standard library, so the CPU suite builds it under ASan / UBSan
// (tests/host/test_source_layout.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "jp2hip.h"

namespace jp2hip {

// Baseline TIFF header parsing (tags 256-339; classic TIFF and BigTIFF).
// `offs` receives the strip table `lay` points into; icc and colormap point
// into `buf`.  false: `err` says why ("tiff: ...").
bool parse_tiff(const uint8_t *buf, size_t len, jp2hip_layout *lay, std::vector<uint64_t> &offs, std::string &err);

// Bytes of a row of `w` pixels: rows start on byte boundaries, samples below
// 8 bits are packed (TIFF 6.0 section 3 and 5).
inline uint64_t packed_row_bytes(uint64_t w, uint64_t spp, uint64_t bits) { return (w * spp * bits + 7) / 8; }

// Sources whose samples are expanded to 8 bits in HBM before ingest
// (expand.hip): 1-, 2- and 4-bit grey and palette colour.
inline bool needs_expand(const jp2hip_layout &lay) { return lay.bits < 8 || lay.photometric == JP2HIP_PHOTO_PALETTE; }

// What the code-stream carries for this source (jp2hip_encoded_format).
void encoded_format(const jp2hip_layout &lay, int &nc, int &bits);

// TIFF Orientation (tag 274) of a file: the tag's value when it is one SHORT
// in 1..8, 1 when the tag is absent or malformed (a metadata tag never fails
// a parse) or the IFD cannot be walked, < 0 when `buf` is no TIFF at all.
int tiff_orientation(const uint8_t *buf, size_t len);

// What the upright image of orientation `o` keeps of a layout that describes
// the stored one: for 5..8 width and height change places, and X and Y
// resolution with them.  (The strips still describe the stored image.)
inline void oriented_header(jp2hip_layout &l, int o) {
    if (o < 5 || o > 8) return;
    std::swap(l.width, l.height);
    std::swap(l.xres_num, l.yres_num);
    std::swap(l.xres_den, l.yres_den);
}

// The pixel format of a layout, the parser's or a caller's: the depths,
// component counts and photometric forms the encoder has a path for.
bool check_pixel_format(const jp2hip_layout *lay, std::string &err);

// The colour table of a palette layout as k_expand reads it: entry i is
// R | G << 8 | B << 16.  ColorMap values are 16-bit (a component is the high
// byte) unless no entry exceeds 255: such maps, from old writers, hold 8-bit
// values and are taken as they are (libtiff's checkcmap).
void palette_lut(const jp2hip_layout &lay, uint32_t *lut);

// The units of a layout: strips (one across, clipped at the image's last
// row) or tiles (never clipped), row-major per plane; unit (p, u, x) is
// entry p * per_plane + u * across + x of the strip table.
struct UnitGrid {
    bool tiled = false;
    bool coded = false;                  // compression > 1: a unit is strip_bytes[i] bytes, read whole
    int64_t unit_w = 0, unit_h = 0;      // pixels per unit row, rows per unit
    int64_t planes = 0;                  // planar 2: one per component
    int64_t across = 0, urows = 0;       // units side by side, unit rows per plane
    int64_t per_plane = 0, needed = 0;   // across * urows, and that times planes
    uint64_t row_bytes = 0;              // bytes of one row of a unit
    uint64_t unit_bytes = 0;             // bytes of a whole uncompressed unit: unit_h * row_bytes
};
// The arithmetic alone, for a geometry already known to be positive.
UnitGrid grid_of(const jp2hip_layout &lay);
// The grid of a layout that passes check_pixel_format, has a positive
// geometry, a known compression code, the tables its form needs and at
// least `needed` entries in them.  false: `err` says why ("layout: ...").
bool unit_grid(const jp2hip_layout &lay, UnitGrid &g, std::string &err);

// The units that image rows [row0, row1) touch, in plane / unit-row / across
// order.  Each lies inside a buffer of `len` bytes, and an uncompressed one
// holds the rows read of it (a whole tile; a strip's rows inside the image).
// Units outside the band are not looked at.
struct BandUnit {
    size_t idx;           // entry of the strip table
    uint64_t off, bytes;  // uncompressed strips: the bytes of its rows, by the geometry
};
struct Band {
    int64_t u0 = 0, u1 = 0;      // unit rows [u0, u1) of every plane
    int64_t row0 = 0, row1 = 0;  // the image rows those hold: [u0 * unit_h, min(height, u1 * unit_h))
    std::vector<BandUnit> units;
};
// An empty row range yields no units; a non-empty one that holds no row of
// the image is an error ("layout: empty band").
bool band_walk(const jp2hip_layout &lay, const UnitGrid &g, int64_t row0, int64_t row1, uint64_t len, Band &band,
               std::string &err);

}  // namespace jp2hip
