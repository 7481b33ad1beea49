// source_layout.cpp -- the TIFF parser, the pixel-format rules, the unit
// grid and the band walk (source_layout.h).  No HIP in here.
#include "source_layout.h"

#include <algorithm>
#include <climits>

namespace jp2hip {

namespace {

// a * b, or the largest value when the product does not fit (a geometry that
// large fits no buffer, so every bounds check against it then fails)
uint64_t mul_sat(uint64_t a, uint64_t b) { return b && a > UINT64_MAX / b ? UINT64_MAX : a * b; }

bool known_compression(int32_t c) { return c <= 1 || c == 5 || c == 8 || c == 32946 || c == 32773; }

// ---- baseline TIFF header parsing (tags 256-339; classic TIFF and BigTIFF) ----
struct TiffReader {
    const uint8_t *b;
    size_t n;
    bool le;
    bool big = false;  // BigTIFF: 8-byte offsets, 20-byte IFD entries
    uint64_t un(size_t o, int k) const {
        if (o + (size_t)k > n || o + (size_t)k < o) return 0;
        uint64_t v = 0;
        for (int i = 0; i < k; i++) v |= (uint64_t)b[o + (le ? i : k - 1 - i)] << (8 * i);
        return v;
    }
    uint32_t u16(size_t o) const { return (uint32_t)un(o, 2); }
    uint32_t u32(size_t o) const { return (uint32_t)un(o, 4); }
    uint64_t u64(size_t o) const { return un(o, 8); }
    size_t entry_size() const { return big ? 20 : 12; }
    uint64_t count(size_t e) const { return big ? u64(e + 4) : u32(e + 4); }
    // value i of the entry at e (SHORT, LONG, LONG8 or BYTE)
    uint64_t val(size_t e, uint64_t i) const {
        const uint32_t type = u16(e + 2);
        const uint64_t cnt = count(e);
        const uint32_t sz = type == 3 ? 2 : (type == 4 ? 4 : (type == 16 ? 8 : 1));
        const size_t inl = big ? 8 : 4, voff = big ? e + 12 : e + 8;
        const uint64_t base = (uint64_t)sz * cnt <= inl ? voff : (big ? u64(voff) : u32(voff));
        if (i >= cnt) return 0;
        const size_t at = (size_t)(base + (uint64_t)sz * i);
        return sz == 2 ? u16(at) : (sz == 4 ? u32(at) : (sz == 8 ? u64(at) : (at < n ? b[at] : 0)));
    }
    // Metadata tags (ICC profile, ExtraSamples, resolution): where the
    // entry's `cnt` values of `sz` bytes lie, or false when they do not lie
    // inside the file -- such a tag counts as absent, it never fails the parse.
    bool data_at(size_t e, uint32_t sz, uint64_t cnt, size_t &at) const {
        const size_t inl = big ? 8 : 4, voff = big ? e + 12 : e + 8;
        if (cnt == 0 || cnt > n / sz) return false;
        const uint64_t bytes = (uint64_t)sz * cnt;
        const uint64_t base = bytes <= inl ? voff : (big ? u64(voff) : u32(voff));
        if (base > n || bytes > n - base) return false;
        at = (size_t)base;
        return true;
    }
    // the first value of a RATIONAL entry (two LONGs: numerator, denominator)
    bool rational(size_t e, uint32_t &num, uint32_t &den) const {
        size_t at;
        if (u16(e + 2) != 5 || !data_at(e, 8, count(e), at)) return false;
        num = u32(at);
        den = u32(at + 4);
        return true;
    }
};

// The file header: the byte order, classic TIFF or BigTIFF, where the first
// IFD's entries start and how many it holds.  0, or (err says why) 1: not a
// TIFF at all, 2: a TIFF whose first IFD does not lie inside the file.
int open_ifd(TiffReader &t, size_t &first, uint64_t &ne, std::string &err) {
    auto fail = [&err](int rc, const char *msg) {
        err = msg;
        return rc;
    };
    const uint8_t *buf = t.b;
    const size_t len = t.n;
    if (!buf || len < 8) return fail(1, "tiff: input too short");
    if (buf[0] == 'I' && buf[1] == 'I') t.le = true;
    else if (buf[0] == 'M' && buf[1] == 'M') t.le = false;
    else return fail(1, "tiff: bad byte-order mark");
    size_t ifd, ifd_hdr;
    if (t.u16(2) == 43) {  // BigTIFF: offset size 8, reserved 0, first IFD at 8
        if (t.u16(4) != 8 || t.u16(6) != 0 || len < 16) return fail(1, "tiff: bad BigTIFF header");
        t.big = true;
        ifd = (size_t)t.u64(8);
        ifd_hdr = 8;
    } else if (t.u16(2) == 42) {
        ifd = t.u32(4);
        ifd_hdr = 2;
    } else {
        return fail(1, "tiff: not a TIFF file");
    }
    if (ifd + ifd_hdr > len || ifd + ifd_hdr < ifd) return fail(2, "tiff: IFD offset out of range");
    ne = t.big ? t.u64(ifd) : t.u16(ifd);
    first = ifd + ifd_hdr;
    if (ne > (len - first) / t.entry_size()) return fail(2, "tiff: truncated IFD");
    return 0;
}

}  // namespace

int tiff_orientation(const uint8_t *buf, size_t len) {
    TiffReader t{buf, len, true};
    size_t first;
    uint64_t ne;
    std::string err;
    const int rc = open_ifd(t, first, ne, err);
    if (rc) return rc == 1 ? -1 : 1;
    int o = 1;
    for (uint64_t i = 0; i < ne; i++) {
        const size_t e = first + t.entry_size() * (size_t)i;
        if (t.u16(e) != 274) continue;
        size_t at;
        const uint32_t v = t.u16(e + 2) == 3 && t.count(e) == 1 && t.data_at(e, 2, 1, at) ? t.u16(at) : 0;
        o = v >= 1 && v <= 8 ? (int)v : 1;
    }
    return o;
}

bool parse_tiff(const uint8_t *buf, size_t len, jp2hip_layout *lay, std::vector<uint64_t> &offs, std::string &err) {
    auto fail = [&err](const std::string &msg) {
        err = msg;
        return false;
    };
    TiffReader t{buf, len, true};
    size_t first;
    uint64_t ne;
    if (open_ifd(t, first, ne, err)) return false;
    uint32_t w = 0, h = 0, spp = 1, bps = 8, comp = 1, planar = 1, rps = 0xFFFFFFFFu, fmt = 1, pred = 1;
    uint32_t photo = 0xFFFFFFFFu;  // absent: inferred from SamplesPerPixel
    uint32_t fill = 1;             // FillOrder: MSB-first when absent
    size_t e_off = 0, e_cnt = 0, e_cmap = 0;
    uint64_t n_off = 0;  // entries of the offsets tag, as far as a layout can count them
    uint32_t tw = 0, th = 0;
    // what the file states about its pixels (the JP2 / JPX header carries it):
    // a malformed one of these tags is an absent one
    int32_t extra = 0;       // ExtraSamples value + 1; 0 absent
    uint32_t res_unit = 2;   // ResolutionUnit: inch when absent
    uint32_t xr[2] = {0, 0}, yr[2] = {0, 0};
    const uint8_t *icc = nullptr;
    uint64_t icc_bytes = 0;
    for (uint64_t i = 0; i < ne; i++) {
        size_t e = first + t.entry_size() * (size_t)i;
        switch (t.u16(e)) {
        case 256: w = (uint32_t)t.val(e, 0); break;
        case 257: h = (uint32_t)t.val(e, 0); break;
        case 258: bps = (uint32_t)t.val(e, 0); break;
        case 259: comp = (uint32_t)t.val(e, 0); break;
        case 262: photo = (uint32_t)t.val(e, 0); break;
        case 266: fill = (uint32_t)t.val(e, 0); break;
        case 320: e_cmap = e; break;  // ColorMap
        case 273: e_off = e; n_off = std::min<uint64_t>(t.count(e), INT32_MAX); break;
        case 277: spp = (uint32_t)t.val(e, 0); break;
        case 278: rps = (uint32_t)std::min<uint64_t>(t.val(e, 0), 0xFFFFFFFFu); break;
        case 279: e_cnt = e; break;
        case 284: planar = (uint32_t)t.val(e, 0); break;
        case 317: pred = (uint32_t)t.val(e, 0); break;
        case 322: tw = (uint32_t)t.val(e, 0); break;
        case 323: th = (uint32_t)t.val(e, 0); break;
        case 324: e_off = e; n_off = std::min<uint64_t>(t.count(e), INT32_MAX); break;  // TileOffsets
        case 325: e_cnt = e; break;                                                      // TileByteCounts
        case 339: fmt = (uint32_t)t.val(e, 0); break;
        case 282: if (!t.rational(e, xr[0], xr[1])) xr[0] = xr[1] = 0; break;  // XResolution
        case 283: if (!t.rational(e, yr[0], yr[1])) yr[0] = yr[1] = 0; break;  // YResolution
        case 296: {                                                            // ResolutionUnit
            size_t at;
            res_unit = (t.u16(e + 2) == 3 && t.data_at(e, 2, t.count(e), at)) ? t.u16(at) : 0;
            break;
        }
        case 338: {  // ExtraSamples: the first value; an unknown one reads as 0 (unspecified)
            size_t at;
            extra = 0;
            if (t.u16(e + 2) == 3 && t.data_at(e, 2, t.count(e), at)) extra = 1 + (int32_t)(t.u16(at) <= 2 ? t.u16(at) : 0);
            break;
        }
        case 34675: {  // ICCProfile: recorded raw, classified when the header is written
            size_t at;
            const uint32_t type = t.u16(e + 2);
            icc = nullptr;
            icc_bytes = 0;
            if ((type == 7 || type == 1) && t.data_at(e, 1, t.count(e), at)) {
                icc = buf + at;
                icc_bytes = t.count(e);
            }
            break;
        }
        default: break;
        }
    }
    if (!w || !h || !e_off) return fail("tiff: missing ImageWidth/ImageLength/StripOffsets");
    if (w > (uint32_t)INT32_MAX || h > (uint32_t)INT32_MAX) return fail("tiff: ImageWidth/ImageLength out of range");
    const bool tiled = tw || th;
    if (tiled && (!tw || !th || (tw % 16) || (th % 16) || tw > 65536 || th > 65536))
        return fail("tiff: bad TileWidth/TileLength");
    if (tiled && !e_cnt) return fail("tiff: tiles need TileByteCounts");
    // strips: uncompressed, LZW, Deflate or PackBits (decoded on the GPU,
    // lzw.hip, unpack.hip k_inflate / k_unpackbits); JPEG / CCITT are not
    if (comp != 1 && comp != 5 && comp != 8 && comp != 32946 && comp != 32773)
        return fail("tiff: compression " + std::to_string(comp) +
                    " is not supported (uncompressed, LZW, Deflate and PackBits only)");
    if (pred != 1 && pred != 2) return fail("tiff: predictor " + std::to_string(pred) + " is not supported");
    if (pred == 2 && comp == 1) return fail("tiff: predictor 2 without compression is not supported");
    if (comp != 1 && !e_cnt) return fail("tiff: compressed strips need StripByteCounts");
    if (bps != 1 && bps != 2 && bps != 4 && bps != 8 && bps != 16)
        return fail("tiff: " + std::to_string(bps) + " bits/sample is not supported");
    if (bps < 8 && spp != 1)
        return fail("tiff: " + std::to_string(bps) + " bits/sample with " + std::to_string(spp) +
                    " samples/pixel is not supported (packed samples: one per pixel only)");
    if (bps < 8 && pred == 2)
        return fail("tiff: predictor 2 with " + std::to_string(bps) + " bits/sample is not supported");
    if (bps < 8 && fill != 1 && fill != 2) return fail("tiff: FillOrder " + std::to_string(fill) + " is not supported");
    if (fmt != 1) return fail("tiff: only unsigned integer samples are supported");
    if (spp < 1 || spp > 4) return fail("tiff: " + std::to_string(spp) + " samples/pixel is not supported");
    if (planar != 1 && planar != 2) return fail("tiff: bad PlanarConfiguration");
    // PhotometricInterpretation: BlackIsZero gray (+ alpha) or RGB (+ alpha);
    // the colour transform assumes RGB in components 0..2
    if (photo == 0xFFFFFFFFu) photo = spp >= 3 ? 2 : 1;
    // WhiteIsZero: the 1-, 2- and 4-bit forms only (bilevel scans; expanded and
    // inverted by k_expand)
    if (photo == 0 && bps >= 8) return fail("tiff: PhotometricInterpretation 0 (WhiteIsZero) is not supported");
    const uint8_t *cmap = nullptr;
    if (photo == 3) {  // palette colour: indices of 1, 2, 4 or 8 bits and a whole ColorMap
        if (spp != 1) return fail("tiff: PhotometricInterpretation 3 (palette) needs 1 sample/pixel");
        if (bps > 8)
            return fail("tiff: PhotometricInterpretation 3 (palette) with " + std::to_string(bps) +
                        "-bit indices is not supported");
        if (!e_cmap) return fail("tiff: PhotometricInterpretation 3 (palette) without a ColorMap is not supported");
        size_t at;
        if (t.u16(e_cmap + 2) != 3 || t.count(e_cmap) != (3ull << bps) || !t.data_at(e_cmap, 2, 3ull << bps, at))
            return fail("tiff: PhotometricInterpretation 3 (palette): the ColorMap must be 3 * 2^" +
                        std::to_string(bps) + " SHORTs inside the file");
        cmap = buf + at;
    } else if (photo != 0 && photo != 1 && photo != 2) {
        return fail("tiff: PhotometricInterpretation " + std::to_string(photo) +
                    " is not supported (gray, RGB or palette only)");
    }
    if (photo == 0 && spp != 1) return fail("tiff: WhiteIsZero with more than 1 sample/pixel is not supported");
    if (photo == 2 && spp < 3) return fail("tiff: RGB needs 3 or 4 samples/pixel");
    if (photo == 1 && spp > 2) return fail("tiff: BlackIsZero with more than 2 samples/pixel is not supported");
    if (rps == 0 && !tiled) rps = h;  // RowsPerStrip 0 is invalid; libtiff reads it as one strip
    if (rps > h) rps = h;
    if (tiled) rps = th;  // per-unit rows (tiles are never clipped)
    jp2hip_layout L{};
    L.width = (int32_t)w;
    L.height = (int32_t)h;
    L.components = (int32_t)spp;
    L.bits = (int32_t)bps;
    L.planar = (int32_t)planar;
    L.big_endian = t.le ? 0 : 1;
    L.rows_per_strip = (int32_t)rps;
    L.compression = (int32_t)comp;
    L.predictor = (int32_t)pred;
    L.tile_width = (int32_t)tw;
    L.tile_height = (int32_t)th;
    const UnitGrid g = grid_of(L);
    const uint64_t need = (uint64_t)g.needed;
    if (n_off < need) return fail(tiled ? "tiff: too few tiles" : "tiff: too few strips");
    const bool packed = g.coded || g.tiled;
    offs.resize(packed ? 2 * (size_t)need : (size_t)need);
    for (uint64_t s = 0; s < need; s++) {
        offs[s] = t.val(e_off, s);
        if (packed) {
            const uint64_t nb = t.val(e_cnt, s);
            if (offs[s] > len || nb > len - offs[s]) return fail("tiff: strip " + std::to_string(s) + " out of range");
            if (tiled && comp == 1 && nb < g.unit_bytes) return fail("tiff: tile byte count too small");
            offs[need + s] = nb;
            continue;
        }
        const uint64_t y0 = (s % (uint64_t)g.per_plane) * rps;
        const uint64_t bytes = mul_sat(std::min<uint64_t>(rps, h - y0), g.row_bytes);
        if (offs[s] > len || bytes > len - offs[s]) return fail("tiff: strip " + std::to_string(s) + " out of range");
        if (e_cnt && t.val(e_cnt, s) < bytes) return fail("tiff: strip byte count too small");
    }
    L.nstrips = (int32_t)need;
    L.strip_offsets = offs.data();
    L.strip_bytes = packed ? offs.data() + need : nullptr;
    // a resolution needs both rationals whole and a unit (1 "none" is kept
    // as stated; the header writes a res box for inch and centimetre only)
    const bool res = xr[0] && xr[1] && yr[0] && yr[1] && res_unit >= 1 && res_unit <= 3;
    L.extra_samples = extra;
    L.res_unit = res ? (int32_t)res_unit : 0;
    L.xres_num = res ? xr[0] : 0;
    L.xres_den = res ? xr[1] : 0;
    L.yres_num = res ? yr[0] : 0;
    L.yres_den = res ? yr[1] : 0;
    L.icc = icc;
    L.icc_bytes = icc_bytes;
    L.photometric = photo == 3 ? JP2HIP_PHOTO_PALETTE : (photo == 0 ? JP2HIP_PHOTO_WHITE_IS_ZERO : JP2HIP_PHOTO_DEFAULT);
    L.fill_order = bps < 8 ? (int32_t)fill : 0;
    L.colormap = cmap;
    L.colormap_entries = cmap ? (3ull << bps) : 0;
    *lay = L;
    return true;
}

void encoded_format(const jp2hip_layout &lay, int &nc, int &bits) {
    nc = lay.photometric == JP2HIP_PHOTO_PALETTE ? 3 : lay.components;
    bits = needs_expand(lay) ? 8 : lay.bits;
}

bool check_pixel_format(const jp2hip_layout *lay, std::string &err) {
    const int b = lay->bits;
    if (b != 1 && b != 2 && b != 4 && b != 8 && b != 16) {
        err = "layout: " + std::to_string(b) + " bits/sample is not supported";
        return false;
    }
    if (lay->components < 1 || lay->components > 4 || (lay->planar != 1 && lay->planar != 2)) {
        err = "layout: bad geometry or strip table";
        return false;
    }
    if (lay->photometric != JP2HIP_PHOTO_DEFAULT && lay->photometric != JP2HIP_PHOTO_WHITE_IS_ZERO &&
        lay->photometric != JP2HIP_PHOTO_PALETTE) {
        err = "layout: unknown photometric " + std::to_string(lay->photometric);
        return false;
    }
    if (b < 8 && lay->components != 1) {
        err = "layout: samples below 8 bits need 1 component";
        return false;
    }
    if (b < 8 && (lay->fill_order < 0 || lay->fill_order > 2)) {
        err = "layout: fill_order must be 0, 1 or 2";
        return false;
    }
    if (b < 8 && lay->predictor == 2) {
        err = "layout: predictor 2 with samples below 8 bits is not supported";
        return false;
    }
    if (lay->photometric == JP2HIP_PHOTO_WHITE_IS_ZERO && (b >= 8 || lay->components != 1)) {
        err = "layout: photometric WhiteIsZero is supported for 1 component of 1, 2 or 4 bits only";
        return false;
    }
    if (lay->photometric == JP2HIP_PHOTO_PALETTE &&
        (b > 8 || lay->components != 1 || !lay->colormap || lay->colormap_entries != (3ull << b))) {
        err = "layout: photometric palette needs 1 component of 1, 2, 4 or 8 bits and a colormap of 3 * 2^bits entries";
        return false;
    }
    if (needs_expand(*lay) && lay->tile_width > 0 && lay->tile_width % 16) {
        err = "layout: tiles of packed samples or palette indices need a tile_width in multiples of 16";
        return false;
    }
    return true;
}

void palette_lut(const jp2hip_layout &lay, uint32_t *lut) {
    const int n = 1 << lay.bits;
    auto entry = [&](int i) -> uint32_t {
        const uint8_t *p = lay.colormap + 2 * (size_t)i;
        return lay.big_endian ? ((uint32_t)p[0] << 8) | p[1] : p[0] | ((uint32_t)p[1] << 8);
    };
    bool wide = false;
    for (int i = 0; i < 3 * n; i++) wide = wide || entry(i) > 255;
    const int sh = wide ? 8 : 0;
    for (int i = 0; i < n; i++)
        lut[i] = (entry(i) >> sh) | ((entry(n + i) >> sh) << 8) | ((entry(2 * n + i) >> sh) << 16);
}

UnitGrid grid_of(const jp2hip_layout &lay) {
    UnitGrid g;
    g.tiled = lay.tile_width > 0;
    g.coded = lay.compression > 1;
    g.unit_w = g.tiled ? lay.tile_width : lay.width;
    g.unit_h = g.tiled ? lay.tile_height : lay.rows_per_strip;
    g.planes = lay.planar == 2 ? lay.components : 1;
    g.across = g.tiled ? ((int64_t)lay.width + g.unit_w - 1) / g.unit_w : 1;
    g.urows = ((int64_t)lay.height + g.unit_h - 1) / g.unit_h;
    g.per_plane = g.across * g.urows;  // (< 2^62)
    g.needed = g.per_plane > INT64_MAX / g.planes ? INT64_MAX : g.per_plane * g.planes;
    g.row_bytes = packed_row_bytes((uint64_t)g.unit_w, lay.planar == 2 ? 1 : (uint64_t)lay.components, (uint64_t)lay.bits);
    g.unit_bytes = mul_sat((uint64_t)g.unit_h, g.row_bytes);
    return g;
}

bool unit_grid(const jp2hip_layout &lay, UnitGrid &g, std::string &err) {
    if (!check_pixel_format(&lay, err)) return false;
    const bool tiled = lay.tile_width > 0 || lay.tile_height > 0;
    if (tiled && (lay.tile_width <= 0 || lay.tile_height <= 0)) {
        err = "layout: tiles need both tile_width and tile_height";
        return false;
    }
    if (lay.width <= 0 || lay.height <= 0 || (!tiled && lay.rows_per_strip <= 0) || lay.nstrips <= 0) {
        err = "layout: bad geometry or strip table";
        return false;
    }
    if (!known_compression(lay.compression)) {
        err = "layout: compression " + std::to_string(lay.compression) + " is not supported";
        return false;
    }
    if (!lay.strip_offsets) {
        err = "layout: bad geometry or strip table (no strip_offsets)";
        return false;
    }
    if ((tiled || lay.compression > 1) && !lay.strip_bytes) {
        err = "layout: compressed strips and tiles need strip_bytes";
        return false;
    }
    g = grid_of(lay);
    if (g.needed > lay.nstrips) {
        err = tiled ? "layout: too few tiles" : "layout: too few strips";
        return false;
    }
    return true;
}

bool band_walk(const jp2hip_layout &lay, const UnitGrid &g, int64_t row0, int64_t row1, uint64_t len, Band &band,
               std::string &err) {
    band = Band{};
    if (row1 <= row0) return true;
    const int64_t r0 = std::max<int64_t>(0, row0), r1 = std::min<int64_t>(row1, lay.height);
    if (r1 <= r0) {
        err = "layout: empty band";
        return false;
    }
    band.u0 = r0 / g.unit_h;
    band.u1 = (r1 + g.unit_h - 1) / g.unit_h;
    band.row0 = band.u0 * g.unit_h;
    band.row1 = std::min<int64_t>(lay.height, band.u1 * g.unit_h);
    band.units.reserve((size_t)(g.planes * (band.u1 - band.u0) * g.across));
    for (int64_t p = 0; p < g.planes; p++)
        for (int64_t u = band.u0; u < band.u1; u++)
            for (int64_t x = 0; x < g.across; x++) {
                const size_t i = (size_t)(p * g.per_plane + u * g.across + x);
                // what is read of an uncompressed unit; a compressed one is read whole
                const uint64_t rows = (uint64_t)(g.tiled ? g.unit_h : std::min(g.unit_h, lay.height - u * g.unit_h));
                const uint64_t want = mul_sat(rows, g.row_bytes);
                const uint64_t o = lay.strip_offsets[i], n = g.tiled || g.coded ? lay.strip_bytes[i] : want;
                if (o > len || n > len - o || (!g.coded && n < want)) {
                    err = std::string("layout: ") + (g.tiled ? "tile " : "strip ") + std::to_string(i) +
                          " lies outside the source buffer or is short";
                    return false;
                }
                band.units.push_back({i, o, n});
            }
    return true;
}

}  // namespace jp2hip
