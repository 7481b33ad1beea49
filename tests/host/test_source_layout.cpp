// CPU test of the source-layout module (csrc/source_layout.cpp), built with
// ASan / UBSan by tests/test_source_layout.py:
//  (a) the unit grid and the band walk against a row-by-row model, every band
//      of a few thousand tiny layouts;
//  (b) each refusal once, by name, with a unit outside the band lying outside
//      the buffer all the while;
//  (c) parse_tiff on every prefix of the TIFFs named on the command line and
//      on every one of their IFD bytes set to 0x00 and to 0xFF, each input a
//      heap copy of exactly its length;
//  (d) palette_lut and encoded_format on fixed values.
#include "source_layout.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <set>

using namespace jp2hip;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                              \
        }                                                            \
    } while (0)

// A layout with its own tables: unit i at offs[i], cnts[i] bytes.
struct Made {
    jp2hip_layout lay;
    std::vector<uint64_t> offs, cnts;
    uint64_t len = 0;  // the buffer ends where the last unit does
    void point() {
        lay.strip_offsets = offs.data();
        lay.strip_bytes = cnts.empty() ? nullptr : cnts.data();
    }
};

static jp2hip_layout geometry(int w, int h, int comps, int bits, int planar, int rps, int tw, int th, int compression) {
    jp2hip_layout l;
    std::memset(&l, 0, sizeof l);
    l.width = w;
    l.height = h;
    l.components = comps;
    l.bits = bits;
    l.planar = planar;
    l.rows_per_strip = rps;
    l.tile_width = tw;
    l.tile_height = th;
    l.compression = compression;
    l.predictor = 1;
    return l;
}

// The model's numbers, each found the slow way.
static int64_t count_units(int extent, int unit) {  // distinct units the pixels 0 .. extent-1 fall in
    std::set<int> s;
    for (int i = 0; i < extent; i++) s.insert(i / unit);
    return (int64_t)s.size();
}
static uint64_t model_row_bytes(int unit_w, int spp_row, int bits) {
    uint64_t nbits = 0;
    for (int x = 0; x < unit_w; x++) nbits += (uint64_t)spp_row * bits;
    return (nbits + 7) / 8;
}

// Unit tables for a geometry: units back to back with a gap of `gap` bytes,
// an uncompressed unit as large as its rows need, a "compressed" one of an
// arbitrary size.  with_counts: uncompressed strips carry strip_bytes too.
static Made make(jp2hip_layout l, bool with_counts, uint64_t gap) {
    Made m;
    m.lay = l;
    const bool tiled = l.tile_width > 0, coded = l.compression > 1;
    const int uw = tiled ? l.tile_width : l.width, uh = tiled ? l.tile_height : l.rows_per_strip;
    const int planes = l.planar == 2 ? l.components : 1;
    const int64_t across = tiled ? count_units(l.width, uw) : 1, urows = count_units(l.height, uh);
    const uint64_t rb = model_row_bytes(uw, l.planar == 2 ? 1 : l.components, l.bits);
    uint64_t pos = 8;
    for (int p = 0; p < planes; p++)
        for (int64_t u = 0; u < urows; u++)
            for (int64_t x = 0; x < across; x++) {
                const uint64_t i = m.offs.size();
                int rows = 0;
                for (int y = 0; y < l.height; y++) rows += y / uh == u;
                const uint64_t n = coded ? 1 + (i * 7) % 13 : (uint64_t)(tiled ? uh : rows) * rb;
                m.offs.push_back(pos);
                if (coded || tiled || with_counts) m.cnts.push_back(n);
                pos += n + gap;
            }
    m.len = pos - gap;
    m.lay.nstrips = (int32_t)m.offs.size();
    m.point();
    return m;
}

// (a) one layout: the grid's numbers, then every band against the model
static void check_layout(const Made &m) {
    const jp2hip_layout &l = m.lay;
    UnitGrid g;
    std::string err;
    CHECK(unit_grid(l, g, err));
    if (failures) return;
    const bool tiled = l.tile_width > 0;
    const int uw = tiled ? l.tile_width : l.width, uh = tiled ? l.tile_height : l.rows_per_strip;
    const int planes = l.planar == 2 ? l.components : 1;
    CHECK(g.tiled == tiled && g.coded == (l.compression > 1));
    CHECK(g.unit_w == uw && g.unit_h == uh && g.planes == planes);
    CHECK(g.across == (tiled ? count_units(l.width, uw) : 1) && g.urows == count_units(l.height, uh));
    CHECK(g.per_plane == g.across * g.urows && g.needed == g.per_plane * planes && g.needed == l.nstrips);
    CHECK(g.row_bytes == model_row_bytes(uw, l.planar == 2 ? 1 : l.components, l.bits));
    CHECK(g.unit_bytes == g.row_bytes * (uint64_t)uh);
    std::vector<int> rows_in((size_t)g.urows, 0);  // rows of the image in each unit row
    for (int y = 0; y < l.height; y++) rows_in[(size_t)(y / uh)]++;
    Band b;
    std::vector<uint8_t> want, got;
    for (int row0 = 0; row0 < l.height; row0++)
        for (int row1 = row0 + 1; row1 <= l.height; row1++) {
            want.assign((size_t)g.needed, 0);  // the units owning at least one row of the band
            for (int y = row0; y < row1; y++)
                for (int p = 0; p < planes; p++)
                    for (int64_t x = 0; x < g.across; x++) want[(size_t)(p * g.per_plane + (y / uh) * g.across + x)] = 1;
            if (!band_walk(l, g, row0, row1, m.len, b, err)) {
                std::printf("FAIL band [%d, %d): %s\n", row0, row1, err.c_str());
                failures++;
                return;
            }
            got.assign((size_t)g.needed, 0);
            bool ordered = true, fits = true;
            for (size_t k = 0; k < b.units.size(); k++) {
                const BandUnit &u = b.units[k];
                if (u.idx >= got.size()) {
                    fits = false;
                    break;
                }
                got[u.idx]++;  // (twice: no longer equal to want)
                // plane / unit-row / across order is the table's order
                ordered = ordered && (k == 0 || b.units[k - 1].idx < u.idx);
                fits = fits && u.off == m.offs[u.idx] && u.off <= m.len && u.bytes <= m.len - u.off;
                const int rows = rows_in[(u.idx % (size_t)g.per_plane) / (size_t)g.across];
                if (l.compression <= 1) fits = fits && u.bytes >= (uint64_t)(tiled ? uh : rows) * g.row_bytes;
                else fits = fits && u.bytes == m.cnts[u.idx];
            }
            CHECK(got == want);
            CHECK(ordered);
            CHECK(fits);
            CHECK(b.u0 == row0 / uh && b.u1 == (row1 - 1) / uh + 1);
            CHECK(b.row0 == b.u0 * uh && b.row1 == (b.u1 * uh < l.height ? b.u1 * uh : l.height));
            if (failures) return;
        }
    // an empty range: no units, no error
    CHECK(band_walk(l, g, 3, 3, m.len, b, err) && b.units.empty());
    CHECK(band_walk(l, g, 5, 2, m.len, b, err) && b.units.empty());
}

static int test_grid_and_band() {
    const int widths[] = {1, 7, 8, 9, 17}, heights[] = {1, 15, 16, 17, 33}, bitses[] = {1, 2, 4, 8, 16};
    const int tiles[][2] = {{0, 0}, {16, 16}, {32, 16}};
    int layouts = 0;
    for (int w : widths)
        for (int h : heights)
            for (const auto &t : tiles)
                for (int rps : {1, 16, h, h + 5}) {
                    if (t[0] && rps != 1) continue;  // (tiles: rows_per_strip plays no part)
                    for (int planar : {1, 2})
                        for (int comps : {1, 3})
                            for (int bits : bitses) {
                                if (bits < 8 && comps != 1) continue;  // (check_pixel_format refuses these)
                                for (int compression : {1, 5}) {
                                    const jp2hip_layout l = geometry(w, h, comps, bits, planar, rps, t[0], t[1], compression);
                                    check_layout(make(l, (layouts & 1) != 0, (uint64_t)(layouts % 3)));
                                    layouts++;
                                    if (failures) {
                                        std::printf("  at w %d h %d tile %dx%d rps %d planar %d comps %d bits %d compression %d\n",
                                                    w, h, t[0], t[1], rps, planar, comps, bits, compression);
                                        return layouts;
                                    }
                                }
                            }
                }
    return layouts;
}

// (b) `m` has at least three unit rows.  Its first unit row is thrown far
// outside the buffer, and the band starts below it: the walk passes.  Then
// `defect` is applied and the grid or the walk must refuse with `name`.
template <typename F>
static void refuses(Made m, int row0, int row1, const char *name, F defect) {
    UnitGrid g;
    Band b;
    std::string err;
    const bool tiled = m.lay.tile_width > 0;
    const int uh = tiled ? m.lay.tile_height : m.lay.rows_per_strip;
    const int across = tiled ? (m.lay.width + m.lay.tile_width - 1) / m.lay.tile_width : 1;
    CHECK(row0 >= uh);
    m.point();  // (a copy: its own tables)
    for (int x = 0; x < across; x++) m.offs[(size_t)x] = (1ull << 63) + 5;  // unit row 0 of plane 0: never in the band
    CHECK(unit_grid(m.lay, g, err) && band_walk(m.lay, g, row0, row1, m.len, b, err) && !b.units.empty());
    defect(m);
    m.point();
    err.clear();
    const bool ok = unit_grid(m.lay, g, err) && band_walk(m.lay, g, row0, row1, m.len, b, err);
    if (ok || err.find(name) == std::string::npos) {
        std::printf("FAIL refusal \"%s\": %s\n", name, ok ? "accepted" : err.c_str());
        failures++;
    }
}

static void test_refusals() {
    const Made strips = make(geometry(9, 40, 3, 8, 1, 8, 0, 0, 1), false, 2);      // 5 strips
    const Made coded = make(geometry(9, 40, 3, 8, 1, 8, 0, 0, 5), false, 2);       // 5 compressed strips
    const Made tiles = make(geometry(40, 40, 1, 8, 1, 1, 16, 16, 1), false, 2);    // 3 x 3 tiles
    const Made planar = make(geometry(9, 40, 3, 16, 2, 8, 0, 0, 1), false, 2);     // 3 planes of 5 strips
    const Made ctiles = make(geometry(40, 40, 1, 8, 1, 1, 16, 16, 8), false, 2);   // 3 x 3 Deflate tiles
    auto one_short = [](Made &m) { m.lay.nstrips--; };
    // the strip table one entry short of the height, on every route
    refuses(strips, 8, 40, "too few strips", one_short);
    refuses(coded, 8, 40, "too few strips", one_short);
    refuses(tiles, 16, 40, "too few tiles", one_short);
    refuses(ctiles, 16, 40, "too few tiles", one_short);
    refuses(planar, 8, 40, "too few strips", one_short);
    // the band's last unit ends one byte past the buffer
    auto past = [](Made &m) { m.len--; };
    refuses(strips, 8, 40, "outside the source buffer", past);
    refuses(coded, 8, 40, "outside the source buffer", past);
    refuses(tiles, 16, 40, "outside the source buffer", past);
    refuses(planar, 8, 40, "outside the source buffer", past);
    // ... and the same unit left out of the band: no refusal
    {
        Made m = strips;
        UnitGrid g;
        Band b;
        std::string err;
        m.point();
        m.len--;
        CHECK(unit_grid(m.lay, g, err) && band_walk(m.lay, g, 0, 32, m.len, b, err) && b.units.size() == 4);
    }
    // an offset that wraps when the size is added
    auto wraps = [](Made &m) { m.offs[2] = ~0ull - 63; };
    refuses(strips, 8, 40, "outside the source buffer", wraps);
    refuses(coded, 8, 40, "outside the source buffer", wraps);
    // an uncompressed tile one byte short of a whole tile
    refuses(tiles, 16, 40, "short", [](Made &m) { m.cnts[4]--; });
    // tables and fields the form needs
    refuses(tiles, 16, 40, "strip_bytes", [](Made &m) { m.cnts.clear(); });
    refuses(coded, 8, 40, "strip_bytes", [](Made &m) { m.cnts.clear(); });
    refuses(tiles, 16, 40, "tile_width and tile_height", [](Made &m) { m.lay.tile_height = 0; });
    refuses(strips, 8, 40, "compression 7", [](Made &m) { m.lay.compression = 7; });
    refuses(strips, 8, 40, "bad geometry", [](Made &m) { m.lay.rows_per_strip = 0; });
    refuses(strips, 8, 40, "bad geometry", [](Made &m) { m.lay.width = -3; });
    refuses(strips, 8, 40, "bits/sample", [](Made &m) { m.lay.bits = 3; });
    // rows that hold none of the image
    {
        UnitGrid g;
        Band b;
        std::string err;
        CHECK(unit_grid(strips.lay, g, err));
        CHECK(!band_walk(strips.lay, g, 40, 48, strips.len, b, err) && err.find("empty band") != std::string::npos);
        CHECK(!band_walk(strips.lay, g, -9, 0, strips.len, b, err) && err.find("empty band") != std::string::npos);
        // a range that reaches past the image is cut to it
        CHECK(band_walk(strips.lay, g, -4, 99, strips.len, b, err) && b.units.size() == 5 && b.row0 == 0 && b.row1 == 40);
    }
    // a missing offsets table
    {
        Made m = strips;
        UnitGrid g;
        std::string err;
        m.lay.strip_offsets = nullptr;
        CHECK(!unit_grid(m.lay, g, err) && err.find("strip_offsets") != std::string::npos);
    }
    // uncompressed strips: the byte count is the geometry's, whatever strip_bytes says
    {
        Made m = make(geometry(9, 40, 3, 8, 1, 8, 0, 0, 1), true, 0);
        UnitGrid g;
        Band b;
        std::string err;
        for (uint64_t &c : m.cnts) c = 1;
        CHECK(unit_grid(m.lay, g, err) && band_walk(m.lay, g, 0, 40, m.len, b, err));
        CHECK(b.units.size() == 5 && b.units[4].bytes == 8 * 27);
    }
    // a whole-image walk looks at the units the image needs, not at every entry
    {
        Made m = coded;
        UnitGrid g;
        Band b;
        std::string err;
        m.offs.push_back(~0ull - 3);
        m.cnts.push_back(100);
        m.lay.nstrips++;
        m.point();
        CHECK(unit_grid(m.lay, g, err) && band_walk(m.lay, g, 0, 40, m.len, b, err) && b.units.size() == 5);
    }
}

// (c) one parse of exactly `n` bytes on the heap; a layout it yields must
// pass its own whole-image walk against n, its pointers inside the input
static void parse_exact(const uint8_t *src, size_t n, int &parsed) {
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
    std::memcpy(buf.get(), src, n);
    jp2hip_layout lay;
    std::vector<uint64_t> offs;
    std::string err;
    if (!parse_tiff(buf.get(), n, &lay, offs, err)) {
        CHECK(err.rfind("tiff: ", 0) == 0);
        return;
    }
    parsed++;
    UnitGrid g;
    Band b;
    const bool ok = unit_grid(lay, g, err) && band_walk(lay, g, 0, lay.height, n, b, err);
    if (!ok) {
        std::printf("FAIL a parsed layout is refused: %s\n", err.c_str());
        failures++;
        return;
    }
    CHECK((int64_t)b.units.size() == g.needed && g.needed == lay.nstrips);
    const uint8_t *end = buf.get() + n;
    if (lay.icc) CHECK(lay.icc >= buf.get() && lay.icc_bytes <= (uint64_t)(end - lay.icc));
    if (lay.colormap) {
        CHECK(lay.colormap >= buf.get() && 2 * lay.colormap_entries <= (uint64_t)(end - lay.colormap));
        uint32_t lut[256];
        palette_lut(lay, lut);  // (reads every entry: the sanitizer sees them)
    }
    int nc, bits;
    encoded_format(lay, nc, bits);
    CHECK((nc == 3 || nc == lay.components) && (bits == 8 || bits == 16));
}

static bool fuzz_file(const char *path) {
    std::ifstream f(path, std::ios::binary);
    const std::vector<uint8_t> tif((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (tif.size() < 16) {
        std::printf("FAIL cannot read %s\n", path);
        return false;
    }
    int whole = 0, parsed = 0;
    parse_exact(tif.data(), tif.size(), whole);
    CHECK(whole == 1);  // the fixture itself is a TIFF the parser takes
    for (size_t n = 0; n < tif.size(); n++) parse_exact(tif.data(), n, parsed);
    // the IFD: entry count, entries and the next-IFD offset
    const bool le = tif[0] == 'I';
    auto rd = [&](size_t o, int k) {
        uint64_t v = 0;
        for (int i = 0; i < k; i++) v |= (uint64_t)tif[o + (le ? i : k - 1 - i)] << (8 * i);
        return v;
    };
    const bool big = rd(2, 2) == 43;
    const size_t ifd = (size_t)(big ? rd(8, 8) : rd(4, 4));
    const size_t ifd_end = ifd + (big ? 8 + 20 * (size_t)rd(ifd, 8) + 8 : 2 + 12 * (size_t)rd(ifd, 2) + 4);
    CHECK(ifd < ifd_end && ifd_end <= tif.size());
    if (failures) return false;
    std::vector<uint8_t> mod = tif;
    for (size_t i = ifd; i < ifd_end; i++)
        for (uint8_t v : {(uint8_t)0x00, (uint8_t)0xFF}) {
            mod[i] = v;
            parse_exact(mod.data(), mod.size(), parsed);
            mod[i] = tif[i];
        }
    std::printf("%s: %zu bytes, IFD of %zu; %d of the damaged inputs still parse\n", path, tif.size(), ifd_end - ifd, parsed);
    return failures == 0;
}

// (d)
static void test_palette_and_format() {
    jp2hip_layout l = geometry(4, 4, 1, 2, 1, 4, 0, 0, 1);
    l.photometric = JP2HIP_PHOTO_PALETTE;
    // 16-bit entries, little-endian: R 0x1100 0x2200 0x3300 0xFFFF, G 0 .., B ..
    const uint16_t wide[12] = {0x1100, 0x2200, 0x3300, 0xFFFF, 0x0000, 0x4400, 0x80FF, 0x0100, 0xAB00, 0x00FF, 0x7F80, 0x1234};
    uint8_t raw[24];
    for (int i = 0; i < 12; i++) {
        raw[2 * i] = (uint8_t)wide[i];
        raw[2 * i + 1] = (uint8_t)(wide[i] >> 8);
    }
    l.colormap = raw;
    l.colormap_entries = 12;
    uint32_t lut[4];
    palette_lut(l, lut);
    CHECK(lut[0] == (0x11u | 0x00u << 8 | 0xABu << 16));
    CHECK(lut[1] == (0x22u | 0x44u << 8 | 0x00u << 16));
    CHECK(lut[2] == (0x33u | 0x80u << 8 | 0x7Fu << 16));
    CHECK(lut[3] == (0xFFu | 0x01u << 8 | 0x12u << 16));
    // the same bytes read big-endian
    l.big_endian = 1;
    palette_lut(l, lut);
    CHECK(lut[0] == (0x00u | 0x00u << 8 | 0x00u << 16));  // 0x0011, 0x0000, 0x00AB: the high bytes
    CHECK(lut[3] == (0xFFu | 0x00u << 8 | 0x34u << 16));  // 0xFFFF, 0x0001, 0x3412
    // no entry above 255: the map holds 8-bit values, taken as they are
    l.big_endian = 0;
    for (int i = 0; i < 12; i++) {
        raw[2 * i] = (uint8_t)(20 * i + 7);
        raw[2 * i + 1] = 0;
    }
    palette_lut(l, lut);
    CHECK(lut[0] == (7u | 87u << 8 | 167u << 16));
    CHECK(lut[3] == (67u | 147u << 8 | 227u << 16));
    // ... and one entry of 256 turns every entry into its high byte
    raw[1] = 1;  // entry 0 = 0x0107
    palette_lut(l, lut);
    CHECK(lut[0] == (1u | 0u << 8 | 0u << 16));
    CHECK(lut[3] == 0u);

    int nc, bits;
    encoded_format(l, nc, bits);
    CHECK(nc == 3 && bits == 8);  // palette: RGB
    l.bits = 8;
    encoded_format(l, nc, bits);
    CHECK(nc == 3 && bits == 8);
    l.photometric = JP2HIP_PHOTO_WHITE_IS_ZERO;
    l.bits = 1;
    encoded_format(l, nc, bits);
    CHECK(nc == 1 && bits == 8);  // packed grey: 8-bit grey
    CHECK(needs_expand(l));
    l = geometry(4, 4, 4, 16, 2, 4, 0, 0, 1);
    encoded_format(l, nc, bits);
    CHECK(nc == 4 && bits == 16 && !needs_expand(l));  // whole samples: as they are
    l.bits = 8;
    l.components = 3;
    encoded_format(l, nc, bits);
    CHECK(nc == 3 && bits == 8 && !needs_expand(l));
    CHECK(packed_row_bytes(9, 1, 1) == 2 && packed_row_bytes(9, 1, 4) == 5 && packed_row_bytes(9, 3, 16) == 54);
}

int main(int argc, char **argv) {
    const int layouts = test_grid_and_band();
    if (failures) return 1;
    std::printf("%d layouts, every band of each\n", layouts);
    test_refusals();
    test_palette_and_format();
    if (failures) return 1;
    for (int i = 1; i < argc; i++)
        if (!fuzz_file(argv[i])) return 1;
    std::printf("SOURCE LAYOUT OK (%d files)\n", argc - 1);
    return 0;
}
