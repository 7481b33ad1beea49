// test_dwt_route.cpp -- csrc/dwt_route.h on the CPU (g++, ASan + UBSan): which
// kernel form lifts each DWT level, on what grid, with how much LDS.
//
//  * sweep: every plane width 1..32768, heights on both sides of every
//    height-dependent rule, 1..4 components, 0..7 levels, one tile and tile
//    counts past what a grid dimension holds: the levels are consecutive and
//    end at `levels` or at a tail, every form's LDS stays inside what its
//    instances may be given, a tail level fits the tail's static buffers, the
//    grid covers the level's rows and column chunks exactly, and a route is
//    refused exactly when a chunked launch would have a dimension out of range;
//  * table: the routes of the shapes the GPU cases are laid around, pinned.
//
// --route tile_w tile_h nc levels prints the route of one tile, a line per
// launch: form level W H threads columns-per-thread grid-x grid-y grid-z LDS.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "dwt_route.h"

using namespace jp2hip;

static int g_fail = 0;
#define CHECK(c, ...)                                        \
    do {                                                     \
        if (!(c)) {                                          \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            if (++g_fail > 20) std::exit(1);                 \
        }                                                    \
    } while (0)

static const size_t KiB = 1024;

static const char *dwt_form_name(DwtForm f) {
    static const char *const kNames[] = {"L1Stream", "L1Window", "L1Chunk", "BandIngest", "Band", "BandChunk", "Tail"};
    return kNames[(int)f];
}

static bool in_range(const DwtLevelRoute &r) {
    return r.gx >= 1 && r.gy >= 1 && r.gy <= 65535 && r.gz >= 1 && r.gz <= 65535;
}

static long g_forms[7], g_refused = 0, g_widest_band = 0;

static void check_level(const DwtLevelRoute &r, int pw, int ph, int nc, int ntc, int levels) {
#define AT "plane %dx%d nc %d ntc %d levels %d level %d (%s): "
#define ARGS pw, ph, nc, ntc, levels, r.level, dwt_form_name(r.form)
    const int sh = r.level - 1;
    CHECK(r.W == (pw + (1 << sh) - 1) >> sh && r.H == (ph + (1 << sh) - 1) >> sh, AT "size %dx%d", ARGS, r.W, r.H);
    const bool stream = r.form == DwtForm::L1Stream, chunk = r.form == DwtForm::L1Chunk || r.form == DwtForm::BandChunk;
    const bool l1 = stream || r.form == DwtForm::L1Window || r.form == DwtForm::L1Chunk || r.form == DwtForm::BandIngest;
    CHECK(l1 == (r.level == 1), AT "form at this level", ARGS);
    switch (r.form) {
    case DwtForm::L1Stream:
        CHECK(r.W <= 1024 && r.cpt * 256 >= r.W && (r.cpt == 1 || r.cpt == 2 || r.cpt == 4), AT "W %d cpt %d", ARGS, r.W, r.cpt);
        CHECK(r.cpt == 1 || (r.cpt / 2) * 256 < r.W, AT "W %d takes fewer than %d columns per thread", ARGS, r.W, r.cpt);
        CHECK(r.lds == dwt_stream_lds(nc, r.W) && r.lds <= 128 * KiB, AT "LDS %zu", ARGS, r.lds);
        break;
    case DwtForm::L1Window:
        CHECK(r.lds == dwt_rows_lds(nc * kRb1, r.W) && r.lds <= 128 * KiB, AT "LDS %zu", ARGS, r.lds);
        break;
    case DwtForm::L1Chunk:
        CHECK(r.lds == band_chunk_lds(nc * kRb1, kL1ChunkW) && r.lds <= 128 * KiB, AT "LDS %zu", ARGS, r.lds);
        CHECK(r.gz == dwt_chunk_count(r.W, kL1ChunkW), AT "chunks %d", ARGS, r.gz);
        break;
    case DwtForm::BandIngest:
    case DwtForm::Band:
        CHECK(r.lds == dwt_rows_lds(kBandRb, r.W) && r.lds <= 160 * KiB, AT "LDS %zu", ARGS, r.lds);
        if (r.W > g_widest_band) g_widest_band = r.W;
        break;
    case DwtForm::BandChunk:
        CHECK(r.lds == band_chunk_lds(kBandRb, kBandChunkW) && r.lds <= 64 * KiB, AT "LDS %zu", ARGS, r.lds);
        CHECK(r.gz == dwt_chunk_count(r.W, kBandChunkW), AT "chunks %d", ARGS, r.gz);
        break;
    case DwtForm::Tail:
        CHECK(r.lds == 0, AT "LDS %zu", ARGS, r.lds);
        CHECK(r.level >= 2, AT "a tail at level 1", ARGS);
        CHECK(lds_row_stride(r.W) * r.H + kPadL + kPadR <= kTailWords, AT "rows of %dx%d", ARGS, r.W, r.H);
        CHECK(((r.W + 1) / 2) * ((r.H + 1) / 2) <= kTailLL, AT "LL of %dx%d", ARGS, r.W, r.H);
        CHECK(r.gx == ntc && r.gy == 1, AT "grid %d x %d", ARGS, r.gx, r.gy);
        break;
    }
    if (!chunk) CHECK(r.gz == 1, AT "grid z %d", ARGS, r.gz);
    if (!stream) CHECK(r.cpt == 0, AT "cpt %d", ARGS, r.cpt);
    const bool narrow = r.form == DwtForm::Band && r.W <= 128;
    CHECK(r.threads == (narrow ? 128 : 256), AT "W %d in %d threads", ARGS, r.W, r.threads);
    if (r.form != DwtForm::Tail) {
        const int rows = dwt_form_rows(r.form);
        CHECK(rows > 0 && (long)r.gx * rows >= r.H && r.H > (long)(r.gx - 1) * rows, AT "%d bands of %d rows for H %d", ARGS, r.gx, rows, r.H);
        const bool per_tile = r.form != DwtForm::BandIngest && r.level == 1;
        CHECK(r.gy == (per_tile ? ntc / nc : ntc), AT "grid y %d", ARGS, r.gy);
    }
    g_forms[(int)r.form]++;
#undef AT
#undef ARGS
}

static void check_route(int pw, int ph, int nc, int ntc, int levels) {
    const DwtRoute rt = dwt_route(pw, ph, nc, ntc, levels);
    CHECK(rt.n >= 0 && rt.n <= levels, "plane %dx%d nc %d levels %d: %d launches", pw, ph, nc, levels, rt.n);
    for (int i = 0; i < rt.n; i++) {
        const DwtLevelRoute &r = rt.lv[i];
        CHECK(r.level == i + 1, "plane %dx%d nc %d levels %d: launch %d is level %d", pw, ph, nc, levels, i, r.level);
        CHECK(r.form != DwtForm::Tail || i == rt.n - 1, "plane %dx%d nc %d levels %d: a tail before the end", pw, ph, nc, levels);
        check_level(r, pw, ph, nc, ntc, levels);
        const bool chunk = r.form == DwtForm::L1Chunk || r.form == DwtForm::BandChunk;
        if (chunk) CHECK(in_range(r), "plane %dx%d nc %d ntc %d levels %d: chunked grid %d x %d x %d accepted", pw, ph, nc, ntc, levels, r.gx, r.gy, r.gz);
    }
    if (rt.refused) {
        const DwtLevelRoute &r = rt.lv[rt.n];
        CHECK(!in_range(r), "plane %dx%d nc %d ntc %d levels %d: refused (%s) with grid %d x %d x %d", pw, ph, nc, ntc, levels, rt.refused, r.gx, r.gy, r.gz);
        g_refused++;
    } else if (levels > 0) {
        const DwtLevelRoute &last = rt.lv[rt.n - 1];
        CHECK(rt.n >= 1 && (last.level == levels || last.form == DwtForm::Tail), "plane %dx%d nc %d levels %d: ends at level %d", pw, ph, nc, levels, last.level);
    } else {
        CHECK(rt.n == 0, "no levels, %d launches", rt.n);
    }
}

// "L1Stream/2@512 Band/256@256 ... Tail@64": form, columns per thread
// (streaming) or threads (whole-row band), width at the level
static std::string describe(const DwtRoute &rt) {
    std::string s;
    for (int i = 0; i < rt.n; i++) {
        const DwtLevelRoute &r = rt.lv[i];
        if (i) s += " ";
        s += dwt_form_name(r.form);
        if (r.form == DwtForm::L1Stream) s += "/" + std::to_string(r.cpt);
        if (r.form == DwtForm::Band) s += "/" + std::to_string(r.threads);
        s += "@" + std::to_string(r.W);
    }
    if (rt.refused) s += std::string(s.empty() ? "" : " ") + "refused";
    return s;
}

struct Pinned {
    int tw, th, nc, levels;
    const char *route;
};
static const Pinned kPinned[] = {
    {512, 512, 3, 6, "L1Stream/2@512 Band/256@256 Band/128@128 Tail@64"},
    {256, 256, 2, 5, "L1Stream/1@256 Band/128@128 Tail@64"},
    {1024, 1024, 3, 6, "L1Stream/4@1024 Band/256@512 Band/256@256 Band/128@128 Tail@64"},
    {128, 128, 3, 2, "L1Stream/1@128 Tail@64"},
    {2048, 2048, 1, 6, "L1Window@2048 Band/256@1024 Band/256@512 Band/256@256 Band/128@128 Tail@64"},
    {2048, 2048, 3, 6, "BandIngest@2048 Band/256@1024 Band/256@512 Band/256@256 Band/128@128 Tail@64"},
    {4224, 128, 3, 6, "L1Chunk@4224 Band/256@2112 Band/256@1056 Band/256@528 Tail@264"},
    {8320, 64, 1, 6, "L1Chunk@8320 BandChunk@4160 Band/256@2080 Band/256@1040 Tail@520"},
    {16512, 128, 1, 7, "L1Chunk@16512 BandChunk@8256 BandChunk@4128 Band/256@2064 Band/256@1032 Tail@516"},
    {64, 4224, 1, 6, "L1Stream/1@64 Band/128@32 Band/128@16 Band/128@8 Band/128@4 Band/128@2"},
    {2560, 64, 1, 5, "L1Window@2560 Band/256@1280 Band/256@640 Tail@320"},
    {2560, 64, 4, 5, "L1Chunk@2560 Band/256@1280 Band/256@640 Tail@320"},
    {3072, 64, 3, 5, "L1Chunk@3072 Band/256@1536 Band/256@768 Tail@384"},
};

static int print_route(int tw, int th, int nc, int levels) {
    const DwtRoute rt = dwt_route(tw, th, nc, nc, levels);
    if (rt.refused) {
        std::printf("refused: %s\n", rt.refused);
        return 2;
    }
    for (int i = 0; i < rt.n; i++) {
        const DwtLevelRoute &r = rt.lv[i];
        std::printf("%s %d %d %d %d %d %d %d %d %zu\n", dwt_form_name(r.form), r.level, r.W, r.H, r.threads, r.cpt, r.gx,
                    r.gy, r.gz, r.lds);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 6 && !std::strcmp(argv[1], "--route"))
        return print_route(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
    if (argc != 1) {
        std::printf("usage: %s [--route tile_w tile_h nc levels]\n", argv[0]);
        return 2;
    }
    // heights: one row, both sides of the tail's 64 x 64 and 128 x 32 at
    // levels 2 and up, of the row bands (8, 16, 64), and the tallest tile
    static const int kHeights[] = {1, 2, 9, 17, 63, 64, 65, 127, 128, 129, 130, 256, 257, 1000, 4224, 32768};
    long nroutes = 0;
    for (int pw = 1; pw <= 32768; pw++)
        for (int ph : kHeights)
            for (int nc = 1; nc <= 4; nc++)
                for (int levels = 0; levels <= 7; levels++) {
                    check_route(pw, ph, nc, nc, levels);
                    nroutes++;
                }
    // many tiles: up to the 65535 a code-stream numbers, so levels >= 2 (a
    // workgroup row per tile-component) can exceed a grid dimension, and more
    // than that (no plan has them: level 1 is refused too)
    for (int pw = 1; pw <= 32768; pw += (pw < 8192 ? 61 : 1021))
        for (int ph : {1, 64, 130})
            for (int nc = 1; nc <= 4; nc++)
                for (int tiles : {2, 16384, 21846, 65535, 65536})
                    for (int levels : {1, 3, 7}) {
                        check_route(pw, ph, nc, tiles * nc, levels);
                        nroutes++;
                    }
    for (int f = 0; f < 7; f++) CHECK(g_forms[f] > 0, "the sweep never reached %s", dwt_form_name((DwtForm)f));
    CHECK(g_refused > 0, "the sweep never reached a refusal");
    // the widest level on whole rows (tests/large_tile_cases.py)
    CHECK(g_widest_band == 2496, "widest whole-row band level %ld", g_widest_band);
    for (const Pinned &p : kPinned) {
        const std::string got = describe(dwt_route(p.tw, p.th, p.nc, p.nc, p.levels));
        CHECK(got == p.route, "%dx%d nc %d levels %d: %s, pinned %s", p.tw, p.th, p.nc, p.levels, got.c_str(), p.route);
    }
    if (g_fail) {
        std::printf("DWT ROUTE FAILED: %d checks\n", g_fail);
        return 1;
    }
    std::printf("DWT ROUTE OK: %ld routes, %ld refused, widest whole-row level %ld, %zu pinned\n", nroutes, g_refused,
                g_widest_band, sizeof kPinned / sizeof kPinned[0]);
    return 0;
}
