// split_host.cpp -- the tile-split inside the library (jp2hip_split_peers):
// one TIFF in host memory, one thread per member context, each uploading its
// band and running encode_split_core (encode.cpp) over a HostGroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "context.h"
#include "encode.h"
#include "host_group.h"
#include "orient_map.h"
#include "source_layout.h"

namespace jp2hip {
namespace {

struct RankResult {
    int rc = -1;
    std::string err;
    uint8_t *part = nullptr;
    size_t part_len = 0;
    uint64_t off = 0, flen = 0;
    jp2hip_stats st;
};

// One rank of a host-driven tile-split: gather the band's strips from the
// TIFF in host memory into pinned memory, upload them to member `m`, run the
// split encode, and (fd >= 0) write the part at its offset of the output file.
void split_rank(jp2hip_ctx *m, int rank, int world, HostGroup &grp, const uint8_t *file, size_t flen,
                const jp2hip_layout &lay, int conversion, const jp2hip_recipe &rc, int fd, double t0, int orient,
                RankResult &o) {
    std::memset(&o.st, 0, sizeof o.st);
    // the rank's band of upright rows, and the stored rows behind it: its own
    // rows, their mirror (orientation 3, 4) or the whole source (5..8)
    int64_t ow, oh, s0, s1;
    orient_size(lay.width, lay.height, orient, ow, oh);
    int r0 = 0, r1 = 0;
    jp2hip_split_rows((int32_t)oh, rc.tile_h, rc.flush_period, rank, world, &r0, &r1);
    orient_source_rows(lay.height, lay.width, orient, r0, r1, s0, s1);
    // what this rank uploads: the units those rows read, whole (the C++ form
    // of jp2hip.split.band_strips)
    UnitGrid grid;
    Band band;
    if (!unit_grid(lay, grid, o.err) || !band_walk(lay, grid, s0, s1, flen, band, o.err)) {
        grp.abort();
        return;
    }
    size_t tot = 0;
    for (const BandUnit &c : band.units) tot += c.bytes;
    uint8_t *h = out_alloc(std::max<size_t>(tot, 1));  // pinned: the upload is one DMA
    if (!h) {
        o.err = "out of (pinned) host memory";
        grp.abort();
        return;
    }
    const bool packed = grid.coded || grid.tiled;
    std::vector<uint64_t> offs((size_t)lay.nstrips * (packed ? 2 : 1), 0);
    size_t pos = 0;
    for (const BandUnit &c : band.units) {
        std::memcpy(h + pos, file + c.off, c.bytes);
        offs[c.idx] = pos;
        if (packed) offs[(size_t)lay.nstrips + c.idx] = c.bytes;
        pos += c.bytes;
    }
    jp2hip_layout bl = lay;
    bl.strip_offsets = offs.data();
    bl.strip_bytes = packed ? offs.data() + lay.nstrips : nullptr;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        if (!m->gpu.upload_source(h, std::max<size_t>(tot, 1), o.err) || !m->gpu.check_residency(o.err)) {
            grp.abort();
        } else {
            jp2hip_split sp{rank, world, &HostGroup::call, &grp};
            o.rc = encode_split_core(m, m->gpu.source(), std::max<size_t>(tot, 1), &bl, conversion, &rc, &sp,
                                     &o.part, &o.part_len, &o.off, &o.flen, &o.st, t0, orient);
            if (o.rc != 0) o.err = jp2hip_last_error();
            grp.abort();  // harmless after the last exchange; wakes the others after a failure
        }
        (void)hipStreamSynchronize(m->gpu.get_stream());  // the upload has read `h`
    }
    out_free(h);
    if (o.rc == 0 && fd >= 0) {
        size_t done = 0;
        while (done < o.part_len) {
            const ssize_t k = pwrite(fd, o.part + done, o.part_len - done, (off_t)(o.off + done));
            if (k <= 0) {
                o.rc = -1;
                o.err = "cannot write output";
                break;
            }
            done += (size_t)k;
        }
    }
}

}  // namespace

bool wants_split(const jp2hip_ctx *ctx, const jp2hip_layout &lay) {
    return !ctx->peers.empty() && (int64_t)lay.width * lay.height >= ctx->split_min_pixels;
}

// A whole-image encode split across ctx (rank 0) and its peers: the TIFF
// bytes are in host memory; the result goes to `fd` (each rank writes its
// part) or, fd < 0, into one pinned buffer *out.
int encode_split_host(jp2hip_ctx *ctx, const uint8_t *file, size_t flen, const jp2hip_layout &lay, int conversion,
                      const jp2hip_recipe *recipe, int fd, uint8_t **out, size_t *out_len, jp2hip_stats *stats,
                      double t0, int orient) {
    if (conversion != JP2HIP_LOSSY && conversion != JP2HIP_LOSSLESS)
        return fail("conversion must be JP2HIP_LOSSY (0) or JP2HIP_LOSSLESS (1)");
    const jp2hip_recipe rc = recipe_of(recipe, conversion);
    std::lock_guard<std::mutex> split_lk(ctx->split_mu);
    std::vector<jp2hip_ctx *> members{ctx};
    members.insert(members.end(), ctx->peers.begin(), ctx->peers.end());
    const int world = (int)members.size();
    HostGroup grp(world);
    std::vector<RankResult> res((size_t)world);
    std::vector<std::thread> th;
    for (int r = 1; r < world; r++)
        th.emplace_back([&, r] {
            split_rank(members[(size_t)r], r, world, grp, file, flen, lay, conversion, rc, fd, t0, orient,
                       res[(size_t)r]);
        });
    split_rank(ctx, 0, world, grp, file, flen, lay, conversion, rc, fd, t0, orient, res[0]);
    for (std::thread &t : th) t.join();
    // report the rank that failed first-hand, not one that saw the abort
    const RankResult *bad = nullptr;
    for (const RankResult &r : res)
        if (r.rc != 0 && (!bad || (bad->err.rfind("split:", 0) == 0 && r.err.rfind("split:", 0) != 0))) bad = &r;
    if (bad) {
        const std::string e = bad->err.empty() ? "split: encode failed" : bad->err;
        for (RankResult &r : res) out_free(r.part);
        return fail(e);
    }
    const uint64_t total = res[0].flen;
    if (fd < 0) {
        uint8_t *buf = out_alloc((size_t)total);
        if (!buf) {
            for (RankResult &r : res) out_free(r.part);
            return fail("out of (pinned) host memory");
        }
        for (const RankResult &r : res) std::memcpy(buf + r.off, r.part, r.part_len);
        *out = buf;
        *out_len = (size_t)total;
    }
    for (RankResult &r : res) out_free(r.part);
    if (stats) {
        *stats = res[0].st;
        for (int r = 1; r < world; r++) {
            stats->codeblocks += res[(size_t)r].st.codeblocks;
            stats->coded_passes += res[(size_t)r].st.coded_passes;
            stats->t1_bytes += res[(size_t)r].st.t1_bytes;
            stats->mq_decisions += res[(size_t)r].st.mq_decisions;
            stats->host_waits = std::max(stats->host_waits, res[(size_t)r].st.host_waits);
        }
        stats->out_bytes = (int64_t)total;
        stats->total_ms = now_ms() - t0;
    }
    return 0;
}

}  // namespace jp2hip
