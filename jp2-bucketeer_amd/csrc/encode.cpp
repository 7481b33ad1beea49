// encode.cpp -- one encode on one context: the single-GPU encode (encode_core)
// and one rank of a tile-split encode (encode_split_core).  They share how an
// encode begins (begin), prepare_source, the rate target and first budget,
// and how a rank's part of the file is written (finish_part).  Their rate
// loops are different algorithms on purpose: the single encode runs the loop
// on the device (GpuEncoder::rate_loop: one host wait, a retry when the
// decision-stream pool was short; the benchmark measures this one), the split
// encode iterates on the host over thresholds its ranks exchange, its pool
// sized for the worst case (pool_worst: ranks cannot repeat an exchange).
// With fixed-slope layers (jp2hip_set_layer_slopes) neither runs: both encodes
// apply the caller's thresholds where the lossless encode applies its own.
// With per-layer rates (jp2hip_set_layer_rates) both loops run with a target
// and a budget per layer and one step, layer_rate_step (jp2hip_internal.h),
// also for a lossless recipe, whose plan then has one rate-control group.
// With PSNR targets (jp2hip_set_layer_psnr) neither loop runs either: the
// thresholds come from one selection over distortion quanta -- on the device
// (GpuEncoder::select_psnr) or, in a split, agreed through
// jp2hip_split_psnr_thresholds -- and the rest is the fixed-slope encode.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"
#include "encode.h"
#include "psnr_quantum.h"
#include "source_layout.h"

namespace jp2hip {

void default_recipe(jp2hip_recipe *r, int conversion) {
    std::memset(r, 0, sizeof *r);
    r->levels = 6;
    r->layers = 6;
    r->tile_w = r->tile_h = 512;
    r->cblk_w_log2 = r->cblk_h_log2 = 6;
    r->nprecincts = 3;
    r->prec_w_log2[0] = r->prec_h_log2[0] = 8;
    r->prec_w_log2[1] = r->prec_h_log2[1] = 8;
    r->prec_w_log2[2] = r->prec_h_log2[2] = 7;
    r->progression = 2;
    r->sop = r->eph = r->plt = r->tparts_r = 1;
    r->guard_bits = 1;
    bool lossless = conversion == JP2HIP_LOSSLESS;
    r->reversible = lossless ? 1 : 0;
    r->mct = 1;
    r->qstep = 1.0 / 256.0;
    r->rate_bpp = lossless ? 0.0 : 3.0;
    r->format = JP2HIP_FORMAT_JPX;
    r->comment = 1;
    r->slope_skip = 1;
    r->flush_period = 1024;
}

// The caller's recipe (or the default for `conversion`) with its padding
// bytes zeroed, so PlanCache's byte compare sees only the fields.
jp2hip_recipe recipe_of(const jp2hip_recipe *recipe, int conversion) {
    jp2hip_recipe rc;
    std::memset(&rc, 0, sizeof rc);
    if (recipe) rc = *recipe;
    else default_recipe(&rc, conversion);
    const size_t gap0 = offsetof(jp2hip_recipe, mct) + sizeof rc.mct, gap1 = offsetof(jp2hip_recipe, qstep);
    if (gap1 > gap0) std::memset((char *)&rc + gap0, 0, gap1 - gap0);
    static_assert(offsetof(jp2hip_recipe, flush_period) + sizeof(int32_t) == sizeof(jp2hip_recipe),
                  "jp2hip_recipe: no tail padding");
    return rc;
}

bool check_layer_slopes(const double *s, int n, const jp2hip_recipe *rc, std::string &err) {
    if (n < 0 || n > kMaxLayers || (n > 0 && !s)) {
        err = "layer slopes: n = " + std::to_string(n) + " is outside 0 .. " + std::to_string(kMaxLayers) +
              " (or no thresholds were given)";
        return false;
    }
    for (int i = 0; i < n; i++) {
        const std::string at = "layer slopes: slopes[" + std::to_string(i) + "]";
        if (std::isnan(s[i])) err = at + " is NaN";
        else if (std::signbit(s[i])) err = at + " = " + std::to_string(s[i]) + " is negative";
        else if (i && s[i] > s[i - 1])
            err = at + " increases over slopes[" + std::to_string(i - 1) + "]: the thresholds fall from layer 0 on";
        else continue;
        return false;
    }
    if (!rc || !n) return true;
    if (n != rc->layers) {
        err = "layer slopes: n = " + std::to_string(n) + " thresholds for an encode of recipe.layers = " +
              std::to_string(rc->layers);
        return false;
    }
    if (rc->rate_bpp <= 0.0 && s[n - 1] != 0.0) {
        err = "layer slopes: slopes[" + std::to_string(n - 1) + "], the last, must be 0 with rate_bpp <= 0 " +
              "(the last layer takes every coded pass)";
        return false;
    }
    return true;
}

bool check_layer_rates(const double *r, int n, const jp2hip_recipe *rc, std::string &err) {
    if (n < 0 || n > kMaxLayers || (n > 0 && !r)) {
        err = "layer rates: n = " + std::to_string(n) + " is outside 0 .. " + std::to_string(kMaxLayers) +
              " (or no rates were given)";
        return false;
    }
    for (int i = 0; i < n; i++) {
        const std::string at = "layer rates: rates[" + std::to_string(i) + "]";
        if (std::isnan(r[i])) err = at + " is NaN";
        else if (std::isinf(r[i])) err = at + " is infinite";
        else if (std::signbit(r[i])) err = at + " = " + std::to_string(r[i]) + " is negative";
        else if (i && r[i] < r[i - 1] && !(i == n - 1 && r[i] == 0.0))
            err = at + " decreases from rates[" + std::to_string(i - 1) + "]: the rates rise from layer 0 on";
        else continue;
        return false;
    }
    if (!rc || !n) return true;
    if (n != rc->layers) {
        err = "layer rates: n = " + std::to_string(n) + " rates for an encode of recipe.layers = " +
              std::to_string(rc->layers);
        return false;
    }
    if (rc->rate_bpp <= 0.0 && r[n - 1] != 0.0) {
        err = "layer rates: rates[" + std::to_string(n - 1) + "], the last, must be 0 with rate_bpp <= 0 " +
              "(the last layer takes every coded pass)";
        return false;
    }
    for (int i = 0; i < n && rc->rate_bpp > 0.0; i++)
        if (r[i] == 0.0) {
            err = "layer rates: rates[" + std::to_string(i) + "] is 0 with rate_bpp > 0 (0 names a lossless top layer: " +
                  "rate_bpp <= 0)";
            return false;
        }
    return true;
}

bool check_layer_psnr(const double *p, int n, const jp2hip_recipe *rc, std::string &err) {
    if (n < 0 || n > kMaxLayers || (n > 0 && !p)) {
        err = "layer psnr: n = " + std::to_string(n) + " is outside 0 .. " + std::to_string(kMaxLayers) +
              " (or no targets were given)";
        return false;
    }
    for (int i = 0; i < n; i++) {
        const std::string at = "layer psnr: psnr_db[" + std::to_string(i) + "]";
        if (std::isnan(p[i])) err = at + " is NaN";
        else if (std::isinf(p[i])) err = at + " is infinite";
        else if (std::signbit(p[i])) err = at + " = " + std::to_string(p[i]) + " is negative";
        else if (i && p[i] < p[i - 1] && !(i == n - 1 && p[i] == 0.0))
            err = at + " decreases from psnr_db[" + std::to_string(i - 1) + "]: the targets rise from layer 0 on";
        else continue;
        return false;
    }
    if (!rc || !n) return true;
    if (n != rc->layers) {
        err = "layer psnr: n = " + std::to_string(n) + " targets for an encode of recipe.layers = " +
              std::to_string(rc->layers);
        return false;
    }
    if (rc->rate_bpp <= 0.0 && p[n - 1] != 0.0) {
        err = "layer psnr: psnr_db[" + std::to_string(n - 1) + "], the last, must be 0 with rate_bpp <= 0 " +
              "(the last layer takes every coded pass)";
        return false;
    }
    for (int i = 0; i < n && rc->rate_bpp > 0.0; i++)
        if (p[i] == 0.0) {
            err = "layer psnr: psnr_db[" + std::to_string(i) + "] is 0 with rate_bpp > 0 (0 names a lossless top layer: " +
                  "rate_bpp <= 0)";
            return false;
        }
    return true;
}

void layer_psnr_targets(int width, int height, int components, int bits, const double *psnr_db, int n,
                        int64_t *targets) {
    const double peak = std::ldexp(1.0, bits) - 1.0;
    // peak^2 N 2^-s: exact in a double up to 2^53, which a 2^29-sample image reaches
    const double full = peak * peak * ((double)width * (double)height * (double)components) *
                        quantum_pow2(-quantum_shift(bits));
    for (int l = 0; l < n; l++) {
        if (l == n - 1 && psnr_db[l] == 0.0) {  // the lossless top layer takes every coded pass
            targets[l] = -1;
            continue;
        }
        const double t = std::floor(full / std::pow(10.0, psnr_db[l] / 10.0));
        targets[l] = t >= (double)kQuantaTargetMax ? kQuantaTargetMax : (int64_t)t;
    }
}

// An upper bound on the quanta of a plan's hull segments (psnr_quantum.h has
// the reasoning): false when it reaches 2^63, an image whose sums could
// overflow and which an encode by PSNR targets therefore refuses.
bool quanta_fit(const Plan &P) {
    const double scale = quantum_pow2(-quantum_shift(P.bits));
    double sum = 0.0;
    for (size_t b = 0; b < P.blocks.size(); b++) {
        const BlockDesc &d = P.blocks[b];
        sum += P.weight[b] * 8.0 * (double)d.w * (double)d.h * std::ldexp(1.0, 2 * d.Mb) * scale +
               (double)std::max(0, 3 * d.Mb - 2);
    }
    return sum < kQuantaLimit;
}

namespace {

// The slope keys of a context's thresholds: the doubles' bit patterns.
std::vector<uint64_t> slope_keys(const std::vector<double> &s) {
    std::vector<uint64_t> K(s.size());
    if (!s.empty()) std::memcpy(K.data(), s.data(), 8 * s.size());
    return K;
}

// A rate-driven encode's target (bytes): the floor(rate * W * H / 8) the
// oracle's predict_and_code uses; slope prediction's is the same, -1 = off
// (an image so small that the target is 0 bytes still predicts, as the
// oracle does: 0 is a target like any other).  org: the bytes of the TLM marker
// segments plus those the L / C tile-part divisions add
// (tile_part_division_bytes), parts of the code-stream the target bounds -- a
// rate-driven encode with either is the encode without whose target is that
// much lower (floored at 0), so everything the target steers sees the lower one.
int64_t rate_target_of(const jp2hip_recipe &rc, int w, int h, int64_t org) {
    const int64_t target = (int64_t)std::floor(rc.rate_bpp * (double)w * (double)h / 8.0);
    return org ? std::max<int64_t>(0, target - org) : target;
}
int64_t skip_target_of(const jp2hip_recipe &rc, int w, int h, int64_t org) {
    return rc.slope_skip && rc.rate_bpp > 0.0 ? rate_target_of(rc, w, h, org) : -1;
}
// The rate loop's first budget: its header estimate (16 bytes per packet)
// lands the usual encode under the target (C2: 8 985 521 of 9 000 000 bytes).
int64_t first_budget_of(const Plan &P, int64_t target) { return target - 16 * P.npackets - 16 * P.ntileparts - 256; }

// How both encodes begin: the checks (sp: a split's rank and group), the
// recipe, what the source states about its pixels (into the file header, per
// encode: a cached plan is shared by files that differ in it) and the
// context's per-encode counters; `end` is armed last.  orient (0 off, 1..8):
// tiles and file header are the upright image's -- `up` receives the layout
// with its width, height and resolution (the strips stay the stored image's).
int begin(jp2hip_ctx *ctx, const void *d_src, const jp2hip_layout *lay, int conversion, const jp2hip_recipe *recipe,
          const jp2hip_split *sp, int orient, jp2hip_recipe &rc, SourceMeta &meta, jp2hip_layout &up, EncodeEnd &end) {
    if (conversion != JP2HIP_LOSSY && conversion != JP2HIP_LOSSLESS)
        return fail("conversion must be JP2HIP_LOSSY (0) or JP2HIP_LOSSLESS (1)");
    const int world = sp ? sp->world : 1, rank = sp ? sp->rank : 0;
    if (world < 1 || rank < 0 || rank >= world) return fail("split: bad rank / world");
    if (world > 1 && !sp->allreduce_sum) return fail("split: world > 1 needs an allreduce_sum callback");
    rc = recipe_of(recipe, conversion);
    if (!lay || !d_src) return fail("null source or layout");
    if (orient < 0 || orient > 8) return fail("source orientation " + std::to_string(orient) + " is outside 0 .. 8");
    up = *lay;
    oriented_header(up, orient);
    std::string terr;  // tile_w = tile_h = 0: one tile for this image
    if (!resolve_tiles(rc, up.width, up.height, terr)) return fail(terr);
    // fixed-slope layers: the thresholds against this encode's recipe (refused
    // before the encode begins: the context stays as it was)
    if (!check_layer_slopes(ctx->slopes.data(), (int)ctx->slopes.size(), &rc, terr)) return fail(terr);
    // per-layer rates likewise
    if (!check_layer_rates(ctx->rates.data(), (int)ctx->rates.size(), &rc, terr)) return fail(terr);
    // PSNR targets likewise
    if (!check_layer_psnr(ctx->psnr.data(), (int)ctx->psnr.size(), &rc, terr)) return fail(terr);
    meta = source_meta(up);  // (a split: rank 0's file header; equal on all ranks, jp2hip.h)
    ctx->gpu.take_waits();     // count this encode's host waits (stats)
    ctx->gpu.begin_encode();
    ctx->reused = ctx->ended;  // (stats: how the call before this one ended)
    ctx->ended = 0;
    end.ctx = ctx;
    return 0;
}

// One rank's part of the file: the file and main headers (with_main: rank
// 0), the tile-parts it coded (have), EOC (with_eoc: the last rank).  The
// single encode is the one rank that has all three.
struct FilePart {
    const Plan &file, &coded;  // names the file (the plan / a split's full plan); was coded here (the plan / sub)
    bool with_main, with_eoc, have;
    size_t fh = 0, head = 0, bytes = 0;  // file header; through the main header (its TLM included); the whole part
    size_t tlm = 0;                      // the TLM marker segments that end the main header (with_main)
    const uint8_t *tlm_host = nullptr;   // ... written on the host (a split's rank 0); null: by the device
    void size(const SourceMeta &meta, size_t mh_bytes, int64_t part_bytes, size_t tlm_segs) {
        fh = with_main ? file_header_bytes(file, meta) : 0;
        tlm = with_main ? tlm_segs : 0;
        head = with_main ? fh + mh_bytes + tlm : 0;
        bytes = head + (size_t)(have ? part_bytes : 0) + (with_eoc ? 2 : 0);
    }
};

// Writes part `fp` into `buf` (pinned, fp.bytes long; released here on
// failure) and hands it to the caller with the encode's stats.  K: the final
// selection's slope keys; tp_hdr, layer_bytes, cs_bytes: whole-image sums
// (Kdu-Layer-Info, the file header's code-stream length); file_bytes: the
// whole file; dist: the layer report's whole-image distortions (null: not
// enabled).  The rank that writes the main header keeps the layer report.
int finish_part(jp2hip_ctx *ctx, const FilePart &fp, const SourceMeta &meta, std::vector<uint64_t> K, int64_t tp_hdr,
                const int64_t *layer_bytes, int64_t cs_bytes, const T2Summary &sum, uint8_t *buf, StageTimes &st,
                uint8_t **out, size_t *out_len, jp2hip_stats *stats, double t_start, double h2d_ms,
                int64_t file_bytes, int iters, const double *dist) {
    const Plan &P = fp.file;
    std::string err;
    struct jp2hip_layer_report rep;  // kept on success
    std::memset(&rep, 0, sizeof rep);
    if (fp.with_main) {
        // Kdu-Layer-Info: the slope keys (lossless: the last layer takes
        // every pass) and the code-stream bytes through each layer
        const int L = P.rc.layers;
        if (P.rc.rate_bpp <= 0.0) K[L - 1] = 0;
        std::vector<int64_t> layer_end((size_t)L);
        int64_t acc = (int64_t)(fp.head - fp.fh) + tp_hdr;
        for (int l = 0; l < L; l++) layer_end[l] = acc += layer_bytes[l];
        std::vector<uint8_t> mh;
        main_header(P, mh, K.data(), layer_end.data());
        struct jp2hip_layer_report &r = rep;
        r.layers = L;
        r.distortion_valid = dist != nullptr;
        for (int l = 0; l < L; l++) {
            if (K[l] >= 0x7FF0000000000000ull) r.threshold[l] = HUGE_VAL;  // nothing taken
            else std::memcpy(&r.threshold[l], &K[l], 8);
            r.bytes[l] = layer_end[l];
            r.distortion[l] = dist ? dist[l] : std::nan("");
        }
        write_file_header(P, meta, (uint64_t)cs_bytes, buf);
        std::memcpy(buf + fp.fh, mh.data(), mh.size());
        if (fp.tlm_host) std::memcpy(buf + fp.head - fp.tlm, fp.tlm_host, fp.tlm);
    }
    const bool prof = ctx->cfg.profile != 0;
    // the device writes the TLM segments in front of its tile-parts: one copy brings both
    const size_t dev_tlm = fp.tlm_host ? 0 : fp.tlm;
    if (fp.have && (!ctx->gpu.t2_emit(fp.coded, dev_tlm, (uint64_t)sum.part_bytes, buf + fp.head - dev_tlm, prof, st, err) ||
                    !ctx->gpu.collect_profile(st, err))) {
        out_free(buf);
        return fail(err);
    }
    if (fp.with_eoc) {
        buf[fp.bytes - 2] = 0xFF;
        buf[fp.bytes - 1] = 0xD9;
    }
    *out = buf;
    *out_len = fp.bytes;
    ctx->report = rep;
    ctx->report_set = fp.with_main;
    if (!stats) return 0;
    std::memset(stats, 0, sizeof *stats);
    stats->total_ms = now_ms() - t_start;
    stats->h2d_ms = h2d_ms;
    stats->ingest_ms = st.ingest;
    stats->dwt_ms = st.dwt;
    stats->quant_ms = st.quant;
    stats->t1_ms = st.t1_cm + st.t1_mq;
    stats->t1_cm_ms = st.t1_cm;
    stats->t1_mq_ms = st.t1_mq;
    stats->pcrd_ms = st.pcrd;
    stats->d2h_ms = st.d2h;
    stats->t2_ms = st.t2;
    stats->codeblocks = (int64_t)fp.coded.blocks.size();
    stats->t1_bytes = sum.t1_bytes;
    stats->coded_passes = sum.coded_passes;
    stats->out_bytes = file_bytes;
    stats->rate_iterations = iters;
    stats->host_waits = ctx->gpu.take_waits();
    stats->mq_decisions = sum.decisions;
    stats->stream_need_bytes = sum.stream_need;
    stats->stream_pool_bytes = (int64_t)ctx->gpu.stream_pool_bytes();
    stats->pool_grows = ctx->gpu.take_pool_grows();
    stats->reused = ctx->reused | ctx->gpu.reuse_bits();
    return 0;
}

}  // namespace

// The whole encode with the source already in device memory.  On success
// *out is the complete file in a pinned buffer from this library's pool
// (out_alloc; released with jp2hip_free).  Everything up to the code-stream
// bytes runs on the GPU (tier-2 included, t2_device.hip); the host picks the
// rate-control budgets from one small summary per pass and writes the file
// and main headers.
int encode_core(jp2hip_ctx *ctx, const void *d_src, size_t src_len, const jp2hip_layout *lay, int conversion,
                const jp2hip_recipe *recipe, uint8_t **out, size_t *out_len, jp2hip_stats *stats, double t_start,
                double h2d_ms, int orient) {
    jp2hip_recipe rc;
    SourceMeta meta;
    jp2hip_layout up;
    EncodeEnd end;
    if (begin(ctx, d_src, lay, conversion, recipe, nullptr, orient, rc, meta, up, end)) return -1;
    std::string err;
    jp2hip_layout ulay;
    std::vector<uint64_t> uoffs;
    UnitGrid grid;
    // (from here on `lay` is the upright image's: the plan, its cache key and
    // the rate targets see the oriented width and height)
    if (!unit_grid(*lay, grid, err) ||
        !prepare_source(ctx, grid, d_src, src_len, lay, 0, up.height, ulay, uoffs, err, orient))
        return fail(err);
    PlanCache &pc = ctx->pc;
    // per-layer rates (jp2hip_set_layer_rates): byte targets for the whole
    // image, so a lossless recipe's plan has one rate-control group, not the
    // flush stripes -- part of the cache's key (the rates themselves are not)
    const bool by_rates = !ctx->rates.empty();
    // PSNR targets (jp2hip_set_layer_psnr): a quality target is the whole
    // image's too -- the same bit of the key
    const bool by_psnr = !ctx->psnr.empty();
    const bool one_group = (by_rates || by_psnr) && rc.rate_bpp <= 0.0;
    if (!pc.valid || pc.w != lay->width || pc.h != lay->height || pc.nc != lay->components || pc.bits != lay->bits ||
        pc.one_group != one_group || std::memcmp(&pc.rc, &rc, sizeof rc) != 0) {
        pc.valid = false;
        pc.tabs_ok = false;
        if (!build_plan(pc.plan, rc, lay->width, lay->height, lay->components, lay->bits, err, one_group))
            return fail(err);
        main_header(pc.plan, pc.mh0, nullptr, nullptr);
        pc.rc = rc;
        pc.one_group = one_group;
        pc.w = lay->width; pc.h = lay->height; pc.nc = lay->components; pc.bits = lay->bits;
        pc.valid = true;
    } else {
        ctx->reused |= JP2HIP_REUSED_PLAN;
    }
    const Plan &plan = pc.plan;
    // the tile-part divisions are no part of the plan's key: other letters on
    // the same plan cut its tables anew
    if (!pc.tabs_ok || pc.tabs.letters != ctx->tparts) {
        pc.tabs_ok = false;
        t2_tables(plan, 0, plan.ntx * plan.nty, 0, pc.tabs, ctx->tparts);
        if (!tile_parts_fit(plan, pc.tabs, err)) return fail(err);
        // E (read by encodes with a target only: a lossless one without rates never sees it)
        pc.division_bytes = tile_part_division_bytes(plan, ctx->tparts, (int64_t)pc.tabs.tp.size());
        pc.tabs_ok = true;
    }
    const bool prof = ctx->cfg.profile != 0;
    StageTimes st;
    // the organisation is no part of the cached plan: its bytes come from the tile-part count alone
    const int64_t tlm = ctx->org.tlm ? tlm_bytes((int64_t)pc.tabs.tp.size()) : 0;
    if (ctx->org.tlm && (int64_t)pc.tabs.tp.size() > kTlmMaxEntries)
        return fail("tlm: more tile-parts than 256 TLM marker segments hold");
    // what the L / C divisions add (counted by encodes with a target)
    const int64_t E = rc.rate_bpp > 0.0 || by_rates ? pc.division_bytes : 0;
    // fixed-slope layers (jp2hip_set_layer_slopes): no target, so nothing is
    // predicted and every plane is coded
    const bool fixed = !ctx->slopes.empty();
    const std::vector<uint64_t> keys = slope_keys(ctx->slopes);
    int64_t skip_target = fixed || by_psnr ? -1 : skip_target_of(rc, plan.w, plan.h, tlm + E);
    // PSNR targets: the quanta each layer may leave; the hulls then come with
    // their histogram of quanta (set_psnr holds for this encode's run_front)
    int64_t qtarget[kMaxLayers] = {};
    if (by_psnr) {
        if (!quanta_fit(plan)) return fail("layer psnr: the distortion quanta of an image this large could overflow 63 bits");
        layer_psnr_targets(plan.w, plan.h, plan.nc, plan.bits, ctx->psnr.data(), rc.layers, qtarget);
    }
    ctx->gpu.set_psnr(by_psnr ? plan.bits : 0);
    // per-layer rates: every layer's target and first budget;
    // slope prediction aims at the top layer's target, the largest (a
    // lossless top layer: off)
    int64_t ltarget[kMaxLayers] = {}, lbudget[kMaxLayers] = {};
    if (by_rates) {
        layer_rate_targets(plan, ctx->rates.data(), rc.layers, tlm + E, ltarget, lbudget);
        skip_target = rc.slope_skip && rc.rate_bpp > 0.0 ? ltarget[rc.layers - 1] : -1;
        if (!ctx->gpu.rates_load(ltarget, lbudget, err)) return fail(err);
    }
    // tier-2 tables first: every host->device copy of the encode is issued
    // while the stream is idle (a copy queued behind kernels holds up the
    // copy engine for the other contexts)
    if (!ctx->gpu.t2_load(plan, pc.tabs, err)) return fail(err);
    if (!ctx->gpu.run_front(d_src, *lay, plan, prof, st, err, skip_target)) return fail(err);
    const size_t mh_bytes = pc.mh0.size();
    T2Summary sum;
    std::memset(&sum, 0, sizeof sum);
    int iters = 0;
    int64_t cs_bytes = 0;
    if (fixed || by_psnr || (rc.rate_bpp <= 0.0 && !by_rates)) {
        // lossless: per -flush_period stripe, layer l keeps the passes whose
        // slopes clear lossless_layer_frac(l) of the stripe's tier-1 bytes;
        // fixed slopes: layer l keeps the passes whose slopes clear the
        // caller's threshold, in every stripe (no target, no rate loop)
        for (int grow = 0;; grow++) {
            // PSNR targets: layer l keeps the passes whose slopes clear the
            // highest threshold that leaves at most qtarget[l] quanta
            if (!(fixed     ? ctx->gpu.select_keys(plan, keys, err)
                  : by_psnr ? ctx->gpu.select_psnr(plan, qtarget, err)
                            : ctx->gpu.select_lossless(plan, err)) ||
                !ctx->gpu.t2_size(plan, true, prof, st, sum, err))
                return fail(err);
            if ((sum.err & kErrSlotPool) && grow < 2) {
                // the decision-stream pool was short: again with the size
                // this encode needed (GpuEncoder::run_front)
                if (!ctx->gpu.pool_grow(err) || !ctx->gpu.run_front(d_src, *lay, plan, prof, st, err, skip_target))
                    return fail(err);
                continue;
            }
            break;
        }
        if (sum.err) return fail("tier-1 output capacity exceeded");
        iters = fixed || by_psnr ? 0 : 1;
        cs_bytes = (int64_t)mh_bytes + tlm + sum.part_bytes + 2;
        // (targets that do not decrease cannot give thresholds that increase)
        for (int l = 1; by_psnr && l < rc.layers; l++)
            if (sum.kc[l] > sum.kc[l - 1]) return fail("layer psnr: the thresholds found increase with the layer");
    } else {
        // the rate loop runs on the device (GpuEncoder::rate_loop): one
        // iteration per host wait, what the usual encode needs (its first
        // budget lands it under the target); an encode whose headers are
        // heavier takes a second wait for its next iterations
        RateState init;
        std::memset(&init, 0, sizeof init);
        // (by rates: the device reads the layers' targets and budgets from
        // what rates_load sent; these two fields are not used)
        init.target = by_rates ? ltarget[rc.layers - 1] : rate_target_of(rc, plan.w, plan.h, tlm + E);
        init.budget = by_rates ? lbudget[rc.layers - 1] : first_budget_of(plan, init.target);
        // the cs_bytes the loop compares leaves E out, as it leaves the TLM
        // out: the encode without letters, at the lower target
        init.fixed = (int64_t)mh_bytes + 2 - E;
        init.skip_target = skip_target;
        RateState rs;
        bool restart = true;
        for (int grow = 0;;) {
            if (!ctx->gpu.rate_loop(plan, init, restart, restart ? 1 : 2, prof, st, rs, sum, err, by_rates))
                return fail(err);
            restart = false;
            if ((sum.err & kErrSlotPool) && grow++ < 2) {
                // the decision-stream pool was short: again with the size
                // this encode needed (GpuEncoder::run_front)
                if (!ctx->gpu.pool_grow(err) ||
                    !ctx->gpu.run_front(d_src, *lay, plan, prof, st, err, init.skip_target))
                    return fail(err);
                restart = true;
                continue;
            }
            if (sum.err) return fail("tier-1 output capacity exceeded");
            if (rs.safety) {
                // slope prediction's safety net (oracle predict_and_code):
                // planes were skipped, yet every coded byte fits -> code all
                init.skip_target = -1;
                if (!ctx->gpu.run_front(d_src, *lay, plan, prof, st, err, -1)) return fail(err);
                restart = true;
                continue;
            }
            if (rs.halt) break;
        }
        iters = rs.iters;
        cs_bytes = rs.cs_bytes + tlm + E;  // (rs.cs_bytes = init.fixed + sum.part_bytes: device_common.h rate_step)
    }
    // the layer report's distortion, after the final selection (enabled only)
    double dist[kMaxLayers];
    if (ctx->report_on && !ctx->gpu.layer_dist(plan, dist, err)) return fail(err);
    FilePart fp{plan, plan, true, true, true};
    fp.size(meta, mh_bytes, sum.part_bytes, (size_t)tlm);
    uint8_t *buf = out_alloc(fp.bytes);
    if (!buf) return fail("out of (pinned) host memory");
    if (finish_part(ctx, fp, meta, std::vector<uint64_t>(sum.kc, sum.kc + rc.layers), sum.tp_hdr_bytes,
                    sum.layer_bytes, cs_bytes, sum, buf, st, out, out_len, stats, t_start, h2d_ms, (int64_t)fp.bytes,
                    iters, ctx->report_on ? dist : nullptr))
        return -1;
    end.ok = true;
    return 0;
}

// Tile-split encode (jp2hip.h, jp2hip_encode_device_split; split.cpp has the
// exchange rule).  Rank `rank` runs the device pipeline -- tier-2 included --
// on its band of tile rows only; budgets, thresholds and tier-2 sizes are
// agreed through sp->allreduce_sum so the parts concatenate to the
// single-GPU file.
int encode_split_core(jp2hip_ctx *ctx, const void *d_src, size_t src_len, const jp2hip_layout *lay, int conversion,
                      const jp2hip_recipe *recipe, const jp2hip_split *sp, uint8_t **out, size_t *out_len,
                      uint64_t *file_offset, uint64_t *file_len, jp2hip_stats *stats, double t_start, int orient) {
    jp2hip_recipe rc;
    SourceMeta meta;
    jp2hip_layout up;  // the upright image's width and height: what the plan and the bands are cut from
    EncodeEnd end;
    if (begin(ctx, d_src, lay, conversion, recipe, sp, orient, rc, meta, up, end)) return -1;
    const int world = sp ? sp->world : 1, rank = sp ? sp->rank : 0;
    std::string err;
    auto allreduce = [&](int64_t *v, int n) {
        return world <= 1 || sp->allreduce_sum(sp->user, v, (int32_t)n) == 0;
    };
    // An exchange that carries a failure flag in v[flag], so that a rank
    // which failed still joins it and the others learn of it: `ok` goes in
    // and comes back false if any rank failed (err: this rank's own text when
    // it failed first-hand).  Returns false when the exchange itself failed:
    // no later one can work, the caller returns.
    auto exchange = [&](std::vector<int64_t> &v, size_t flag, bool &ok) {
        v[flag] = ok ? 0 : 1;
        if (!allreduce(v.data(), (int)v.size())) {
            err = "split: all-reduce failed";
            return false;
        }
        if (ok && v[flag]) {
            ok = false;
            err = "split: another rank failed";
        }
        return true;
    };
    Plan full;
    UnitGrid grid;  // (the same on every rank: a layout it refuses fails them all here)
    if (!unit_grid(*lay, grid, err)) return fail(err);
    int enc_nc, enc_bits;  // the plan sees what the code-stream carries
    encoded_format(*lay, enc_nc, enc_bits);
    // per-layer rates (collective, like the slopes): a lossless recipe's plan
    // then has one rate-control group, and takes the rate-driven exchange
    const bool by_rates = !ctx->rates.empty();
    // PSNR targets likewise (collective): one group, and an exchange of their own
    const bool by_psnr = !ctx->psnr.empty();
    if (!build_plan(full, rc, up.width, up.height, enc_nc, enc_bits, err, (by_rates || by_psnr) && rc.rate_bpp <= 0.0))
        return fail(err);
    int64_t qtarget[kMaxLayers] = {};
    if (by_psnr) {  // (the full plan's: the same on every rank)
        if (!quanta_fit(full)) return fail("layer psnr: the distortion quanta of an image this large could overflow 63 bits");
        layer_psnr_targets(full.w, full.h, full.nc, full.bits, ctx->psnr.data(), rc.layers, qtarget);
    }
    ctx->gpu.set_psnr(by_psnr ? full.bits : 0);
    int tr0, tr1;
    if (untiled(recipe)) {  // one tile row, all of it rank 0's (jp2hip_split_rows with tile_h = 0)
        tr0 = rank ? 1 : 0;
        tr1 = 1;
    } else {
        split_tile_rows(full.nty, rc.tile_h, full.h, rc.flush_period, rank, world, tr0, tr1);
    }
    Plan sub;
    make_subplan(full, tr0, tr1, sub);
    const bool have = sub.ntc > 0;
    // only this rank's rows are read, so only their strips (or tiles) must be
    // in d_src; compressed / tiled units of the band are decoded here (a rank
    // that fails here still joins every exchange below).  With an orientation
    // the band is one of upright rows: 3 and 4 read the mirrored band's
    // strips, 5..8 the whole source (prepare_source)
    jp2hip_layout ulay;
    std::vector<uint64_t> uoffs;
    bool ok = !have ||
              prepare_source(ctx, grid, d_src, src_len, lay, sub.row0, sub.row0 + sub.band_h, ulay, uoffs, err, orient);
    const bool prof = ctx->cfg.profile != 0;
    StageTimes st;
    std::vector<uint64_t> keys;
    std::vector<int64_t> cum;
    // TLM (collective, like the recipe: every rank's context has the same
    // organisation): its bytes are known from the full plan alone (so a plan
    // with too many tile-parts fails every rank here, before any exchange)
    // The tile-part divisions are collective in the same way; a tile they cut
    // into too many parts fails every rank here as well.  ntp[t]: tile-parts
    // of the full plan's tiles before t (file order keeps a band's contiguous)
    const int letters = ctx->tparts;
    const int ntiles = full.ntx * full.nty;
    std::vector<int64_t> ntp((size_t)ntiles + 1, 0);
    if (ctx->org.tlm || letters) {
        std::vector<int> count;
        if (!tile_part_counts(full, letters, count, err)) return fail(err);
        for (int t = 0; t < ntiles; t++) ntp[(size_t)t + 1] = ntp[(size_t)t] + count[(size_t)t];
    }
    const int64_t ntp_full = ctx->org.tlm ? ntp[(size_t)ntiles] : 0;
    if (ntp_full > kTlmMaxEntries) return fail("tlm: more tile-parts than 256 TLM marker segments hold");
    const int64_t tlm = tlm_bytes(ntp_full);
    // E: what the L / C divisions add (encodes with a target only)
    const int64_t E =
        rc.rate_bpp > 0.0 || by_rates ? tile_part_division_bytes(full, letters, ntp[(size_t)ntiles]) : 0;
    // slope prediction over the whole image: the plane histogram is summed
    // over ranks (one all-reduce of kSlopeBins + 1 int64, the last a failure
    // flag, so a rank that failed earlier still joins the exchange)
    // fixed-slope layers (collective, like the organisation): no target,
    // nothing predicted, no threshold exchange
    const bool fixed = !ctx->slopes.empty();
    int64_t skip_target = fixed || by_psnr ? -1 : skip_target_of(rc, full.w, full.h, tlm + E);
    int64_t ltarget[kMaxLayers] = {}, lbudget[kMaxLayers] = {};
    if (by_rates) {  // (as encode_core)
        layer_rate_targets(full, ctx->rates.data(), rc.layers, tlm + E, ltarget, lbudget);
        skip_target = rc.slope_skip && rc.rate_bpp > 0.0 ? ltarget[rc.layers - 1] : -1;
    }
    bool hist_done = false;
    GpuEncoder::HistReduce reduce = [&](std::vector<int64_t> &h) {
        hist_done = true;
        std::vector<int64_t> v(h.size() + 1, 0);
        std::copy(h.begin(), h.end(), v.begin());
        bool all = true;
        if (!exchange(v, h.size(), all) || !all) return false;
        std::copy(v.begin(), v.end() - 1, h.begin());
        return true;
    };
    T2Tables tabs;  // loaded before the front (host->device copies on an idle stream)
    const int tile0 = sub.tile0, tile1 = sub.tile0 + full.ntx * (tr1 - tr0);
    if (ok && have) {
        t2_tables(full, tile0, tile1, sub.block0, tabs, letters);
        ok = ctx->gpu.t2_load(sub, tabs, err);
    }
    ok = ok && (!have || ctx->gpu.run_front(d_src, *lay, sub, prof, st, err, skip_target, &reduce, true));
    if (skip_target >= 0 && !hist_done) {  // no blocks here, or failed before the exchange
        std::vector<int64_t> v((size_t)kSlopeBins + 1, 0);
        if (!exchange(v, (size_t)kSlopeBins, ok)) return fail(err);
    }
    const int L = rc.layers;
    std::vector<int64_t> budgets((size_t)L, 0);
    std::vector<uint64_t> K((size_t)L);
    int iters = 0;
    int64_t cs_bytes = 0;
    T2Summary sum;
    std::memset(&sum, 0, sizeof sum);
    int64_t g_part = 0;                            // whole-image sums of the last pass: tile-part bytes,
    int64_t g_tp_hdr = 0;                          // tile-part header bytes and packet bytes per layer
    std::vector<int64_t> g_layer((size_t)L, 0);    // (Kdu-Layer-Info)
    std::vector<uint8_t> mh;
    main_header(full, mh, nullptr, nullptr);
    // One selection (rate-driven: at the thresholds of `budgets`) and tier-2
    // sizing pass, its sums exchanged: [0] part bytes, [1] failure flag, [2]
    // tile-part header bytes, [3..] packet bytes per layer (Kdu-Layer-Info),
    // then, lossless, L slope keys per rank.  False on failure (err).
    // fixed_keys: K holds the caller's thresholds, nothing about them is exchanged.
    auto round = [&](bool lossless, bool fixed_keys = false) -> bool {
        if (!lossless && !fixed_keys &&
            jp2hip_split_thresholds(keys.data(), cum.data(), (int64_t)keys.size(), budgets.data(), L, sp, K.data()) != 0) {
            err = "split: threshold exchange failed";
            return false;
        }
        bool rok = ok;
        if (rok && have)
            rok = (lossless ? ctx->gpu.select_lossless(sub, err) : ctx->gpu.select_keys(sub, K, err)) &&
                  ctx->gpu.t2_size(sub, lossless, prof, st, sum, err);
        if (rok && have && sum.err) {
            rok = false;
            err = "tier-1 output capacity exceeded";
        }
        std::vector<int64_t> v((size_t)L + 3 + (lossless ? (size_t)world * L : 0), 0);
        if (rok && have) {
            v[0] = sum.part_bytes;
            v[2] = sum.tp_hdr_bytes;
            for (int l = 0; l < L; l++) {
                v[3 + l] = sum.layer_bytes[l];
                if (lossless) v[3 + L + (size_t)rank * L + l] = (int64_t)sum.kc[l];  // (positive doubles: < 2^63)
            }
        }
        if (!exchange(v, 1, rok) || !rok) return false;
        g_part = v[0];
        cs_bytes = (int64_t)mh.size() + 2 + v[0] - E;  // (without E, as the target: added back below)
        g_tp_hdr = v[2];
        g_layer.assign(v.begin() + 3, v.begin() + 3 + L);
        iters++;
        for (int l = 0; lossless && l < L; l++) {  // a layer's key: the largest over the ranks' stripes
            K[l] = 0;
            for (int r = 0; r < world; r++) K[l] = std::max(K[l], (uint64_t)v[3 + L + (size_t)r * L + l]);
        }
        return true;
    };
    for (int attempt = 0; attempt < 2; attempt++) {
        if (fixed) {
            K = slope_keys(ctx->slopes);
            if (!round(false, true)) return fail(err);
            iters = 0;
            break;
        }
        if (by_psnr) {
            // every rank's segments with their quanta; the thresholds agreed
            // over the same all-reduce, then one round at those keys (a rank
            // that failed still joins every exchange)
            ok = ok && (!have || ctx->gpu.segments(sub, keys, cum, err, true));
            std::vector<int64_t> flag(1);
            if (!exchange(flag, 0, ok) || !ok) return fail(err);
            if (jp2hip_split_psnr_thresholds(keys.data(), cum.data(), (int64_t)keys.size(), qtarget, L, sp, K.data()) != 0)
                return fail("split: threshold exchange failed");
            for (int l = 1; l < L; l++)
                if (K[l] > K[l - 1]) return fail("layer psnr: the thresholds found increase with the layer");
            if (!round(false, true)) return fail(err);
            iters = 0;
            break;
        }
        if (attempt == 1) {  // the prediction's safety net, decided globally (below)
            keys.clear();
            cum.clear();
            ok = !have || ctx->gpu.run_front(d_src, *lay, sub, prof, st, err, -1, nullptr, true);
            skip_target = -1;
            iters = 0;
        }
        if (rc.rate_bpp <= 0.0 && !by_rates) {
            // lossless: every -flush_period stripe's layers come from its own
            // tier-1 bytes (the plan's rate-control groups; a rank holds
            // whole stripes), so the selection needs no exchange -- only the
            // part sizes, the Kdu-Layer-Info bytes and the slope keys are shared
            if (!round(true)) return fail(err);
            break;
        }
        ok = ok && (!have || ctx->gpu.segments(sub, keys, cum, err));
        std::vector<int64_t> flag(1);
        if (!exchange(flag, 0, ok) || !ok) return fail(err);
        const int64_t target = rate_target_of(rc, full.w, full.h, tlm + E);  // (cs_bytes: without the TLM and E, as the target)
        int64_t budget = first_budget_of(full, target);
        bool rerun = false;
        if (by_rates) budgets.assign(lbudget, lbudget + L);
        for (int it = 0; it < 8; it++) {
            if (budget < 0) budget = 0;
            for (int l = 0; l < L && !by_rates; l++) budgets[l] = budget >> (L - 1 - l);
            if (!round(false)) return fail(err);
            if (it == 0 && skip_target > 0) {
                int64_t v[2] = {have ? sum.t1_bytes : 0, have ? sum.skipped : 0};
                if (!allreduce(v, 2)) return fail("split: all-reduce failed");
                if (v[1] && v[0] < skip_target) { rerun = true; break; }
            }
            if (by_rates) {
                // every layer against its own target: the device loop's step
                // (layer_rate_step) on the whole image's sums
                if (layer_rate_step(L, it, (int64_t)mh.size() + 2 - E, g_part, g_layer.data(), ltarget,
                                    budgets.data()))
                    break;
                continue;
            }
            if (cs_bytes <= target) break;
            // exponential back-off + 1/16 of the overshoot + 64 B (device_common.h rate_step)
            budget -= ((cs_bytes - target) << it) + ((cs_bytes - target) >> 4) + 64;
        }
        if (!rerun) break;
    }
    // the layer report's distortion (collective in jp2hip_set_layer_report):
    // every rank's sums travel in its own slots of one exchange as bit
    // patterns, zeros elsewhere, and are added here in rank order
    double dist[kMaxLayers] = {};
    if (ctx->report_on) {
        double mine[kMaxLayers] = {};
        bool dok = !have || ctx->gpu.layer_dist(sub, mine, err);
        std::vector<int64_t> v((size_t)world * L + 1, 0);
        if (dok && have) std::memcpy(&v[(size_t)rank * L], mine, 8 * (size_t)L);
        if (!exchange(v, (size_t)world * L, dok) || !dok) return fail(err);
        for (int r = 0; r < world; r++)
            for (int l = 0; l < L; l++) {
                double d;
                std::memcpy(&d, &v[(size_t)r * L + l], 8);
                dist[l] += d;
            }
    }
    // this rank's part of the file.  Everything its emission allocates is
    // allocated before the ranks agree on the part sizes, so a rank that
    // cannot fails with the others (the failure slot sizes[world]); a HIP
    // error in the emission itself, after the exchange, fails this rank
    // alone: the caller treats any rank's failure as the encode's (jp2hip.h)
    FilePart fp{full, sub, rank == 0, rank == world - 1, have};
    fp.size(meta, mh.size(), sum.part_bytes, (size_t)tlm);
    uint8_t *buf = out_alloc(fp.bytes);
    bool ready = buf != nullptr;
    if (!ready) err = "out of (pinned) host memory";
    if (ready && have) ready = ctx->gpu.t2_reserve(sum.part_bytes, err);
    // TLM: this rank's tile-part lengths (Psot, file order) come off the
    // device before the exchange below, which carries the failure of a rank
    // that could not read them
    std::vector<uint32_t> tp_len;
    if (ready && have && tlm) {
        ready = ctx->gpu.t2_tp_lengths(tp_len, err);
        if (ready && (int64_t)tp_len.size() != ntp[(size_t)tile1] - ntp[(size_t)tile0]) {
            ready = false;
            err = "tlm: the band's tile-part count differs from its plan's";
        }
    }
    std::vector<int64_t> sizes((size_t)world + 1, 0);
    sizes[rank] = (int64_t)fp.bytes;
    if (!exchange(sizes, (size_t)world, ready) || !ready) {
        out_free(buf);
        return fail(err);
    }
    uint64_t off = 0, flen = 0;
    for (int r = 0; r < world; r++) {
        if (r < rank) off += (uint64_t)sizes[r];
        flen += (uint64_t)sizes[r];
    }
    // TLM: rank 0 owns the main header, so the ranks sum their lengths into
    // the file-order vector -- a rank's tile-parts are one contiguous run of
    // it (whole flush stripes, after those of the tiles before its band), the
    // other ranks add zeros -- kTlmChunk entries an exchange; every rank joins
    // every chunk, one with an empty band too.  Rank 0 then writes the
    // segments on the host with the function jp2hip_tlm_segments exports.
    std::vector<uint8_t> tlm_seg;
    if (tlm) {
        constexpr int64_t kTlmChunk = 1024;
        std::vector<int64_t> all((size_t)ntp_full, 0);
        const int64_t first = tp_len.empty() ? 0 : ntp[(size_t)tile0];
        for (size_t i = 0; i < tp_len.size(); i++) all[(size_t)first + i] = (int64_t)tp_len[i];
        for (int64_t c0 = 0; c0 < ntp_full; c0 += kTlmChunk)
            if (!allreduce(all.data() + c0, (int)std::min(kTlmChunk, ntp_full - c0))) {
                out_free(buf);
                return fail("split: all-reduce failed");
            }
        if (rank == 0) {
            std::vector<uint16_t> tiles;
            tile_part_order(full, 0, ntiles, tiles, letters);
            std::vector<uint32_t> lens(all.begin(), all.end());
            tlm_seg.resize((size_t)tlm);
            tlm_segments(tiles.data(), lens.data(), ntp_full, tlm_seg.data());
            fp.tlm_host = tlm_seg.data();
        }
    }
    cs_bytes += tlm + E;
    if (finish_part(ctx, fp, meta, K, g_tp_hdr, g_layer.data(), cs_bytes, sum, buf, st, out, out_len, stats, t_start,
                    0.0, (int64_t)flen, iters, ctx->report_on ? dist : nullptr))
        return -1;
    if (file_offset) *file_offset = off;
    if (file_len) *file_len = flen;
    end.ok = true;
    return 0;
}

}  // namespace jp2hip
