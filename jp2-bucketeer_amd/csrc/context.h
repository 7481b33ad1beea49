// context.h -- what the host sources behind the C ABI share (api.cpp,
// encode.cpp, split_host.cpp): the context, its plan cache, the
// end-of-encode memory policy and the error report.  Private to csrc.
#pragma once

#include <mutex>
#include <string>
#include <vector>

#include "gpu_encoder.h"
#include "jp2hip.h"
#include "jp2hip_internal.h"
#include "mem_policy.h"

// The last geometry's plan, tier-2 tables and main-header length: a batch of
// same-size images (the common case) builds them once (C2: ~5 ms of host
// time per encode otherwise), and the device keeps their tables resident.
struct PlanCache {
    bool valid = false;
    jp2hip_recipe rc;
    int w = 0, h = 0, nc = 0, bits = 0;
    // part of the key: a lossless recipe encoded by per-layer rates has one
    // rate-control group, not the flush stripes (Plan::one_group)
    bool one_group = false;
    jp2hip::Plan plan;
    // the tables are the plan's cut by the context's tile-part divisions
    // (tabs.letters; tabs_ok false: none built for this plan yet), which are
    // no part of the key above: a change of letters rebuilds the tables alone
    jp2hip::T2Tables tabs;
    bool tabs_ok = false;
    int64_t division_bytes = 0;  // tile_part_division_bytes of (plan, tabs.letters)
    std::vector<uint8_t> mh0;
};

struct jp2hip_ctx {
    std::mutex mu;
    // whole tile-split encodes on this context, one at a time: each rank
    // takes its member's `mu`, so two concurrent splits could otherwise hold
    // one member each and wait for each other in an exchange
    std::mutex split_mu;
    jp2hip::GpuEncoder gpu;
    jp2hip_config cfg;
    int threads = 1;
    PlanCache pc;
    // jp2hip_set_organisation: read by every encode, no part of the plan
    // cache's key (the plan, its tables and the main header up to the TLM
    // are the same with and without it)
    jp2hip_organisation org{};
    // jp2hip_set_tile_part_divisions: JP2HIP_TPARTS_L | _C, read by every
    // encode; the tier-2 tables depend on it, the plan does not
    int32_t tparts = 0;
    // jp2hip_set_layer_slopes: the layers' thresholds (empty: off), read by
    // every encode, no part of the plan cache's key; jp2hip_set_layer_report
    // and what the last successful encode's layers came to
    std::vector<double> slopes;
    // jp2hip_set_layer_rates: the bound (bpp) on the code-stream through each
    // layer (empty: off; excludes slopes), read by every encode.  The rates
    // are no part of the plan cache's key; that they are set is, for a
    // lossless recipe (PlanCache::one_group)
    std::vector<double> rates;
    // jp2hip_set_layer_psnr: the predicted PSNR (dB) each layer must reach
    // (empty: off; excludes slopes and rates), read by every encode.  As with
    // the rates, that targets are set is part of the plan cache's key for a
    // lossless recipe (PlanCache::one_group), the targets are not
    std::vector<double> psnr;
    // jp2hip_set_source_orientation: JP2HIP_ORIENT_OFF, 1..8 or
    // JP2HIP_ORIENT_TIFF, read by every encode, no part of the recipe (the
    // plan cache's key holds the upright width and height it leads to)
    int32_t orient = 0;
    int32_t report_on = 0;
    bool report_set = false;
    struct jp2hip_layer_report report{};
    // tile-split members (jp2hip_split_peers): images of at least
    // split_min_pixels are encoded by this context (rank 0) and these
    // (ranks 1..), owned here
    std::vector<jp2hip_ctx *> peers;
    int64_t split_min_pixels = 0;
    // device memory policy (jp2hip_set_memory_limits): 0 = default
    int64_t mem_soft = 0;
    size_t dev_total = 0;  // the device's memory (hipMemGetInfo at create)
    std::vector<size_t> needs;  // what the last encodes asked for (the context's usual image)
    int64_t reclaimed = 0;      // times another context took this one's idle buffers
    // jp2hip_stats.reused: how the last call that began an encode ended
    // (JP2HIP_AFTER_TRIM, JP2HIP_AFTER_FAILURE; set by EncodeEnd), and the
    // current encode's bits (begin takes `ended` over; the plan cache adds its own)
    int ended = 0, reused = 0;
    ~jp2hip_ctx() {
        for (jp2hip_ctx *p : peers) jp2hip_destroy(p);
    }
};

// Sets this thread's jp2hip_last_error() text (api.cpp); returns -1.
namespace jp2hip {
int fail(const std::string &msg);
}

// Every encode ends here, success or not: a failed one drains the stream
// first (no buffer is released while a kernel may still read it), then the
// context's device-memory policy decides whether it keeps its buffers.
//  - an explicit soft limit (jp2hip_set_memory_limits): release everything
//    when the context holds more;
//  - by default, relative to the context's usual image: release everything
//    when it holds more than twice the median of what its last 8 encodes
//    needed (plus 256 MiB) -- one C5-class master in a pool of C2 / C4 work
//    is released right after it, while a steady run of large masters (C3
//    every time) keeps its buffers instead of reallocating per image.
// Memory pressure between contexts is handled where it arises: an
// allocation that fails takes back what idle contexts of the device hold
// (api.cpp reclaim_idle).  `ctx` stays null until the encode has begun
// (encode.cpp begin_encode): a call refused before that leaves the context
// as it was.
struct EncodeEnd {
    jp2hip_ctx *ctx = nullptr;
    bool ok = false;
    ~EncodeEnd() {
        if (!ctx) return;
        if (!ok) ctx->gpu.quiesce();
        ctx->ended = ok ? 0 : JP2HIP_AFTER_FAILURE;
        if (ok) jp2hip::record_need(ctx->needs, ctx->gpu.need_bytes());
        const size_t limit = jp2hip::keep_limit(ctx->needs, ctx->mem_soft);  // (mem_policy.h)
        if (ctx->gpu.device_bytes() > limit) {
            ctx->gpu.quiesce();
            if (ctx->gpu.trim(limit)) ctx->ended |= JP2HIP_AFTER_TRIM;
        }
    }
};
