// gpu_encoder.h -- device side of one encode (buffers, stream, stage kernels).
#pragma once

#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <array>
#include <chrono>
#include <cstdint>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "jp2hip_internal.h"
#include "source_layout.h"
#include "stages.h"

namespace jp2hip {

struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    size_t want = 0;  // bytes the current encode asked for (need accounting)
};

struct StageTimes {
    double ingest = 0, dwt = 0, quant = 0, t1_cm = 0, t1_mq = 0, pcrd = 0, d2h = 0, t2 = 0;
};

struct T2Args;    // t2_device.hip
struct FrontJob;  // front.hip

// Every device buffer of a context, named once: the DevBuf members and
// bufs() (need accounting, trim, the destructor) both come from this list.
#define JP2HIP_DEVBUFS(X)                                                                                     \
    X(coef) X(blocks) X(order) X(bp) X(sm) X(P) X(dref) X(dsig) X(t1out) X(rates) X(dists) X(npasses)         \
    X(lengths) X(weight) X(nhull) X(hpass) X(hkey) X(budget) X(nl) X(lrate) X(err) X(tcw) X(tch) X(strips)    \
    X(src) X(segcnt) X(segoff) X(est) X(hist) X(pmin) X(mqspan) X(stage) X(soff) X(lzwseg) X(untiled)         \
    X(inflnk) X(segkey) X(llbuf0) X(llbuf1) X(ordkey) X(segval) X(thr) X(items) X(slotoff) X(stream_buf)      \
    X(counts) X(dspp) X(dbgbuf) X(t1fill) X(dbgsel)                                                           \
    /* PCRD selection (k_hull / k_select): slope-bin histogram, ticket + list fills, candidate lists */      \
    X(pcrd_hb) X(pcrd_hc) X(sel_ctl) X(sel_key) X(sel_size)                                                   \
    /* rate-control groups (Plan::grp_b0, then each group's first candidate slot) and each group's */        \
    /* tier-1 bytes (k_hull) */                                                                               \
    X(grptab) X(gtot)                                                                                         \
    /* device tier-2 (t2_device.hip) */                                                                       \
    X(hdist) X(rstate) X(t2ticket) X(t2prec) X(t2tp) X(t2tt) X(t2lblock) X(t2incl) X(t2pklen) X(t2pkoff)      \
    X(t2tplen) X(t2tphdr) X(t2tpoff) X(t2blkdst) X(t2out) X(t2sum) X(t2seq)                                   \
    /* S1b sample expansion (expand.hip): the 8-bit copy, its unit offsets and the colour table */           \
    X(expanded) X(exoff) X(exlut)                                                                             \
    /* S1c orientation (orient.hip): the upright copy and the stored image's strip offsets */                \
    X(oriented) X(oroff)                                                                                      \
    /* the layer report's per-workgroup distortion sums and their totals (k_layer_dist) */                   \
    X(ldist)                                                                                                  \
    /* an encode by per-layer rates: kMaxLayers targets, then kMaxLayers first budgets (rates_load) */        \
    X(ltarget)                                                                                                \
    /* an encode by PSNR targets: k_hull's histogram of distortion quanta per slope bin */                   \
    X(pcrd_hq)

// Owns all device memory of a context; buffers only grow while the context
// stays within its soft limit, so repeated encodes of the same geometry never
// allocate.  Every allocation goes through ensure(), which keeps the total
// (device_bytes) and refuses to pass the hard limit; trim() releases every
// buffer after an image that left the context above its soft limit.
class GpuEncoder {
  public:
    ~GpuEncoder();
    bool init(int device, std::string &err);

    // device memory held by this context's buffers
    size_t device_bytes() const { return held; }
    // hard: no buffer may take the total past it (the encode fails with an
    // error -- before its kernels, or between them on a stream that is then
    // drained -- instead of faulting); soft: an encode that leaves the
    // context above it releases every buffer at its end (trim)
    void set_limits(size_t soft, size_t hard) {
        mem_soft = soft;
        mem_hard = hard;
    }
    size_t soft_limit() const { return mem_soft; }
    size_t hard_limit() const { return mem_hard; }
    // releases every device buffer if more than `soft` bytes are held (the
    // stream must be idle: called after an encode's last wait); true if it did
    bool trim(size_t soft);
    // need accounting: begin_encode() clears every buffer's request, and
    // need_bytes() is what this encode asked for (held may be more: buffers
    // keep the size of the largest image since the last trim)
    void begin_encode() {
        for (DevBuf *b : bufs()) b->want = 0;
        expand_timed = false;
        orient_timed = false;
        reuse = 0;
        reuse_front_noted = false;
    }
    // what this encode found resident (jp2hip_stats.reused: the
    // JP2HIP_REUSED_* bits of the front's tables, the tier-2 tables and the
    // strip offsets); a record of the branches taken, read by nothing else
    int reuse_bits() const { return reuse; }
    size_t need_bytes() {
        size_t n = 0;
        for (DevBuf *b : bufs()) n += b->want;
        return n;
    }
    // called when hipMalloc fails: frees what other, idle contexts of the
    // device hold (api.cpp reclaim_idle); true if anything was released
    std::function<bool()> reclaim;
    // waits for the stream, ignoring its errors (failure paths: no buffer is
    // released or reused while kernels may still read it)
    void quiesce();
    template <typename T>
    bool ensure(DevBuf &b, size_t count, std::string &err);

    // host -> device copy of a source buffer into the internal `src` buffer
    bool upload_source(const void *host, size_t len, std::string &err);
    const void *source() const { return src.ptr; }
    // LZW / PackBits strips (+ Predictor 2) -> an uncompressed staging copy
    // in HBM; `out` describes it (offsets in out_offs).  untile = false
    // (sources that expand_samples reads next, which untiles itself): decoded
    // tiles stay tiles, one per entry of out_offs.  `g` is lay's grid
    // (source_layout.h unit_grid): lay's table holds exactly the units of
    // its height, each checked against the source (prepare_source.cpp)
    bool unpack_strips(const void *d_src, const jp2hip_layout &lay, const UnitGrid &g, jp2hip_layout &out,
                       std::vector<uint64_t> &out_offs, const void **d_out, std::string &err, bool untile = true);

    // S1b (expand.hip): the rows of `lay` -- uncompressed 1-, 2-, 4-bit
    // samples or palette indices (lut: 2^bits packed colours, else nullptr)
    // in units of grid `g` -> 8-bit samples in the `expanded` buffer, one
    // row-major strip; enqueued only
    bool expand_samples(const void *d_src, const jp2hip_layout &lay, const UnitGrid &g, const uint32_t *lut,
                        bool profile, const void **d_out, std::string &err);

    // S1c (orient.hip): upright rows [row0, row1) of the image `lay` stores
    // -- uncompressed strips of 8- or 16-bit samples -- under TIFF Orientation
    // o = 2..8, into the `oriented` buffer, plane after plane; enqueued only
    bool orient_samples(const void *d_src, const jp2hip_layout &lay, int o, int row0, int row1, bool profile,
                        const void **d_out, std::string &err);

    // Sums a slope-prediction histogram over the ranks of a tile-split
    // encode, in place; false = exchange failed (or another rank failed).
    using HistReduce = std::function<bool(std::vector<int64_t> &)>;
    // ingest, DWT, quantiser, tier-1, hulls; downloads per-block totals.
    // skip_target >= 0: rate-driven encode of skip_target bytes with slope
    // prediction (bit-planes far below the predicted threshold not coded;
    // 0 bytes is a target too: a few pixels at a few bits each); -1: off;
    // reduce (tile-split only) makes the prediction global.
    // pool_worst: size the decision-stream pool for every plane of every
    // block (the tile-split path, whose ranks cannot repeat an exchange);
    // else the encode may end with kErrSlotPool in its summary's err, and
    // the caller grows the pool (pool_grow) and encodes again.
    bool run_front(const void *d_src, const jp2hip_layout &lay, const Plan &plan, bool profile,
                   StageTimes &st, std::string &err, int64_t skip_target = -1,
                   const HistReduce *reduce = nullptr, bool pool_worst = false);
    // after an encode that ended with kErrSlotPool: the next run_front
    // sizes the pool for what that encode needed (+12.5 %)
    bool pool_grow(std::string &err);
    size_t stream_pool_bytes() const { return stream_buf.bytes; }
    int take_pool_grows() {
        const int g = pool_grows;
        pool_grows = 0;
        return g;
    }
    // lossless "-rate -": per -flush_period stripe (the plan's rate-control
    // groups), layer budgets lossless_layer_frac of the stripe's tier-1
    // bytes, computed on the device (enqueued only; t2_size reads the result)
    bool select_lossless(const Plan &plan, std::string &err);
    // per-block layer tables for explicit slope thresholds K[layer]
    // (tile-split: thresholds agreed across ranks)
    // (and fixed-slope layers: the caller's own), the same keys for every
    // rate-control group, shown as K and as Kc (T2Summary::kc)
    bool select_keys(const Plan &plan, const std::vector<uint64_t> &K, std::string &err);
    // quality layers by target PSNR (jp2hip_set_layer_psnr).  set_psnr before
    // run_front: bits > 0 makes its k_hull also histogram every hull segment's
    // distortion quantum for `bits`-bit samples (psnr_quantum.h) and the
    // candidate lists 64 bits wide; 0 (every other encode): neither exists.
    // select_psnr then finds, on the device, per layer the highest threshold
    // that leaves at most target[l] quanta (-1: the lossless top layer) and
    // applies it (enqueued only; t2_size reads the result, its kc the keys)
    void set_psnr(int bits) { psnr_bits = bits; }
    bool select_psnr(const Plan &plan, const int64_t *target, std::string &err);
    // jp2hip_layer_report's distortion: per layer, over the plan's blocks,
    // weight x the distortion decrease of the passes the final selection
    // (the thresholds in `thr`) leaves out; d[kMaxLayers]; one host wait
    bool layer_dist(const Plan &plan, double *d, std::string &err);
    // tier-2 on the device (t2_device.hip): tables for the tiles coded, one sizing
    // pass per layer table (one host wait: the summary), then the code-stream
    // part (tile-parts, in stream order) written in HBM and copied to host_dst
    bool t2_load(const Plan &plan, const T2Tables &T, std::string &err);
    bool t2_size(const Plan &plan, bool with_kc, bool profile, StageTimes &st, T2Summary &sum, std::string &err);
    // rate-driven encode: the whole rate loop on the device (RateState),
    // `batch` iterations enqueued per host wait; returns the final state and
    // the summary of the selection it stopped at.  restart = begin a new loop
    // (else continue the one on the device).
    // by_rates: an encode by per-layer rates -- the targets and first budgets
    // of rates_load steer every layer (rate_step_layers); init.budget and
    // init.target are not used
    bool rate_loop(const Plan &plan, const RateState &init, bool restart, int batch, bool profile, StageTimes &st,
                   RateState &rs, T2Summary &sum, std::string &err, bool by_rates = false);
    // an encode by per-layer rates: its layers' targets and first budgets
    // (kMaxLayers each; layer_rate_targets) into device memory through the
    // pinned staging, issued with the tier-2 tables while the stream is idle
    bool rates_load(const int64_t *target, const int64_t *first_budget, std::string &err);
    // the device code-stream buffer t2_emit writes, sized for part_bytes
    // (t2_emit reserves it too; the split path reserves before its exchange)
    bool t2_reserve(uint64_t part_bytes, std::string &err);
    // host_dst must be pinned (hipHostMalloc) memory.  tlm_bytes > 0: the
    // TLM marker segments of the part's tile-parts (k_t2_tlm; tlm_bytes is
    // jp2hip::tlm_bytes of their count) are written in front of them, and
    // host_dst receives tlm_bytes + part_bytes in the one copy
    bool t2_emit(const Plan &plan, uint64_t tlm_bytes, uint64_t part_bytes, uint8_t *host_dst, bool profile,
                 StageTimes &st, std::string &err);
    // the tile-part lengths (Psot) of the last sizing pass, in the part's
    // stream order (one host wait; the split's TLM exchange)
    bool t2_tp_lengths(std::vector<uint32_t> &lengths, std::string &err);
    // stage times of the last encode from its events (profile mode; call
    // after the encode's last host wait)
    bool collect_profile(StageTimes &st, std::string &err);
    // this encode's hull segments: slope keys (descending) and inclusive byte
    // sums -- quanta: inclusive sums of distortion quanta (after set_psnr)
    bool segments(const Plan &plan, std::vector<uint64_t> &keys, std::vector<int64_t> &cum, std::string &err,
                  bool quanta = false);
    hipStream_t get_stream() const { return stream; }
    int get_device() const { return device; }
    // the stream and the main buffers are on this context's device (a
    // tile-split member is checked before every split encode)
    bool check_residency(std::string &err);
    // host waits since the last call (stats: host_waits per encode)
    int take_waits() {
        const int w = waits;
        waits = 0;
        return w;
    }

  private:
    // debug: JP2HIP_DUMP_DIR=<dir> writes every stage's device buffer
    bool dump(const char *dir, const char *name, const DevBuf &b, size_t bytes, std::string &err);
    // run_front's stages, in its order (front.hip; hull_launch: pcrd.hip)
    bool front_reserve(FrontJob &j, std::string &err);
    bool front_upload(const FrontJob &j, std::string &err);
    bool front_first_args(FrontJob &j, std::string &err);
    bool front_ingest_dwt(const FrontJob &j, std::string &err);
    bool front_quant(const FrontJob &j, std::string &err);
    bool front_predict_items(const FrontJob &j, std::string &err);
    bool front_t1(const FrontJob &j, std::string &err);
    bool hull_launch(const Plan &plan, std::string &err);
    bool front_dumps(const FrontJob &j, std::string &err);
    bool apply_thresholds(const Plan &plan, const int *halt, std::string &err);
    void select_launch(const Plan &plan, const int *halt, const RateState *init = nullptr, RateState *rs = nullptr,
                       bool by_rates = false, const int64_t *qtarget = nullptr);
    T2Args t2_args(const Plan &plan) const;
    // tier-2 sizing; with rs (device rate loop) k_t2_total also runs the
    // loop's step, leaving state + summary at out_rs (host-mapped)
    void t2_size_launch(const Plan &plan, bool with_kc, const int *halt, RateState *rs = nullptr,
                        RateState *out_rs = nullptr, bool by_rates = false);
    bool host_wait(std::string &err);
    // The code-stream D2H on an SDMA engine (ROCr hsa_amd_memory_async_copy):
    // the HIP runtime moves a device -> pinned-host copy with a blit kernel
    // on the CUs (tests/tools/d2h_engine_probe.sh), which under load waits
    // for CU slots like any kernel.  The copy is queued behind `dma_dep`,
    // which the stream's last kernel (k_release_dma) sets to 0 after the
    // emission kernels, so it starts with no host round trip; the host
    // waits on `dma_done`.
    bool dma_init(std::string &err);
    bool dma_to_host(uint8_t *host_dst, const void *src, size_t bytes, std::string &err);
    hsa_signal_t dma_dep{0}, dma_done{0};
    volatile hsa_signal_value_t *dma_dep_val = nullptr;
    hsa_agent_t dma_gpu{0}, dma_cpu{0};
    int dma_engine = -1;  // SDMA engine of this context (-1: the runtime's choice)
    bool dma_ok = false, hsa_up = false;
    // host -> device copy through this context's pinned staging memory: a
    // pageable source goes through the runtime's shared staging buffer and
    // blocks until the stream reaches the copy, serialising the contexts
    bool h2d(void *dst, const void *src, size_t bytes, std::string &err);
    struct PinnedChunk {
        uint8_t *p;
        size_t cap;
    };
    std::vector<PinnedChunk> stg;
    size_t stg_used = 0;
    hipEvent_t stg_ev = nullptr;  // after the last staged copy
    // Timing events on the stream, in the order an encode records them; what
    // lies between two of them is a StageTimes field (collect_profile,
    // t2_size, rate_loop, t2_emit).
    enum Ev {
        kEvFrontBegin,   // run_front: .. kEvDwtBegin = ingest (nothing is launched between them)
        kEvDwtBegin,     // .. kEvDwtEnd = dwt (k_ingest when there is no decomposition)
        kEvDwtEnd,       // .. kEvQuantEnd = quant (quantiser, slope prediction, tier-1 items)
        kEvQuantEnd,
        kEvCmBegin,      // .. kEvCmEnd = t1_cm
        kEvCmEnd,        // .. kEvMqEnd = t1_mq
        kEvMqEnd,        // .. kEvHullEnd = pcrd (k_hull)
        kEvHullEnd,
        kEvSelectBegin,  // .. kEvSelectEnd = pcrd (k_select, k_apply); .. kEvT2End = t2 (rate_loop)
        kEvSelectEnd,
        kEvT2Begin,      // .. kEvT2End = t2 (t2_size) or d2h (t2_emit)
        kEvT2End,
        kEvExpandBegin,  // expand_samples: .. kEvExpandEnd = ingest (k_expand; before kEvFrontBegin)
        kEvExpandEnd,
        kEvOrientBegin,  // orient_samples: .. kEvOrientEnd = ingest (k_orient_*; before kEvFrontBegin)
        kEvOrientEnd,
        kNumEvents
    };
    int device = 0;
    int waits = 0;
    hipEvent_t sync_ev = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[kNumEvents] = {};
#define X(name) DevBuf name;
    JP2HIP_DEVBUFS(X)
#undef X
    RateState *h_rs = nullptr;      // host-mapped: rate state, then the T2Summary (k_rate_step)
    RateState *d_rs_out = nullptr;  // its device address
    int t2_nprec = 0, t2_ntp = 0;
    bool t2_wave = true;  // precincts of <= 64 blocks: k_t2_wave (layer assignment fused in)
    bool t2_seq = false;  // a progression order other than RPCL: t2seq holds its forward map
    uint64_t front_gen = 0, t2_gen = 0;  // plan generation whose tables are resident
    int t2_letters = 0;                  // ... and the tile-part divisions of the tier-2 tables
    int reuse = 0;                   // reuse_bits() of the current encode
    bool reuse_front_noted = false;  // (its first run_front is the one noted: a repeat finds its own uploads)
    T2Summary *h_sum = nullptr;
    double *h_dist = nullptr;  // pinned [kMaxLayers]: layer_dist's result
    int64_t *h_tot = nullptr;  // pinned [8]: t1 total, -, k_t1_mq span[2], unpack error, segment tail[2]
    bool profiled = false;
    bool expand_timed = false;  // this encode recorded kEvExpandBegin / End
    bool orient_timed = false;  // ... kEvOrientBegin / End
    int nseg = 0;  // hull segments at most: the bound sum(3 Mb - 2)
    int psnr_bits = 0;  // set_psnr: the sample depth of an encode by PSNR targets, 0 = any other encode
    std::vector<int64_t> h_hist;
    std::vector<uint64_t> strips_host;  // strip offsets last uploaded to `strips`
    const void *strips_dev = nullptr;
    size_t held = 0, mem_soft = SIZE_MAX, mem_hard = SIZE_MAX;
    static constexpr int kReclaimWaitMs = 30000;
    // hipMalloc, or hipErrorOutOfMemory past JP2HIP_TEST_DEVICE_BYTES held by
    // every context of the process together (tests: a small device)
    hipError_t device_alloc(void **p, size_t n);
    void device_free(DevBuf &b);
    // decision-stream pool: the first encode of a geometry reserves this
    // fraction of the every-plane bound; pool_hint = what the last
    // overflowing encode needed (+12.5 %)
    static constexpr double kPoolFracLossy = 0.3, kPoolFracLossless = 0.7;
    uint64_t pool_hint = 0;
    int pool_grows = 0;
    double pool_frac_test = -1.0;  // JP2HIP_TEST_POOL_FRAC (tests: force the grow path)
#define X(name) +1
    static constexpr int kNumBufs = 0 JP2HIP_DEVBUFS(X);
#undef X
#define X(name) &name,
    std::array<DevBuf *, kNumBufs> bufs() { return {{JP2HIP_DEVBUFS(X)}}; }
#undef X
};

// Grows b to at least count T's (12.5 % headroom), within the hard limit.
template <typename T>
bool GpuEncoder::ensure(DevBuf &b, size_t count, std::string &err) {
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    if (bytes > b.want) b.want = bytes;  // (also when the buffer is big enough already)
    if (b.bytes >= bytes) return true;
    const size_t alloc = bytes + bytes / 8;
    if (held - b.bytes + alloc > mem_hard) {
        err = "device memory limit: this image needs a " + std::to_string(alloc) + "-byte buffer, the context holds " +
              std::to_string(held) + " of its " + std::to_string(mem_hard) + " bytes";
        return false;
    }
    device_free(b);
    hipError_t e = device_alloc(&b.ptr, alloc);
    // out of device memory: other contexts of this device that are idle give
    // their buffers back (they reallocate at their next encode), and an
    // encode in progress elsewhere is waited for -- up to kReclaimWaitMs --
    // before this encode fails
    // (every round counts 5 ms against the wait, freed or not, so two
    // contexts taking memory from each other cannot loop for ever)
    for (int waited = 0; e == hipErrorOutOfMemory && reclaim && waited <= kReclaimWaitMs; waited += 5) {
        (void)hipGetLastError();
        if (!reclaim()) std::this_thread::sleep_for(std::chrono::milliseconds(5));
        e = device_alloc(&b.ptr, alloc);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        b.ptr = nullptr;
        err = std::string("hipMalloc(") + std::to_string(alloc) + "): " + hipGetErrorString(e);
        return false;
    }
    b.bytes = alloc;
    held += alloc;
    return true;
}

}  // namespace jp2hip
