// api.cpp -- the C ABI of libjp2hip (include/jp2hip.h) and nothing else:
// contexts and their registry, the device queries, the layout and header
// entry points, and the encode entry points, which lock the context and call
// encode.cpp (one encode on one context) or split_host.cpp (one image across
// a context and its peers).
//
// jp2hip_encode_file() is the in-process replacement for the kdu_compress
// child process that KakaduConverter.convert() spawns
// (KakaduConverter.java:55-77 -> AbstractConverter.run, AbstractConverter.java:29-39):
// same inputs (TIFF path, output path, Conversion), same recipe, blocking,
// and every failure surfaces as a negative return code plus a message,
// never as a partially written output file.
//
// Which bytes of a source hold the image -- the TIFF parser, the pixel-format
// rules, the strip / tile grid and the bounds of the units a band of rows
// reads -- is decided in source_layout.cpp (no HIP in it; the CPU suite runs
// it under ASan / UBSan); encode.cpp prepare_source applies that to an encode.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "context.h"
#include "encode.h"
#include "orient_map.h"
#include "pinned_pool.h"
#include "psnr_quantum.h"
#include "source_layout.h"

namespace jp2hip {

static thread_local std::string g_err;

int fail(const std::string &msg) {
    g_err = msg;
    return -1;
}

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// The library's pinned output pool (pinned_pool.h has the rules).
static PinnedPool &pinned_pool() {
    static PinnedPool *p = new PinnedPool(  // never destroyed: buffers may be freed at exit
        [](size_t n) -> void * {
            void *b = nullptr;
            return hipHostMalloc(&b, n, hipHostMallocDefault) == hipSuccess ? b : nullptr;
        },
        [](void *b) { (void)hipHostFree(b); });
    return *p;
}
uint8_t *out_alloc(size_t n) { return pinned_pool().alloc(n); }
void out_free(void *p) { pinned_pool().free(p); }

// JP2HIP_ORIENT_TIFF is resolved where a TIFF is parsed: the file's own tag
// (the parse has accepted the file, so the tag reads as 1..8).
int source_orientation(const jp2hip_ctx *ctx, const uint8_t *tiff, size_t len) {
    return ctx->orient == JP2HIP_ORIENT_TIFF ? std::max(1, tiff_orientation(tiff, len)) : ctx->orient;
}

}  // namespace jp2hip

using namespace jp2hip;

namespace {

// jp2hip_encode_device and _split under JP2HIP_ORIENT_TIFF: a caller's layout names no tag
const char *const kOrientNeedsTiff =
    "source orientation: JP2HIP_ORIENT_TIFF needs the TIFF itself, and this call takes a caller's layout -- read the "
    "tag with jp2hip_tiff_orientation and give its value to jp2hip_set_source_orientation";

// Contexts alive in this process (jp2hip_env_check).
std::atomic<int> g_live_contexts{0};

// The TIFF parser (source_layout.cpp), reporting as this file does.
int read_tiff(const uint8_t *buf, size_t len, jp2hip_layout *lay, std::vector<uint64_t> &offs) {
    std::string err;
    return jp2hip::parse_tiff(buf, len, lay, offs, err) ? 0 : fail(err);
}

// A read-only mapping of a whole file (the split path reads each rank's band
// of a multi-GB TIFF straight from the page cache, in parallel).
struct MappedFile {
    int fd = -1;
    const uint8_t *p = nullptr;
    size_t n = 0;
    bool open(const char *path) {
        fd = ::open(path, O_RDONLY | O_CLOEXEC);
        if (fd < 0) return false;
        struct stat sb;
        if (fstat(fd, &sb) != 0 || sb.st_size <= 0) return false;
        n = (size_t)sb.st_size;
        void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) return false;
        p = (const uint8_t *)m;
        return true;
    }
    ~MappedFile() {
        if (p) munmap((void *)p, n);
        if (fd >= 0) ::close(fd);
    }
};

// The output is written under a temp name of its own (per process and
// thread) and renamed into place once complete (commit), else removed: a
// reader never sees a partial file.
struct TempOutput {
    const char *out_path;
    const std::string name;
    bool committed = false;
    explicit TempOutput(const char *path)
        : out_path(path),
          name(std::string(path) + ".part-" + std::to_string((long)getpid()) + "-" +
               std::to_string((unsigned long)std::hash<std::thread::id>()(std::this_thread::get_id()) % 100000)) {}
    bool commit() { return committed = std::rename(name.c_str(), out_path) == 0; }
    ~TempOutput() {
        if (!committed) std::remove(name.c_str());
    }
};

}  // namespace

extern "C" {

const char *jp2hip_version(void) { return "jp2hip 0.1.0 (gfx950)"; }

const char *jp2hip_last_error(void) { return g_err.c_str(); }

int jp2hip_probe(void) { return jp2hip_device_ordinals(nullptr, 0) > 0; }

int jp2hip_device_ordinals(int32_t *ordinals, int32_t max) {
    int n = 0, k = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) {
            if (ordinals && k < max) ordinals[k] = i;
            k++;
        }
    }
    return k;
}

int jp2hip_device_count(void) { return jp2hip_device_ordinals(nullptr, 0); }

void jp2hip_recipe_init(jp2hip_recipe *recipe, int conversion) {
    if (recipe) default_recipe(recipe, conversion);
}

// Every context alive in the process, by device: an allocation that fails
// for lack of device memory takes back the buffers of idle contexts of its
// device (GpuEncoder::reclaim -> reclaim_idle).  A context is idle when its
// lock is free (no encode in it); its buffers are rebuilt by its next encode.
static std::mutex g_reg_mu;
static std::vector<jp2hip_ctx *> g_reg;

static bool reclaim_idle(jp2hip_ctx *self) {
    bool freed = false;
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (jp2hip_ctx *c : g_reg) {
        if (c == self || c->cfg.device != self->cfg.device) continue;
        std::unique_lock<std::mutex> cl(c->mu, std::try_to_lock);
        if (!cl.owns_lock() || c->gpu.device_bytes() == 0) continue;
        c->gpu.quiesce();
        freed = c->gpu.trim(0) || freed;
        c->reclaimed++;
    }
    return freed;
}

const char *jp2hip_env_check(void) {
    thread_local std::string msg;
    msg.clear();
    const char *q = std::getenv("GPU_MAX_HW_QUEUES");
    const int queues = q && *q ? std::atoi(q) : 4;  // HIP's default
    const int live = g_live_contexts.load();
    if (live > queues)
        msg += "GPU_MAX_HW_QUEUES=" + std::to_string(queues) + " is below the " + std::to_string(live) +
               " contexts of this process (contexts sharing a hardware queue run their kernels one after "
               "another; set it to contexts per GPU + 4 before the library loads); ";
    if (!msg.empty()) msg.resize(msg.size() - 2);
    return msg.c_str();
}

int jp2hip_create(jp2hip_ctx **out, const jp2hip_config *cfg) {
    if (!out) return fail("null output pointer");
    *out = nullptr;
    jp2hip_ctx *c = new (std::nothrow) jp2hip_ctx();
    if (!c) return fail("out of memory");
    std::memset(&c->cfg, 0, sizeof c->cfg);
    if (cfg) c->cfg = *cfg;
    int hw = (int)std::thread::hardware_concurrency();
    c->threads = c->cfg.host_threads > 0 ? c->cfg.host_threads : std::max(1, std::min(16, hw));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        delete c;
        return fail("no HIP device visible (libjp2hip needs an MI355X / gfx950)");
    }
    if (c->cfg.device < 0 || c->cfg.device >= ndev) {
        delete c;
        return fail("device ordinal " + std::to_string(c->cfg.device) + " out of range (" + std::to_string(ndev) +
                    " visible)");
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->cfg.device) != hipSuccess ||
        std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        delete c;
        return fail("device " + std::to_string(c->cfg.device) + " is not a gfx950 (MI355X) device");
    }
    std::string err;
    if (!c->gpu.init(c->cfg.device, err)) {
        delete c;
        return fail(err);
    }
    size_t fr = 0, tot = 0;
    c->dev_total = hipMemGetInfo(&fr, &tot) == hipSuccess ? tot : 0;  // (init selected the device)
    c->gpu.reclaim = [c] { return reclaim_idle(c); };
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        g_reg.push_back(c);
    }
    *out = c;
    g_live_contexts++;
    return 0;
}

int64_t jp2hip_device_bytes(jp2hip_ctx *ctx) {
    if (!ctx) return 0;
    int64_t n;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        n = (int64_t)ctx->gpu.device_bytes();
    }
    for (jp2hip_ctx *p : ctx->peers) n += jp2hip_device_bytes(p);
    return n;
}

int jp2hip_set_memory_limits(jp2hip_ctx *ctx, int64_t soft, int64_t hard) {
    if (!ctx) return fail("null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->mem_soft = soft > 0 ? soft : 0;
    ctx->gpu.set_limits(ctx->gpu.soft_limit(), hard > 0 ? (size_t)hard : SIZE_MAX);
    for (jp2hip_ctx *p : ctx->peers)
        if (jp2hip_set_memory_limits(p, soft, hard) != 0) return -1;
    return 0;
}

int jp2hip_set_organisation(jp2hip_ctx *ctx, const jp2hip_organisation *org) {
    jp2hip_organisation o;
    std::memset(&o, 0, sizeof o);
    if (org) o = *org;
    if (o.tlm != 0 && o.tlm != 1) return fail("organisation: tlm must be 0 or 1, not " + std::to_string(o.tlm));
    for (int32_t r : o.reserved)
        if (r != 0) return fail("organisation: reserved must be 0");
    if (!ctx) return fail("null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->org = o;
    for (jp2hip_ctx *p : ctx->peers)
        if (jp2hip_set_organisation(p, &o) != 0) return -1;
    return 0;
}

int jp2hip_set_source_orientation(jp2hip_ctx *ctx, int32_t o) {
    if (o < JP2HIP_ORIENT_OFF || o > JP2HIP_ORIENT_TIFF)
        return fail("source orientation: " + std::to_string(o) + " is neither JP2HIP_ORIENT_OFF (0), a TIFF Orientation " +
                    "(1 .. 8) nor JP2HIP_ORIENT_TIFF (9)");
    if (!ctx) return fail("null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->orient = o;
    for (jp2hip_ctx *p : ctx->peers)
        if (jp2hip_set_source_orientation(p, o) != 0) return -1;
    return 0;
}

int32_t jp2hip_tiff_orientation(const uint8_t *tiff, size_t len) {
    const int o = jp2hip::tiff_orientation(tiff, len);
    return o < 0 ? fail("tiff: not a TIFF file") : o;
}

int jp2hip_oriented_size(int32_t w, int32_t h, int32_t o, int32_t *ow, int32_t *oh) {
    if (!ow || !oh) return fail("null argument");
    if (o < 0 || o > 8) return fail("orientation " + std::to_string(o) + " is outside 0 .. 8");
    int64_t a, b;
    jp2hip::orient_size(w, h, o, a, b);
    *ow = (int32_t)a;
    *oh = (int32_t)b;
    return 0;
}

int jp2hip_orientation_source_rows(int32_t height, int32_t width, int32_t o, int32_t row0, int32_t row1,
                                   int32_t *src_row0, int32_t *src_row1) {
    if (!src_row0 || !src_row1) return fail("null argument");
    if (o < 0 || o > 8) return fail("orientation " + std::to_string(o) + " is outside 0 .. 8");
    if (height <= 0 || width <= 0) return fail("orientation: bad geometry");
    int64_t s0, s1;
    jp2hip::orient_source_rows(height, width, o, row0, row1, s0, s1);
    *src_row0 = (int32_t)s0;
    *src_row1 = (int32_t)s1;
    return 0;
}

// the letters a context may hold; the message for the ones it may not
static bool letters_ok(int32_t letters, std::string &err) {
    if (letters & 1) {
        err = "tile-part divisions: R (bit 1) is the recipe's: set recipe.tparts_r";
        return false;
    }
    if (letters & ~(JP2HIP_TPARTS_L | JP2HIP_TPARTS_C)) {
        err = "tile-part divisions: " + std::to_string(letters) + " has a bit that is neither JP2HIP_TPARTS_L (2) nor " +
              "JP2HIP_TPARTS_C (4)";
        return false;
    }
    return true;
}

int jp2hip_set_tile_part_divisions(jp2hip_ctx *ctx, int32_t letters) {
    std::string err;
    if (!letters_ok(letters, err)) return fail(err);
    if (!ctx) return fail("null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->tparts = letters;
    for (jp2hip_ctx *p : ctx->peers)
        if (jp2hip_set_tile_part_divisions(p, letters) != 0) return -1;
    return 0;
}

int jp2hip_check_layer_slopes(const double *slopes, int32_t n, const jp2hip_recipe *recipe) {
    std::string err;
    return jp2hip::check_layer_slopes(slopes, n, recipe, err) ? 0 : fail(err);
}

int jp2hip_set_layer_slopes(jp2hip_ctx *ctx, const double *slopes, int32_t n) {
    if (!slopes) n = 0;
    if (jp2hip_check_layer_slopes(slopes, n, nullptr) != 0) return -1;
    if (!ctx) return fail("null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (n && !ctx->rates.empty())
        return fail("layer slopes: per-layer rates are set on this context (jp2hip_set_layer_rates); turn them off first");
    if (n && !ctx->psnr.empty())
        return fail("layer slopes: PSNR targets are set on this context (jp2hip_set_layer_psnr); turn them off first");
    ctx->slopes.assign(slopes, slopes + n);
    for (jp2hip_ctx *p : ctx->peers)
        if (jp2hip_set_layer_slopes(p, slopes, n) != 0) return -1;
    return 0;
}

int jp2hip_check_layer_rates(const double *rates_bpp, int32_t n, const jp2hip_recipe *recipe) {
    std::string err;
    return jp2hip::check_layer_rates(rates_bpp, n, recipe, err) ? 0 : fail(err);
}

int jp2hip_set_layer_rates(jp2hip_ctx *ctx, const double *rates_bpp, int32_t n) {
    if (!rates_bpp) n = 0;
    if (jp2hip_check_layer_rates(rates_bpp, n, nullptr) != 0) return -1;
    if (!ctx) return fail("null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (n && !ctx->slopes.empty())
        return fail("layer rates: fixed-slope layers are set on this context (jp2hip_set_layer_slopes); turn them off first");
    if (n && !ctx->psnr.empty())
        return fail("layer rates: PSNR targets are set on this context (jp2hip_set_layer_psnr); turn them off first");
    ctx->rates.assign(rates_bpp, rates_bpp + n);
    for (jp2hip_ctx *p : ctx->peers)
        if (jp2hip_set_layer_rates(p, rates_bpp, n) != 0) return -1;
    return 0;
}

int jp2hip_check_layer_psnr(const double *psnr_db, int32_t n, const jp2hip_recipe *recipe) {
    std::string err;
    return jp2hip::check_layer_psnr(psnr_db, n, recipe, err) ? 0 : fail(err);
}

int jp2hip_set_layer_psnr(jp2hip_ctx *ctx, const double *psnr_db, int32_t n) {
    if (!psnr_db) n = 0;
    if (jp2hip_check_layer_psnr(psnr_db, n, nullptr) != 0) return -1;
    if (!ctx) return fail("null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (n && !ctx->slopes.empty())
        return fail("layer psnr: fixed-slope layers are set on this context (jp2hip_set_layer_slopes); turn them off first");
    if (n && !ctx->rates.empty())
        return fail("layer psnr: per-layer rates are set on this context (jp2hip_set_layer_rates); turn them off first");
    ctx->psnr.assign(psnr_db, psnr_db + n);
    for (jp2hip_ctx *p : ctx->peers)
        if (jp2hip_set_layer_psnr(p, psnr_db, n) != 0) return -1;
    return 0;
}

int64_t jp2hip_distortion_quantum(double weight, int64_t dd, int32_t bits) {
    if (bits < 1 || bits > 16) return fail("distortion quantum: bits = " + std::to_string(bits) + " is outside 1 .. 16");
    return jp2hip::distortion_quantum(weight, dd, bits);
}

int jp2hip_layer_psnr_targets(int32_t width, int32_t height, int32_t components, int32_t bits, const double *psnr_db,
                              int32_t n, int64_t *targets) {
    if (!targets) return fail("null argument");
    if (width <= 0 || height <= 0 || components < 1 || components > 4 || bits < 1 || bits > 16)
        return fail("layer psnr: bad geometry (1-4 components, 1-16 bits)");
    std::string err;
    if (!jp2hip::check_layer_psnr(psnr_db, n, nullptr, err)) return fail(err);
    jp2hip::layer_psnr_targets(width, height, components, bits, psnr_db, n, targets);
    return 0;
}

int jp2hip_layer_psnr_fits(int32_t width, int32_t height, int32_t components, int32_t bits,
                           const jp2hip_recipe *recipe) {
    if (!recipe) return fail("null argument");
    jp2hip::Plan plan;
    std::string err;
    jp2hip_recipe rc = *recipe;
    if (!jp2hip::resolve_tiles(rc, width, height, err) ||
        !jp2hip::build_plan(plan, rc, width, height, components, bits, err, rc.rate_bpp <= 0.0))
        return fail(err);
    return jp2hip::quanta_fit(plan) ? 1 : 0;
}

int jp2hip_layer_rate_step(int32_t layers, int32_t it, int64_t fixed, int64_t part_bytes, const int64_t *layer_bytes,
                           const int64_t *targets, int64_t *budgets) {
    if (layers < 1 || layers > jp2hip::kMaxLayers || it < 0 || it > 7 || !layer_bytes || !targets || !budgets)
        return fail("layer rate step: layers outside 1 .. 32, it outside 0 .. 7, or a null array");
    return jp2hip::layer_rate_step(layers, it, fixed, part_bytes, layer_bytes, targets, budgets);
}

int jp2hip_layer_rate_targets(int32_t width, int32_t height, int32_t components, int32_t bits,
                              const jp2hip_recipe *recipe, int32_t letters, int32_t tlm, const double *rates_bpp,
                              int32_t n, int64_t *targets, int64_t *budgets, int64_t *info) {
    if (!recipe || !rates_bpp || !targets || !budgets) return fail("null argument");
    jp2hip::Plan plan;
    std::string err;
    jp2hip_recipe rc = *recipe;
    if (!jp2hip::check_layer_rates(rates_bpp, n, &rc, err) || !letters_ok(letters, err) ||
        !jp2hip::resolve_tiles(rc, width, height, err) ||
        !jp2hip::build_plan(plan, rc, width, height, components, bits, err, rc.rate_bpp <= 0.0))
        return fail(err);
    if (n != rc.layers) return fail("layer rates: none given");
    std::vector<int> count;
    if (!jp2hip::tile_part_counts(plan, letters, count, err)) return fail(err);
    int64_t ntp = 0;
    for (int c : count) ntp += c;
    const int64_t T = tlm ? jp2hip::tlm_bytes(ntp) : 0, E = jp2hip::tile_part_division_bytes(plan, letters, ntp);
    jp2hip::layer_rate_targets(plan, rates_bpp, n, T + E, targets, budgets);
    if (info) {
        info[0] = T;
        info[1] = E;
        info[2] = plan.ntileparts;
        info[3] = plan.npackets;
    }
    return 0;
}

double jp2hip_slope_from_log2(double v, int32_t bits) { return std::exp2(v + 2.0 * bits); }
double jp2hip_slope_to_log2(double s, int32_t bits) { return std::log2(s) - 2.0 * bits; }

int jp2hip_set_layer_report(jp2hip_ctx *ctx, int32_t on) {
    if (on != 0 && on != 1) return fail("layer report: on must be 0 or 1, not " + std::to_string(on));
    if (!ctx) return fail("null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->report_on = on;
    for (jp2hip_ctx *p : ctx->peers)
        if (jp2hip_set_layer_report(p, on) != 0) return -1;
    return 0;
}

int jp2hip_layer_report(jp2hip_ctx *ctx, struct jp2hip_layer_report *r) {
    if (!ctx || !r) return fail("null argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->report_set) return fail("layer report: no encode on this context has written a main header yet");
    *r = ctx->report;
    return 0;
}

int64_t jp2hip_tile_parts(int32_t width, int32_t height, int32_t components, int32_t bits,
                          const jp2hip_recipe *recipe, int32_t letters, int32_t tile, uint32_t *first, int64_t cap) {
    if (!recipe || cap < 0 || (cap > 0 && !first)) return fail("null recipe, or no room for the tile-parts");
    // the plan an encode of this image builds and the checks it makes, then
    // the function its tier-2 tables take the tile-parts from
    jp2hip::Plan plan;
    std::string err;
    jp2hip_recipe rc = *recipe;
    if (!letters_ok(letters, err) || !jp2hip::resolve_tiles(rc, width, height, err) ||
        !jp2hip::build_plan(plan, rc, width, height, components, bits, err))
        return fail(err);
    std::vector<int> count;
    if (!jp2hip::tile_part_counts(plan, letters, count, err)) return fail(err);
    if (tile < 0 || tile >= plan.ntx * plan.nty) return fail("tile index outside the image's tiles");
    std::vector<uint32_t> f;
    const int n = jp2hip::tile_part_runs(plan, tile, letters, nullptr, f);
    std::copy(f.begin(), f.begin() + (ptrdiff_t)std::min<int64_t>(cap, (int64_t)f.size()), first);
    return n;
}

int64_t jp2hip_tlm_segments(const uint16_t *tiles, const uint32_t *lengths, int64_t n, uint8_t *dst, size_t cap) {
    if (!tiles || !lengths || n < 0) return fail("null tiles or lengths, or a negative count");
    if (n > jp2hip::kTlmMaxEntries)
        return fail("more tile-parts than 256 TLM marker segments hold (" + std::to_string(jp2hip::kTlmMaxEntries) + ")");
    const int64_t bytes = jp2hip::tlm_bytes(n);
    if (dst && cap >= (size_t)bytes) jp2hip::tlm_segments(tiles, lengths, n, dst);
    return bytes;
}

const char *jp2hip_dma_engines(void) {
    thread_local std::string s;
    s = jp2hip::dma_engine_report();
    return s.c_str();
}

int jp2hip_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes) {
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (hipSetDevice(device) != hipSuccess) return fail("device ordinal " + std::to_string(device) + " not usable");
    size_t fr = 0, tot = 0;
    const hipError_t e = hipMemGetInfo(&fr, &tot);
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) return fail(std::string("hipMemGetInfo: ") + hipGetErrorString(e));
    if (free_bytes) *free_bytes = (int64_t)fr;
    if (total_bytes) *total_bytes = (int64_t)tot;
    return 0;
}

void jp2hip_destroy(jp2hip_ctx *ctx) {
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        g_reg.erase(std::remove(g_reg.begin(), g_reg.end(), ctx), g_reg.end());
    }
    g_live_contexts--;  // its peers count themselves down as they go
    delete ctx;
}

int jp2hip_tiff_layout(const uint8_t *tiff, size_t len, jp2hip_layout *layout, uint64_t *offsets,
                       int32_t max_offsets) {
    if (!layout) return fail("null layout");
    std::vector<uint64_t> offs;
    if (read_tiff(tiff, len, layout, offs)) return -1;
    if ((int32_t)offs.size() > max_offsets || !offsets) {
        layout->strip_offsets = nullptr;
        return fail("offsets array too small: need " + std::to_string(offs.size()));
    }
    std::memcpy(offsets, offs.data(), offs.size() * sizeof(uint64_t));
    layout->strip_offsets = offsets;
    layout->strip_bytes = (layout->compression > 1 || layout->tile_width > 0) ? offsets + layout->nstrips : nullptr;
    return 0;
}

int jp2hip_encoded_format(const jp2hip_layout *layout, int32_t *components, int32_t *bits) {
    if (!layout || !components || !bits) return fail("null argument");
    int nc, b;
    jp2hip::encoded_format(*layout, nc, b);
    *components = nc;
    *bits = b;
    return 0;
}

int64_t jp2hip_file_header(const jp2hip_layout *layout, int32_t format, uint64_t codestream_bytes, uint8_t *dst,
                           size_t cap) {
    if (!layout) return fail("null layout");
    if (format != JP2HIP_FORMAT_J2K && format != JP2HIP_FORMAT_JP2 && format != JP2HIP_FORMAT_JPX)
        return fail("format must be JP2HIP_FORMAT_J2K, _JP2 or _JPX");
    // the two functions the encodes call, on a plan that holds what they read
    jp2hip::Plan hdr;
    std::memset(&hdr.rc, 0, sizeof hdr.rc);
    hdr.rc.format = format;
    hdr.w = layout->width;
    hdr.h = layout->height;
    jp2hip::encoded_format(*layout, hdr.nc, hdr.bits);
    const jp2hip::SourceMeta meta = jp2hip::source_meta(*layout);
    const size_t n = jp2hip::file_header_bytes(hdr, meta);
    if (n && dst && cap >= n) jp2hip::write_file_header(hdr, meta, codestream_bytes, dst);
    return (int64_t)n;
}

int64_t jp2hip_packet_sequence(int32_t width, int32_t height, int32_t components, int32_t bits,
                               const jp2hip_recipe *recipe, int32_t tile, uint32_t *seq, int64_t cap) {
    if (!recipe || cap < 0 || (cap > 0 && !seq)) return fail("null recipe, or no room for the sequence");
    // the plan an encode of this image builds (its refusals included), then
    // the function its tier-2 tables take the order from
    jp2hip::Plan plan;
    std::string err;
    jp2hip_recipe rc = *recipe;
    if (!jp2hip::resolve_tiles(rc, width, height, err) ||
        !jp2hip::build_plan(plan, rc, width, height, components, bits, err))
        return fail(err);
    if (tile < 0 || tile >= plan.ntx * plan.nty) return fail("tile index outside the image's tiles");
    std::vector<uint32_t> s;
    jp2hip::packet_sequence(plan, tile, s);
    std::copy(s.begin(), s.begin() + (ptrdiff_t)std::min<int64_t>(cap, (int64_t)s.size()), seq);
    return (int64_t)s.size();
}

int jp2hip_encode_device(jp2hip_ctx *ctx, const void *d_src, size_t src_len, const jp2hip_layout *layout,
                         int conversion, const jp2hip_recipe *recipe, uint8_t **out, size_t *out_len,
                         jp2hip_stats *stats) {
    if (!ctx || !out || !out_len) return fail("null argument");
    *out = nullptr;
    *out_len = 0;
    double t0 = now_ms();
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->orient == JP2HIP_ORIENT_TIFF) return fail(kOrientNeedsTiff);
    return encode_core(ctx, d_src, src_len, layout, conversion, recipe, out, out_len, stats, t0, 0.0, ctx->orient);
}

int jp2hip_encode_tiff(jp2hip_ctx *ctx, const uint8_t *tiff, size_t len, int conversion,
                       const jp2hip_recipe *recipe, uint8_t **out, size_t *out_len, jp2hip_stats *stats) {
    if (!ctx || !out || !out_len) return fail("null argument");
    *out = nullptr;
    *out_len = 0;
    double t0 = now_ms();
    jp2hip_layout lay;
    std::vector<uint64_t> offs;
    if (read_tiff(tiff, len, &lay, offs)) return -1;
    const int orient = source_orientation(ctx, tiff, len);
    if (wants_split(ctx, lay))
        return encode_split_host(ctx, tiff, len, lay, conversion, recipe, -1, out, out_len, stats, t0, orient);
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::string err;
    double th = now_ms();
    if (!ctx->gpu.upload_source(tiff, len, err)) return fail(err);
    double h2d = now_ms() - th;
    return encode_core(ctx, ctx->gpu.source(), len, &lay, conversion, recipe, out, out_len, stats, t0, h2d, orient);
}

int jp2hip_encode_file(jp2hip_ctx *ctx, const char *tiff_path, const char *out_path, int conversion,
                       const jp2hip_recipe *recipe, jp2hip_stats *stats) {
    if (!ctx || !tiff_path || !out_path) return fail("null argument");
    const double t0 = now_ms();
    MappedFile mf;
    if (!mf.open(tiff_path)) {
        if (mf.fd < 0) return fail(std::string("cannot open TIFF: ") + tiff_path);
        return fail(std::string("cannot read TIFF: ") + tiff_path);
    }
    jp2hip_layout lay;
    std::vector<uint64_t> offs;
    if (read_tiff(mf.p, mf.n, &lay, offs)) return -1;
    const std::string cannot_write = std::string("cannot write output: ") + out_path;
    if (wants_split(ctx, lay)) {
        // every rank writes its part at its offset of the temp file
        TempOutput tmp(out_path);
        const int fd = ::open(tmp.name.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        if (fd < 0) return fail(cannot_write);
        const int rc = encode_split_host(ctx, mf.p, mf.n, lay, conversion, recipe, fd, nullptr, nullptr, stats, t0,
                                         source_orientation(ctx, mf.p, mf.n));
        const bool closed = ::close(fd) == 0;
        if (rc != 0) return -1;
        return closed && tmp.commit() ? 0 : fail(cannot_write);
    }
    uint8_t *out = nullptr;
    size_t olen = 0;
    if (jp2hip_encode_tiff(ctx, mf.p, mf.n, conversion, recipe, &out, &olen, stats)) return -1;
    TempOutput tmp(out_path);
    FILE *o = std::fopen(tmp.name.c_str(), "wb");
    bool ok = o && std::fwrite(out, 1, olen, o) == olen;
    ok = o && (std::fclose(o) == 0) && ok;
    out_free(out);
    if (!ok || !tmp.commit()) return fail(cannot_write);
    if (stats) stats->total_ms = now_ms() - t0;
    return 0;
}

int64_t jp2hip_tiff_pixels(const char *tiff_path) {
    if (!tiff_path) return fail("null argument");
    MappedFile mf;
    if (!mf.open(tiff_path)) return fail(std::string("cannot open TIFF: ") + tiff_path);
    jp2hip_layout lay;
    std::vector<uint64_t> offs;
    if (read_tiff(mf.p, mf.n, &lay, offs)) return -1;
    return (int64_t)lay.width * lay.height;
}

int jp2hip_split_peers(jp2hip_ctx *ctx, const int32_t *ordinals, int32_t n, int64_t min_pixels) {
    if (!ctx || n < 0 || (n > 0 && !ordinals)) return fail("null argument");
    if (n > 64) return fail("split: at most 64 peers");
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::vector<jp2hip_ctx *> made;
    for (int i = 0; i < n; i++) {
        jp2hip_config c = ctx->cfg;
        c.device = ordinals[i];
        jp2hip_ctx *p = nullptr;
        if (jp2hip_create(&p, &c) != 0) {
            const std::string e = std::string("split peer on device ") + std::to_string(ordinals[i]) + ": " + g_err;
            for (jp2hip_ctx *q : made) jp2hip_destroy(q);
            return fail(e);
        }
        p->org = ctx->org;  // (jp2hip_set_organisation: peers added later inherit it)
        p->tparts = ctx->tparts;  // (jp2hip_set_tile_part_divisions likewise)
        p->slopes = ctx->slopes;  // (jp2hip_set_layer_slopes, _rates, _psnr, jp2hip_set_layer_report likewise)
        p->rates = ctx->rates;
        p->psnr = ctx->psnr;
        p->report_on = ctx->report_on;
        p->orient = ctx->orient;  // (jp2hip_set_source_orientation likewise)
        made.push_back(p);
    }
    for (jp2hip_ctx *p : ctx->peers) jp2hip_destroy(p);
    ctx->peers = made;
    ctx->split_min_pixels = std::max<int64_t>(0, min_pixels);
    return 0;
}

int jp2hip_encode_device_split(jp2hip_ctx *ctx, const void *d_src, size_t src_len, const jp2hip_layout *layout,
                               int conversion, const jp2hip_recipe *recipe, const jp2hip_split *split,
                               uint8_t **out, size_t *out_len, uint64_t *file_offset, uint64_t *file_len,
                               jp2hip_stats *stats) {
    if (!ctx || !out || !out_len) return fail("null argument");
    *out = nullptr;
    *out_len = 0;
    double t0 = now_ms();
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->orient == JP2HIP_ORIENT_TIFF) return fail(kOrientNeedsTiff);
    return encode_split_core(ctx, d_src, src_len, layout, conversion, recipe, split, out, out_len, file_offset,
                             file_len, stats, t0, ctx->orient);
}

void jp2hip_free(void *p) { out_free(p); }

}  // extern "C"
