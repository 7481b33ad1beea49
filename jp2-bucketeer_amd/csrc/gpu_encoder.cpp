// gpu_encoder.cpp -- the part of GpuEncoder that launches no kernel: device
// memory accounting (the buffers themselves are listed in gpu_encoder.h),
// the pinned staging ring of host -> device copies, host waits, debug dumps
// and the stage times read from the events.  The members that enqueue a
// stage live next to its kernels (unpack.hip, expand.hip, front.hip, pcrd.hip,
// t2_device.hip).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "gpu_encoder.h"
#include "hip_check.h"

namespace jp2hip {

// test-only model of a small device: every context's buffers together may
// not pass JP2HIP_TEST_DEVICE_BYTES (0 / unset: the device's own memory)
static std::atomic<long long> g_test_held{0};
static long long test_device_bytes() {
    static const long long v = [] {
        const char *s = getenv("JP2HIP_TEST_DEVICE_BYTES");
        return s ? atoll(s) : 0ll;
    }();
    return v;
}

hipError_t GpuEncoder::device_alloc(void **p, size_t n) {
    const long long cap = test_device_bytes();
    if (cap > 0) {
        if (g_test_held.fetch_add((long long)n) + (long long)n > cap) {
            g_test_held.fetch_sub((long long)n);
            return hipErrorOutOfMemory;
        }
        const hipError_t e = hipMalloc(p, n);
        if (e != hipSuccess) g_test_held.fetch_sub((long long)n);
        return e;
    }
    return hipMalloc(p, n);
}

void GpuEncoder::device_free(DevBuf &b) {
    if (b.ptr) {
        (void)hipFree(b.ptr);
        if (test_device_bytes() > 0) g_test_held.fetch_sub((long long)b.bytes);
    }
    held -= b.bytes;
    b.ptr = nullptr;
    b.bytes = 0;
}

bool GpuEncoder::trim(size_t soft) {
    if (held <= soft) return false;
    for (DevBuf *b : bufs()) device_free(*b);
#ifdef JP2HIP_DEBUG_DUMPS
    if (held != 0) {  // bufs() lists every buffer ensure() can grow, so the sum is back at 0
        fprintf(stderr, "jp2hip: trim: %zu bytes still accounted after every buffer was freed\n", held);
        abort();
    }
#endif
    // the device copies of the plan's tables went with the buffers
    front_gen = 0;
    t2_gen = 0;
    strips_dev = nullptr;
    strips_host.clear();
    dma_ok = false;  // (re-reads t2out's owner agent at the next copy)
    pool_hint = 0;   // (the outsized image's need)
    return true;
}

bool GpuEncoder::pool_grow(std::string &err) {
    unsigned long long used = 0;
    HIPCHECK(hipStreamSynchronize(stream));
    HIPCHECK(hipMemcpy(&used, (unsigned long long *)mqspan.ptr + 2, sizeof used, hipMemcpyDeviceToHost));
    pool_hint = std::max<uint64_t>(pool_hint, used + used / 8);
    pool_grows++;
    return true;
}

void GpuEncoder::quiesce() {
    if (stream) (void)hipStreamSynchronize(stream);
    (void)hipGetLastError();
}

GpuEncoder::~GpuEncoder() {
    for (DevBuf *b : bufs()) device_free(*b);
    if (sync_ev) (void)hipEventDestroy(sync_ev);
    if (stg_ev) (void)hipEventDestroy(stg_ev);
    for (const PinnedChunk &c : stg) (void)hipHostFree(c.p);
    if (stream) (void)hipStreamDestroy(stream);
    for (int i = 0; i < kNumEvents; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (h_sum) (void)hipHostFree(h_sum);
    if (h_tot) (void)hipHostFree(h_tot);
    if (h_rs) (void)hipHostFree(h_rs);
    if (h_dist) (void)hipHostFree(h_dist);
    if (dma_dep.handle) (void)hsa_signal_destroy(dma_dep);
    if (dma_done.handle) (void)hsa_signal_destroy(dma_done);
    if (hsa_up) (void)hsa_shut_down();
}

bool GpuEncoder::init(int dev, std::string &err) {
    device = dev;
    if (const char *f = getenv("JP2HIP_TEST_POOL_FRAC")) pool_frac_test = atof(f);
    HIPCHECK(hipSetDevice(dev));
    HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (int i = 0; i < kNumEvents; i++) HIPCHECK(hipEventCreate(&ev[i]));
    HIPCHECK(hipEventCreateWithFlags(&sync_ev, hipEventBlockingSync | hipEventDisableTiming));
    HIPCHECK(hipEventCreateWithFlags(&stg_ev, hipEventDisableTiming));
    HIPCHECK(hipHostMalloc((void **)&h_tot, 8 * sizeof(int64_t), hipHostMallocDefault));
    return true;
}

bool GpuEncoder::check_residency(std::string &err) {
    hipDevice_t sd = -1;
    HIPCHECK(hipStreamGetDevice(stream, &sd));
    if ((int)sd != device) {
        err = "context on device " + std::to_string(device) + ": its stream is on device " + std::to_string((int)sd);
        return false;
    }
    const DevBuf *bufs[] = {&src, &coef, &bp, &t1out, &stream_buf, &t2out, &blocks};
    for (const DevBuf *b : bufs) {
        if (!b->ptr) continue;
        hipPointerAttribute_t at;
        HIPCHECK(hipPointerGetAttributes(&at, b->ptr));
        if (at.device != device) {
            err = "context on device " + std::to_string(device) + ": a buffer lives on device " +
                  std::to_string(at.device);
            return false;
        }
    }
    return true;
}

bool GpuEncoder::h2d(void *dst, const void *src, size_t bytes, std::string &err) {
    if (!bytes) return true;
    if (hipEventQuery(stg_ev) == hipSuccess) {  // every staged copy has landed: reuse from the start
        if (stg.size() > 1) {
            size_t tot = 0;
            for (const PinnedChunk &c : stg) {
                tot += c.cap;
                HIPCHECK(hipHostFree(c.p));
            }
            stg.clear();
            PinnedChunk c{nullptr, tot};
            HIPCHECK(hipHostMalloc((void **)&c.p, tot, hipHostMallocDefault));
            stg.push_back(c);
        }
        stg_used = 0;
    }
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (stg.empty() || stg_used + need > stg.back().cap) {  // a new chunk; the older ones stay until the copies land
        PinnedChunk c{nullptr, std::max<size_t>(need, stg.empty() ? (size_t)1 << 20 : 2 * stg.back().cap)};
        HIPCHECK(hipHostMalloc((void **)&c.p, c.cap, hipHostMallocDefault));
        stg.push_back(c);
        stg_used = 0;
    }
    uint8_t *h = stg.back().p + stg_used;
    stg_used += need;
    std::memcpy(h, src, bytes);
    HIPCHECK(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipEventRecord(stg_ev, stream));
    return true;
}

// Host waits for this context's stream by sleeping on an event rather than
// spinning: with many images in flight the spinning callers would take the
// cores the tier-2 threads need.
#ifndef JP2HIP_WAIT_POLL_US
#define JP2HIP_WAIT_POLL_US 0  // A/B builds: poll the event every N us instead of sleeping on it
#endif
bool GpuEncoder::host_wait(std::string &err) {
    waits++;
    HIPCHECK(hipEventRecord(sync_ev, stream));
#if JP2HIP_WAIT_POLL_US > 0
    for (;;) {
        const hipError_t q = hipEventQuery(sync_ev);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) HIPCHECK(q);
        std::this_thread::sleep_for(std::chrono::microseconds(JP2HIP_WAIT_POLL_US));
    }
#else
    HIPCHECK(hipEventSynchronize(sync_ev));
#endif
    return true;
}

bool GpuEncoder::upload_source(const void *host, size_t len, std::string &err) {
    HIPCHECK(hipSetDevice(device));
    if (!ensure<uint8_t>(src, len, err)) return false;
    // stream-ordered: the encode that follows (same stream) waits for it, and
    // the caller's buffer outlives the synchronous encode call
    HIPCHECK(hipMemcpyAsync(src.ptr, host, len, hipMemcpyHostToDevice, stream));
    return true;
}

bool GpuEncoder::dump(const char *dir, const char *name, const DevBuf &b, size_t bytes,
                      std::string &err) {
    std::vector<uint8_t> h(bytes);
    if (!host_wait(err)) return false;
    if (bytes) HIPCHECK(hipMemcpy(h.data(), b.ptr, bytes, hipMemcpyDeviceToHost));
    std::string path = std::string(dir) + "/" + name;
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { err = "cannot write dump " + path; return false; }
    fwrite(h.data(), 1, bytes, f);
    fclose(f);
    return true;
}

// Stage times from the events of the last encode (all complete once the
// encode's final host wait returned).
bool GpuEncoder::collect_profile(StageTimes &st, std::string &err) {
    if (!profiled || !h_tot) return true;
    float t;
    HIPCHECK(hipEventElapsedTime(&t, ev[kEvFrontBegin], ev[kEvDwtBegin])); st.ingest = t;
    if (expand_timed) {
        HIPCHECK(hipEventElapsedTime(&t, ev[kEvExpandBegin], ev[kEvExpandEnd]));
        st.ingest += t;
    }
    if (orient_timed) {
        HIPCHECK(hipEventElapsedTime(&t, ev[kEvOrientBegin], ev[kEvOrientEnd]));
        st.ingest += t;
    }
    HIPCHECK(hipEventElapsedTime(&t, ev[kEvDwtBegin], ev[kEvDwtEnd])); st.dwt = t;
    HIPCHECK(hipEventElapsedTime(&t, ev[kEvDwtEnd], ev[kEvQuantEnd])); st.quant = t;
    HIPCHECK(hipEventElapsedTime(&t, ev[kEvCmBegin], ev[kEvCmEnd])); st.t1_cm = t;
    // k_t1_mq from HIP events on the context's stream around its launch, as
    // rocprofv3 times a dispatch (from when the queue reaches it: under load
    // that includes waiting for CUs)
    HIPCHECK(hipEventElapsedTime(&t, ev[kEvCmEnd], ev[kEvMqEnd])); st.t1_mq = t;
    HIPCHECK(hipEventElapsedTime(&t, ev[kEvMqEnd], ev[kEvHullEnd])); st.pcrd += t;
    return true;
}

}  // namespace jp2hip
