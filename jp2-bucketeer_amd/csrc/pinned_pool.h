// pinned_pool.h -- the bookkeeping of the pinned output pool.  Encoded files
// are returned in pinned host memory: the final code-stream D2H lands in the
// caller's buffer directly (no staging copy; a C3 file is ~340 MB) and
// jp2hip_free() hands the buffer back to the pool, so steady state allocates
// and pins nothing.  The pool keeps returned buffers up to the most that
// were ever handed out at once, each counted at the largest size pinned so
// far (at least 4 GiB): with a fixed 4 GiB, twelve contexts of C3 files
// (385 MB buffers) overflowed it whenever most of their files were returned
// at once, and the next encodes pinned fresh buffers -- hipHostMalloc /
// hipHostFree of that size took tens of ms and held up the other contexts'
// launches meanwhile (a 19 ms window with no kernel on the GPU,
// profiles/r06/c3_pinned_pool.txt); a batch queue holds more files than
// contexts (its uploaders' queue), hence the high-water mark rather than the
// context count.  free() of a pointer the pool does not know is std::free().
// No HIP in it: the two allocator calls are given at construction (api.cpp
// passes hipHostMalloc / hipHostFree), and the CPU suite runs the rules under
// ASan / UBSan (tests/host/test_pinned_pool.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <unordered_map>

namespace jp2hip {

class PinnedPool {
  public:
    using PinFn = void *(*)(size_t bytes);  // nullptr on failure
    using UnpinFn = void (*)(void *);
    static constexpr size_t kIdleFloor = (size_t)4 << 30;
    PinnedPool(PinFn pin, UnpinFn unpin, size_t idle_floor = kIdleFloor)
        : pin_(pin), unpin_(unpin), idle_floor_(idle_floor) {}
    // a buffer of at least max(n, 1) bytes; nullptr when pinning failed
    uint8_t *alloc(size_t n);
    void free(void *p);
    size_t idle_count();
    size_t idle_bytes();
    size_t idle_cap();

  private:
    size_t cap_locked() const;
    const PinFn pin_;
    const UnpinFn unpin_;
    const size_t idle_floor_;
    std::mutex mu_;
    std::unordered_map<void *, size_t> live_;  // handed out: capacity
    std::multimap<size_t, void *> idle_;       // returned: capacity -> buffer
    size_t idle_bytes_ = 0;
    size_t max_cap_ = 0;    // the largest buffer pinned so far
    size_t peak_live_ = 0;  // the most buffers handed out at once
};

}  // namespace jp2hip
