// pinned_pool.cpp -- see pinned_pool.h.
#include "pinned_pool.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <vector>

namespace jp2hip {

size_t PinnedPool::cap_locked() const { return std::max(idle_floor_, peak_live_ * max_cap_); }

uint8_t *PinnedPool::alloc(size_t n) {
    n = std::max<size_t>(n, 1);
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = idle_.lower_bound(n);
        if (it != idle_.end() && it->first <= 2 * n + ((size_t)1 << 20)) {
            void *b = it->second;
            live_[b] = it->first;
            peak_live_ = std::max(peak_live_, live_.size());
            idle_bytes_ -= it->first;
            idle_.erase(it);
            return (uint8_t *)b;
        }
    }
    const size_t cap = n + n / 8 + 4096;  // room for a slightly larger file next time
    static const bool log = getenv("JP2HIP_LOG_POOL") != nullptr;  // diagnostics: pool misses
    const auto t0 = std::chrono::steady_clock::now();
    void *b = pin_(cap);
    if (!b) return nullptr;
    std::lock_guard<std::mutex> lk(mu_);
    if (log)
        fprintf(stderr, "jp2hip pool miss: %zu bytes pinned in %.1f ms (idle %zu buffers, %zu bytes)\n", cap,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                idle_.size(), idle_bytes_);
    live_[b] = cap;
    peak_live_ = std::max(peak_live_, live_.size());
    max_cap_ = std::max(max_cap_, cap);
    return (uint8_t *)b;
}

void PinnedPool::free(void *p) {
    if (!p) return;
    std::vector<void *> drop;
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = live_.find(p);
        if (it == live_.end()) {
            std::free(p);
            return;
        }
        const size_t cap = it->second;
        live_.erase(it);
        idle_.emplace(cap, p);
        idle_bytes_ += cap;
        const size_t idle_cap = cap_locked();
        while (idle_bytes_ > idle_cap && !idle_.empty()) {  // largest first
            auto last = std::prev(idle_.end());
            idle_bytes_ -= last->first;
            drop.push_back(last->second);
            idle_.erase(last);
        }
    }
    for (void *b : drop) unpin_(b);  // outside the lock: unpinning takes long
}

size_t PinnedPool::idle_count() {
    std::lock_guard<std::mutex> lk(mu_);
    return idle_.size();
}
size_t PinnedPool::idle_bytes() {
    std::lock_guard<std::mutex> lk(mu_);
    return idle_bytes_;
}
size_t PinnedPool::idle_cap() {
    std::lock_guard<std::mutex> lk(mu_);
    return cap_locked();
}

}  // namespace jp2hip
