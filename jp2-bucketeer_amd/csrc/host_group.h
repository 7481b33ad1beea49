// host_group.h -- the all-reduce of a tile-split inside the library
// (jp2hip_split_peers).  The ranks of one encode are threads of this process,
// one per member context (each with its own GPU and stream); their exchanges
// (split.cpp, encode.cpp encode_split_core) are summed here on the host: a
// few hundred vectors of at most 1 025 int64 per image, nothing that needs
// RCCL.  A rank that fails before an exchange, or returns, aborts the group,
// so no rank waits forever in an exchange another rank will never join.
// No HIP in it: the CPU suite runs it under TSan and ASan / UBSan
// (tests/host/test_host_group.cpp).
#pragma once

#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

namespace jp2hip {

class HostGroup {
  public:
    explicit HostGroup(int world) : world_(world) {}
    int reduce(int64_t *v, int n) {
        std::unique_lock<std::mutex> lk(mu_);
        if (aborted_) return -1;
        if (n < 0) {  // a bug in the caller: fail every rank, not just this one
            aborted_ = true;
            cv_.notify_all();
            return -1;
        }
        if (arrived_ == 0) {
            acc_.assign((size_t)n, 0);
            n_ = n;
        } else if (n != n_) {  // ranks out of step: a bug, never a wrong sum
            aborted_ = true;
            cv_.notify_all();
            return -1;
        }
        for (int i = 0; i < n; i++) acc_[(size_t)i] += v[i];
        const uint64_t g = gen_;
        if (++arrived_ == world_) {
            res_[g & 1].swap(acc_);  // generation g+2 reuses it only after every rank copied it
            arrived_ = 0;
            gen_++;
            cv_.notify_all();
        } else {
            cv_.wait(lk, [&] { return gen_ != g || aborted_; });
            if (gen_ == g) return -1;  // aborted before this exchange completed
        }
        for (int i = 0; i < n; i++) v[i] = res_[g & 1][(size_t)i];
        return 0;
    }
    void abort() {
        std::lock_guard<std::mutex> lk(mu_);
        aborted_ = true;
        cv_.notify_all();
    }
    static int call(void *user, int64_t *v, int32_t n) { return static_cast<HostGroup *>(user)->reduce(v, n); }

  private:
    std::mutex mu_;
    std::condition_variable cv_;
    int world_, arrived_ = 0, n_ = 0;
    uint64_t gen_ = 0;
    bool aborted_ = false;
    std::vector<int64_t> acc_, res_[2];
};

}  // namespace jp2hip
