// CPU unit test of the in-process all-reduce of a tile-split encode
// (csrc/host_group.h), built under TSan and under ASan / UBSan.
#include "host_group.h"

#include <atomic>
#include <cstdio>
#include <functional>
#include <thread>

using jp2hip::HostGroup;

static std::atomic<int> failures{0};
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                              \
        }                                                            \
    } while (0)

// `world` threads, each running rank(r)
static void run_ranks(int world, const std::function<void(int)> &rank) {
    std::vector<std::thread> th;
    for (int r = 0; r < world; r++) th.emplace_back(rank, r);
    for (std::thread &t : th) t.join();
}

static int64_t value(int rank, int gen, int i) { return (int64_t)(rank + 1) * 1000003 + (int64_t)gen * 31 + i * 7; }

// 2 000 back-to-back exchanges of changing length: every rank sees every sum
// (res_[g & 1] is reused two generations later)
static void exchanges(int world) {
    static const int kLen[4] = {1, 3, 21, 1025};
    HostGroup g(world);
    run_ranks(world, [&](int rank) {
        std::vector<int64_t> v;
        int bad = 0;
        for (int gen = 0; gen < 2000; gen++) {
            const int n = kLen[gen % 4];
            v.resize((size_t)n);
            for (int i = 0; i < n; i++) v[(size_t)i] = value(rank, gen, i);
            if (g.reduce(v.data(), n) != 0) bad++;
            const int64_t ranks = (int64_t)world * (world + 1) / 2 * 1000003;
            for (int i = 0; i < n; i++) bad += v[(size_t)i] != ranks + (int64_t)world * ((int64_t)gen * 31 + i * 7);
        }
        CHECK(bad == 0);
    });
}

// one rank calls with `odd_n`, the others with 3: every rank gets -1, none hangs
static void out_of_step(int world, int odd_rank, int odd_n) {
    HostGroup g(world);
    run_ranks(world, [&](int rank) {
        int64_t v[5] = {1, 2, 3, 4, 5};
        CHECK(g.reduce(v, rank == odd_rank ? odd_n : 3) == -1);
    });
    int64_t v[3] = {0, 0, 0};
    CHECK(g.reduce(v, 3) == -1);  // and stays aborted
}

int main() {
    for (int world : {1, 2, 4, 7}) exchanges(world);
    for (int odd_rank : {0, 3}) {
        out_of_step(4, odd_rank, 5);
        out_of_step(4, odd_rank, -1);
    }
    {
        // abort() while world - 1 ranks are in an exchange (or about to
        // join it): all of them return -1; a later reduce returns -1 at once
        const int world = 4;
        HostGroup g(world);
        std::atomic<int> joining{0};
        std::thread aborter([&] {
            while (joining.load() < world - 1) std::this_thread::yield();
            g.abort();
        });
        run_ranks(world - 1, [&](int rank) {
            int64_t v[2] = {rank, 1};
            joining++;
            CHECK(g.reduce(v, 2) == -1);
        });
        aborter.join();
        int64_t v[2] = {0, 0};
        CHECK(g.reduce(v, 2) == -1);
    }
    // abort() right after the last exchange, as every rank of a split encode
    // calls it on return: a rank still copying that exchange's result keeps it
    for (int rep = 0; rep < 300; rep++) {
        const int world = 3;
        HostGroup g(world);
        run_ranks(world, [&](int rank) {
            int64_t v[3] = {rank, 10 * rank, 1};
            CHECK(g.reduce(v, 3) == 0);
            g.abort();
            CHECK(v[0] == 3 && v[1] == 30 && v[2] == 3);
        });
    }
    if (failures) return 1;
    std::printf("HOST GROUP OK\n");
    return 0;
}
