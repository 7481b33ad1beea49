// Host build of psnr_quantum.h and of the tile-split's PSNR exchange
// (csrc/split.cpp), compiled by tests/test_layer_psnr_host.py with
// -fsanitize=address,undefined and run on the extremes: the quantum at the
// ends of both arguments' ranges, and the exchange against a brute-force
// selection on random segment lists with ties and empty segments (world = 1;
// tests/test_layer_psnr.py drives several ranks through Python groups), and
// the refused arguments.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "jp2hip.h"
#include "psnr_quantum.h"

using jp2hip::distortion_quantum;

// split.cpp's jp2hip_split_rows calls into plan.cpp, which this program does
// not link: nothing here reaches it
namespace jp2hip {
void split_tile_rows(int, int, int, int, int, int, int &a, int &b) { a = b = 0; }
}  // namespace jp2hip

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                           \
        }                                                         \
    } while (0)

struct Seg {
    uint64_t key;
    int64_t q;
};

// the rule, by brute force over the whole list
static uint64_t brute(const std::vector<Seg> &all, int64_t target) {
    int64_t total = 0;
    uint64_t top = 0;
    for (const Seg &s : all) {
        total += s.q;
        top = std::max(top, s.key);
    }
    const int64_t need = target < 0 ? total + 1 : total - target;
    if (need <= 0) return all.empty() ? 0 : top + 1;
    uint64_t best = 0;
    for (const Seg &s : all) {
        int64_t sum = 0;
        for (const Seg &t : all) sum += t.key >= s.key ? t.q : 0;
        if (sum >= need) best = std::max(best, s.key);
    }
    return best;
}

static void lists(const std::vector<Seg> &segs, std::vector<uint64_t> &keys, std::vector<int64_t> &cum) {
    std::vector<Seg> s = segs;
    std::stable_sort(s.begin(), s.end(), [](const Seg &a, const Seg &b) { return a.key > b.key; });
    keys.clear();
    cum.clear();
    int64_t acc = 0;
    for (const Seg &x : s) {
        keys.push_back(x.key);
        cum.push_back(acc += x.q);
    }
}

int main() {
    // ---- the quantum
    CHECK(jp2hip::quantum_shift(8) == -8 && jp2hip::quantum_shift(16) == 8 && jp2hip::quantum_shift(1) == -22);
    CHECK(distortion_quantum(0.25, 4, 8) == 256);
    CHECK(distortion_quantum(1.0, 127, 16) == 0 && distortion_quantum(1.0, 128, 16) == 1);
    CHECK(distortion_quantum(1.0, 0, 8) == 0 && distortion_quantum(1.0, -5, 8) == 0 && distortion_quantum(-1.0, 5, 8) == 0);
    CHECK(distortion_quantum(std::numeric_limits<double>::quiet_NaN(), 5, 8) == 0);
    CHECK(distortion_quantum(std::numeric_limits<double>::infinity(), 5, 8) == INT64_MAX);
    CHECK(distortion_quantum(1.0, INT64_MAX, 8) == INT64_MAX && distortion_quantum(1.0, INT64_MIN, 8) == 0);
    CHECK(distortion_quantum(1e300, INT64_MAX, 1) == INT64_MAX);
    CHECK(distortion_quantum(std::numeric_limits<double>::min(), 1, 16) == 0);
    CHECK(distortion_quantum(1.0, (int64_t)1 << 62, 16) == (int64_t)1 << 54);
    CHECK(distortion_quantum(0.5, ((int64_t)1 << 53) + 1, 8) == (int64_t)1 << 60);  // (double)dd rounds to even
    // ---- the exchange against brute force
    std::srand(20261021);
    for (int round = 0; round < 300; round++) {
        const int n = std::rand() % 40;
        std::vector<Seg> all((size_t)n);
        for (Seg &s : all) {
            s.key = 0x4000000000000000ull + (uint64_t)(std::rand() % 12) * 0x1000000ull;  // ties
            s.q = std::rand() % 5 == 0 ? 0 : std::rand() % 1000;
        }
        int64_t total = 0;
        for (const Seg &s : all) total += s.q;
        const int64_t targets[6] = {total + 3, total, total > 0 ? total - 1 : 0, total / 2, 0, -1};
        uint64_t want[6], K[6];
        for (int l = 0; l < 6; l++) want[l] = brute(all, targets[l]);
        std::vector<uint64_t> keys;
        std::vector<int64_t> cum;
        lists(all, keys, cum);
        CHECK(jp2hip_split_psnr_thresholds(keys.data(), cum.data(), n, targets, 6, nullptr, K) == 0);
        for (int l = 0; l < 6; l++) CHECK(K[l] == want[l]);
        // no rank has a segment: every threshold is 0
        CHECK(jp2hip_split_psnr_thresholds(nullptr, nullptr, 0, targets, 6, nullptr, K) == 0);
        for (int l = 0; l < 6; l++) CHECK(K[l] == 0);
    }
    uint64_t K1[1];
    const int64_t t1[1] = {0};
    CHECK(jp2hip_split_psnr_thresholds(nullptr, nullptr, 3, t1, 1, nullptr, K1) == -1);
    CHECK(jp2hip_split_psnr_thresholds(nullptr, nullptr, 0, t1, 0, nullptr, K1) == -1);
    CHECK(jp2hip_split_psnr_thresholds(nullptr, nullptr, 0, nullptr, 1, nullptr, K1) == -1);
    jp2hip_split bad{0, 2, nullptr, nullptr};
    CHECK(jp2hip_split_psnr_thresholds(nullptr, nullptr, 0, t1, 1, &bad, K1) == -2);
    if (failures) return 1;
    std::printf("psnr quantum and exchange: ok\n");
    return 0;
}
