// split.cpp -- exact global PCRD thresholds for a tile-split encode
// (one oversized image, contiguous bands of tile rows per
// GPU).  Host-only: no device code, so the exchange is testable on CPU.
//
// Single-image rule (pcrd.hip k_select, oracle/jp2_oracle.c
// select_threshold): walk the hull segments of every code-block in
// decreasing slope-key order and take whole equal-key groups while the
// running byte total fits the layer budget; the threshold K is the last key
// taken.  Equivalently, with S(k) = bytes of segments whose key >= k (monotone
// non-increasing), the included set is {key >= K'} for
//     K' = min { k : S(k) <= budget },
// since no key lies strictly between the last group taken and the next one.
// S(k) is a sum over ranks, so K' is found by bisection over the 64-bit key
// space with one all-reduce(sum) of `layers` int64 per step (64 steps, all
// layers at once).  Every rank sees the same sums, so every rank ends with
// the same K' and the split encode includes exactly the passes the
// single-GPU encode does.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "jp2hip.h"
#include "jp2hip_internal.h"

namespace {

// bytes of this rank's segments with key >= k (keys descending, cum inclusive)
int64_t bytes_at_least(const uint64_t *keys, const int64_t *cum, int64_t n, uint64_t k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] >= k) lo = mid + 1;
        else hi = mid;
    }
    return lo ? cum[lo - 1] : 0;
}

}  // namespace

extern "C" {

void jp2hip_split_rows(int32_t height, int32_t tile_h, int32_t flush_period, int32_t rank, int32_t world,
                       int32_t *row0, int32_t *row1) {
    int tr0 = 0, tr1 = 0;
    if (tile_h == 0) {  // untiled: one tile row, which the tile-split cannot divide; all of it is rank 0's
        const bool valid = height > 0 && world > 0 && rank >= 0 && rank < world;
        if (row0) *row0 = valid && rank ? height : 0;
        if (row1) *row1 = valid ? height : 0;
        return;
    }
    if (tile_h > 0 && height > 0 && world > 0 && rank >= 0 && rank < world)
        jp2hip::split_tile_rows((height + tile_h - 1) / tile_h, tile_h, height, flush_period, rank, world, tr0, tr1);
    if (row0) *row0 = (int32_t)std::min<int64_t>(height, (int64_t)tr0 * tile_h);
    if (row1) *row1 = (int32_t)std::min<int64_t>(height, (int64_t)tr1 * tile_h);
}

int jp2hip_split_thresholds(const uint64_t *keys, const int64_t *cum, int64_t nseg, const int64_t *budgets,
                            int32_t layers, const jp2hip_split *split, uint64_t *K) {
    if (layers <= 0 || layers > 64 || !budgets || !K || (nseg > 0 && (!keys || !cum))) return -1;
    // positive finite doubles: bit patterns order like the values and stay
    // below 0x7FF0000000000000; one past that includes nothing
    const uint64_t kNone = 0x7FF0000000000001ull;
    std::vector<uint64_t> lo((size_t)layers, 0), hi((size_t)layers, kNone);
    std::vector<int64_t> v((size_t)layers);
    for (;;) {
        bool open = false;
        for (int l = 0; l < layers; l++) {
            const uint64_t mid = lo[l] + ((hi[l] - lo[l]) >> 1);
            v[l] = lo[l] < hi[l] ? bytes_at_least(keys, cum, nseg, mid) : 0;
            open = open || lo[l] < hi[l];
        }
        if (!open) break;  // identical on every rank: same sums, same bounds
        if (split && split->world > 1) {
            if (!split->allreduce_sum || split->allreduce_sum(split->user, v.data(), layers) != 0) return -2;
        }
        for (int l = 0; l < layers; l++) {
            if (lo[l] >= hi[l]) continue;
            const uint64_t mid = lo[l] + ((hi[l] - lo[l]) >> 1);
            if (v[l] <= budgets[l]) hi[l] = mid;
            else lo[l] = mid + 1;
        }
    }
    for (int l = 0; l < layers; l++) K[l] = lo[l];
    return 0;
}

// The distortion counterpart (quality layers by target PSNR; pcrd.hip
// k_select<true> has the single-image rule).  The inclusive sums are of
// distortion quanta, and layer l must remove need[l] = total - targets[l] of
// them, the total being the all-reduced sum of every rank's last entry.  With
// S(k) = quanta of the segments whose key >= k (non-increasing),
//     K[l] = max { k : S(k) >= need[l] },
// the tie group at K[l] taken; found by the same bisection, the other way
// round: lo keeps S(lo) >= need, hi keeps S(hi) < need.  A need the total does
// not reach (targets[l] < 0, the lossless top layer) leaves lo at 0: every
// segment.  need <= 0 takes nothing: the threshold is one above the largest
// key of all ranks, which the same bisection finds over segment counts (the
// largest k that one segment still reaches), and 0 when no rank has a segment.
int jp2hip_split_psnr_thresholds(const uint64_t *keys, const int64_t *cum_quanta, int64_t nseg, const int64_t *targets,
                                 int32_t layers, const jp2hip_split *split, uint64_t *K) {
    if (layers <= 0 || layers > 64 || !targets || !K || nseg < 0 || (nseg > 0 && (!keys || !cum_quanta))) return -1;
    const bool shared = split && split->world > 1;
    auto reduce = [&](int64_t *v, int n) {
        return !shared || (split->allreduce_sum && split->allreduce_sum(split->user, v, n) == 0);
    };
    int64_t tot[2] = {nseg ? cum_quanta[nseg - 1] : 0, nseg};  // quanta, segments
    if (!reduce(tot, 2)) return -2;
    const uint64_t kNone = 0x7FF0000000000001ull;  // (as jp2hip_split_thresholds)
    std::vector<uint64_t> lo((size_t)layers, 0), hi((size_t)layers, kNone);
    std::vector<int64_t> need((size_t)layers), v((size_t)layers);
    std::vector<char> nothing((size_t)layers);
    // this rank's segments with key >= k (keys descending)
    auto count_at_least = [&](uint64_t k) {
        return (int64_t)(std::upper_bound(keys, keys + nseg, k, [](uint64_t a, uint64_t b) { return a > b; }) - keys);
    };
    for (int l = 0; l < layers; l++) {
        need[l] = targets[l] < 0 ? tot[0] + 1 : tot[0] - targets[l];
        nothing[l] = need[l] <= 0;
        if (nothing[l]) need[l] = 1;  // (of the counts: one segment)
    }
    for (;;) {
        bool open = false;
        for (int l = 0; l < layers; l++) {
            const bool o = hi[l] - lo[l] > 1;
            const uint64_t mid = lo[l] + ((hi[l] - lo[l]) >> 1);
            v[l] = !o ? 0 : nothing[l] ? count_at_least(mid) : bytes_at_least(keys, cum_quanta, nseg, mid);
            open = open || o;
        }
        if (!open) break;  // identical on every rank: same sums, same bounds
        if (!reduce(v.data(), layers)) return -2;
        for (int l = 0; l < layers; l++) {
            if (hi[l] - lo[l] <= 1) continue;
            const uint64_t mid = lo[l] + ((hi[l] - lo[l]) >> 1);
            if (v[l] >= need[l]) lo[l] = mid;
            else hi[l] = mid;
        }
    }
    for (int l = 0; l < layers; l++) K[l] = nothing[l] ? (tot[1] ? lo[l] + 1 : 0) : lo[l];
    return 0;
}

}  // extern "C"
