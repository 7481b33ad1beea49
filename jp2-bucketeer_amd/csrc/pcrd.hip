// pcrd.hip -- PCRD-opt on the GPU (stage S6 of the map in front.hip): the
// convex hull of every code-block (k_hull, enqueued by run_front), the slope
// thresholds of every layer (k_select, k_select_resolve), the per-block layer
// tables for precincts the wave coder of t2_device.hip does not take
// (k_apply), the hull segment list of the tile-split exchange
// (k_seg_offsets, k_seg_emit), caller-given thresholds for every rate-control
// group (k_fill_keys: the tile-split's agreed keys and fixed-slope layers) and
// the layer report's distortion sums (k_layer_dist, k_layer_dist_sum).  The
// GpuEncoder members that launch them follow the kernels: hull_launch,
// select_launch, select_lossless, select_psnr, select_keys, layer_dist,
// apply_thresholds, rate_loop, segments.  k_hull, k_select and
// k_select_resolve have a second instantiation each for quality layers by
// target PSNR, whose measure is distortion quanta (psnr_quantum.h), not bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "device_common.h"
#include "gpu_encoder.h"
#include "hip_check.h"
#include "psnr_quantum.h"
#include "stage_repeat.h"

namespace jp2hip {

// --------------------------------------------------------------------------
// S6: PCRD-opt.  Hull per block (thread per block, k_hull), which also
// histograms every hull segment's bytes over kPcrdBins slope-key bins; then
// k_select finds each layer's threshold: the bin its budget falls in from the
// histogram, the exact key inside that bin by a radix select over the
// segments of that bin only (no sort of all segments).
// --------------------------------------------------------------------------
struct HullArgs {
    int nblocks;
    const uint8_t *npasses;
    const int32_t *rates;
    const int64_t *dists;
    const double *weight;
    uint8_t *nhull;
    uint8_t *hpass;   // [block][kMaxPasses+1]
    uint64_t *hkey;   // [block][kMaxPasses+1]
    int64_t *hdist;   // [block][kMaxPasses+1] HullPt: the stack's distortion and rate at each point
    unsigned long long *hbytes;  // [group][kPcrdBins] segment bytes per slope bin (zeroed by k_quant)
    uint32_t *hcount;            // [group][kPcrdBins] segments per slope bin
    const int32_t *grp_b0;       // rate-control groups' block ranges (Plan::grp_b0): grid.y = group
    unsigned long long *gtot;    // [group] tier-1 bytes (lossless budgets; zeroed by k_quant)
    // the tier-1 totals of T2Summary (t1_bytes, coded_passes, decisions,
    // skipped; zeroed by k_quant), summed here once per encode instead of by
    // every rate iteration's totals
    const int32_t *lengths;
    const unsigned long long *acc;
    const uint8_t *pmin;
    T2Summary *sum;
    // quality layers by target PSNR (k_hull<true> only): the same histogram of
    // distortion quanta (psnr_quantum.h; zeroed by hull_launch) for `qbits`-bit samples
    unsigned long long *hquanta;  // [group][kPcrdBins]
    int qbits;
};

// slope-key bin: monotone in the key (positive doubles order like their bits)
__device__ __forceinline__ int pcrd_bin(uint64_t key) {
    const int b = (int)(key >> 47) - kPcrdBinBase;
    return b < 0 ? 0 : (b >= kPcrdBins ? kPcrdBins - 1 : b);
}

// hull stack entry beside the output arrays (pass index, slope key): the
// cumulative distortion and the rate at the point, so a pop is one round
// trip (no pass-index -> rate chain)
struct HullPt {
    int64_t d;
    int32_t r, pad;
};
static_assert(sizeof(HullPt) == 16, "HullPt layout");

__device__ __forceinline__ int hull_one(const HullArgs &a, int b, uint32_t *lb, uint32_t *lc) {
    const int np = a.npasses[b];
    const int32_t *R = a.rates + (size_t)b * kMaxPasses;
    const int64_t *Dd = a.dists + (size_t)b * kMaxPasses;
    uint8_t *hp = a.hpass + (size_t)b * (kMaxPasses + 1);
    uint64_t *hk = a.hkey + (size_t)b * (kMaxPasses + 1);
    // the hull stack lives in the output arrays themselves plus hs, so the
    // lane keeps no per-pass arrays (no scratch memory); its top entry (key,
    // cumulative distortion, rate) also lives in registers, so only a pop
    // reads the stack back
    HullPt *hs = (HullPt *)a.hdist + (size_t)b * (kMaxPasses + 1);
    const double wgt = a.weight[b];
    int nh = 1;
    hp[0] = 0;
    hk[0] = 0;
    uint64_t tk = 0;
    int64_t td = 0;
    int32_t tr = 0;
    int64_t Dn = 0;
    // The workgroup's slope-bin histogram follows the stack: a push adds its
    // segment (key, bytes), a pop takes it back out, so what remains is the
    // final hull's segments (no pass over the hull afterwards)
    auto seg = [&](uint64_t key, int32_t bytes, int sign) {
        const int bn = pcrd_bin(key);
        atomicAdd(&lb[bn], (uint32_t)(sign * bytes));
        atomicAdd(&lc[bn], (uint32_t)sign);
    };
    // passes 8 at a time: their rate and distortion loads in flight together
    for (int n0 = 0; n0 < np; n0 += 8) {
        int32_t r8[8];
        int64_t d8[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int i = min(n0 + j, np - 1);
            r8[j] = R[i];
            d8[j] = Dd[i];
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int n = n0 + j + 1;
            if (n > np) break;
            const int32_t Rn = r8[j];
            Dn += d8[j];
            for (;;) {
                const int64_t dD = Dn - td;
                const int32_t dR = Rn - tr;
                bool pop = false;
                double s = 0.0;
                if (dD <= 0) break;
                if (dR <= 0) pop = true;
                else {
                    s = (double)dD * wgt / (double)dR;
                    pop = nh >= 2 && s >= __longlong_as_double((long long)tk);
                }
                if (pop) {
                    nh--;
                    const int32_t rpop = tr;
                    const uint64_t kpop = tk;
                    if (nh <= 1) {
                        tk = 0;
                        td = 0;
                        tr = 0;
                    } else {
                        const HullPt e = hs[nh - 1];
                        tk = hk[nh - 1];
                        td = e.d;
                        tr = e.r;
                    }
                    seg(kpop, rpop - tr, -1);
                    continue;
                }
                seg((uint64_t)__double_as_longlong(s), Rn - tr, 1);
                tk = (uint64_t)__double_as_longlong(s);
                td = Dn;
                tr = Rn;
                hp[nh] = (uint8_t)n;
                hk[nh] = tk;
                hs[nh].d = Dn;
                hs[nh].r = Rn;
                nh++;
                break;
            }
        }
    }
    a.nhull[b] = (uint8_t)nh;
    return nh;
}

// Q: also the histogram of distortion quanta (an encode by PSNR targets).  It
// is built from the finished hull, not on the push / pop path: a quantum is a
// rounded product, which a pop could not take back out the way it takes bytes.
// Each segment's quantum goes to the workgroup's 64-bit LDS bins (32 KB more;
// only this instantiation has them), the bins to memory once per workgroup.
constexpr int kHullThreads = 256;
template <bool Q>
__global__ void __launch_bounds__(kHullThreads) k_hull(HullArgs a) {
    // a workgroup's bytes per bin fit 32 bits (256 blocks of < 100 KB; the
    // pops' transient negatives wrap and cancel): 32 KB of LDS, not 48
    __shared__ uint32_t lb[kPcrdBins];
    __shared__ uint32_t lc[kPcrdBins];
    __shared__ unsigned long long lq[Q ? kPcrdBins : 1];
    for (int i = threadIdx.x; i < kPcrdBins; i += kHullThreads) {
        lb[i] = 0;
        lc[i] = 0;
        if (Q) lq[i] = 0ull;
    }
    __syncthreads();
    const int g = blockIdx.y, gb1 = a.grp_b0[g + 1];
    const int b = a.grp_b0[g] + blockIdx.x * kHullThreads + threadIdx.x;
    if (a.grp_b0[g] + blockIdx.x * kHullThreads >= gb1) return;  // (the whole workgroup)
    int64_t tb = 0, tp = 0, nd = 0;
    bool sk = false;
    if (b < gb1) {
        const int nh = hull_one(a, b, lb, lc);
        if (Q) {
            const uint64_t *hk = a.hkey + (size_t)b * (kMaxPasses + 1);
            const HullPt *hs = (const HullPt *)a.hdist + (size_t)b * (kMaxPasses + 1);
            const double wgt = a.weight[b];
            int64_t prev = 0;
            for (int i = 1; i < nh; i++) {  // (the lane reads back its own stores)
                const int64_t d = hs[i].d;
                const int64_t q = distortion_quantum(wgt, d - prev, a.qbits);
                prev = d;
                if (q) atomicAdd(&lq[pcrd_bin(hk[i])], (unsigned long long)q);
            }
        }
        tb = a.lengths[b];
        tp = a.npasses[b];
        nd = (int64_t)(a.acc[b] & ((1ull << 40) - 1ull));  // decisions (k_t1_cm3)
        sk = a.pmin[b] > 0;
    }
    tb = wave_sum64(tb);
    tp = wave_sum64(tp);
    nd = wave_sum64(nd);
    sk = __any(sk);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&a.gtot[g], (unsigned long long)tb);
        atomicAdd((unsigned long long *)&a.sum->t1_bytes, (unsigned long long)tb);
        atomicAdd((unsigned long long *)&a.sum->coded_passes, (unsigned long long)tp);
        atomicAdd((unsigned long long *)&a.sum->decisions, (unsigned long long)nd);
        if (sk) atomicOr(&a.sum->skipped, 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kPcrdBins; i += kHullThreads)
        if (lc[i]) {
            atomicAdd(&a.hbytes[(size_t)g * kPcrdBins + i], (unsigned long long)lb[i]);
            atomicAdd(&a.hcount[(size_t)g * kPcrdBins + i], lc[i]);
            if (Q && lq[i]) atomicAdd(&a.hquanta[(size_t)g * kPcrdBins + i], lq[i]);
        }
}


// Layer thresholds.  The oracle's rule (oracle/jp2_oracle.c select_threshold)
// is: walk hull segments in decreasing slope-key order, group equal keys, and
// take whole groups while the running byte total fits the budget.  With
// S(k) = bytes of the segments whose key >= k (non-increasing), that takes
// exactly the keys >= K' = min { k : S(k) <= budget } (split.cpp), and K' is
// one above the first key not taken -- the rule's Kc (Kdu-Layer-Info).
//
// Two launches, no sort:
//  1. every workgroup of both: suffix sums of the k_hull bin histogram; per
//     layer the bin b whose segments straddle the budget (S over the bins
//     above b fits, with b's bytes it does not);
//  2. k_select, thread per code-block: the hull segments whose key falls in
//     one of those bins are appended to that bin's candidate list;
//  3. k_select_resolve, a workgroup per layer: the largest key v with (bytes
//     above the bin) + (candidate bytes with key >= v) > budget is the first
//     key not taken, K' = v + 1.
// The list fill counters are zeroed by k_quant and left zero by
// k_select_resolve for the next k_select (the device rate loop runs several).
struct SelectArgs {
    const int *halt;  // device rate loop: nothing to do once it has stopped
    // device rate loop, first iteration: the budgets come from `init` (every
    // workgroup derives them), and k_select's workgroup 0 writes the loop's
    // state and budgets (what a separate init launch did).  init_on = 2, an
    // encode by per-layer rates: the first budgets are `budget`'s (device
    // memory, one per layer), which workgroup 0 copies to budget_w for the step
    int init_on;
    RateState init;
    RateState *rs;
    int64_t *budget_w;
    int nblocks, layers;
    const uint8_t *nhull, *hpass;
    const uint64_t *hkey;
    const int32_t *rates;
    // rate-control groups (grid.y = group): block ranges, first candidate
    // slot (the bound on the hull segments of the groups before), and per
    // group: histogram kPcrdBins apart, budgets / thresholds kMaxLayers
    // apart, list fills kMaxLayers + 1 apart
    const int32_t *grp_b0;
    const uint32_t *grp_seg0;
    const unsigned long long *hbytes;
    const uint32_t *hcount;
    const int64_t *budget;
    // lossless: group g's layer-l budget is gtot[g] * frac[l] >> 16 (the
    // group's tier-1 bytes, k_hull), not budget[]
    int lossless;
    const unsigned long long *gtot;
    int32_t frac[kMaxLayers];
    uint64_t *lkey;   // candidate lists, capacity >= every hull segment
    uint32_t *lsize;
    uint32_t *ctl;    // [group][1 + i] fill of list i ([0] unused)
    uint64_t *K, *Kc;
    int64_t *dbg;     // debug builds: [0] lists, [1 + i] list sizes, [33 + l] rounds, [65 + l] survivors
    // The distortion instantiations (D; an encode by PSNR targets): hbytes is
    // the histogram of quanta, a candidate's size its quantum (64 bits, lsize64)
    // from the hull's cumulative distortions and the block's weight, and layer
    // l may leave qtarget[l] quanta (-1: a lossless top layer, K = 0)
    int64_t qtarget[kMaxLayers];
    uint64_t *lsize64;
    const int64_t *hdist;
    const double *weight;
    int qbits;
};
// lneed of a layer that takes nothing (D): its threshold is one above the largest key
constexpr int64_t kSelNothing = INT64_MIN;

// 256 threads a workgroup (4 waves): under load a 1 024-thread workgroup
// waits for 16 free wave slots on one CU
constexpr int kSelThreads = 256, kSelBrute = 64;
constexpr int kSelPer = kPcrdBins / kSelThreads;  // bins per thread in the scans
// k_select_resolve narrows a layer's key range 1 024 ways per round
constexpr int kResLog2 = 10, kResBins = 1 << kResLog2, kResPer = kResBins / kSelThreads;
// phase 1, run by every workgroup of both kernels (a few microseconds; no
// hand-off through memory): suffix sums of the bin histogram, per layer the
// bin and what it must supply, one candidate list per distinct bin
struct SelBins {
    uint64_t csfx[kSelThreads + 1];     // bytes of the bins >= kSelPer * t (t = 0 .. kSelThreads)
    uint64_t wsum[kSelThreads / 64 + 1];
    int lbin[kMaxLayers], lli[kMaxLayers];
    int64_t lneed[kMaxLayers];          // budget - bytes above the bin
    int list_bin[kMaxLayers];
    uint32_t list_off[kMaxLayers + 1];
    int nlist;
    int wtop[kSelThreads / 64];         // D: each wave's highest bin that holds a segment (-1: none)
};
// The suffix sums are kept per thread chunk (kSelPer bins), 2 KB of LDS
// instead of a 32 KB table per bin (and no 4 KB bin -> list map): a layer's
// bin is found by a binary search over the chunks, then a walk down its
// chunk's bins (re-read from L2).
//
// D (distortion): the measure is quanta and layer l must remove need = total -
// qtarget[l] of them.  With T = need - 1 the search below is the byte select's
// unchanged -- the largest v whose suffix sum exceeds T is the largest whose
// suffix sum reaches need -- but v itself is the threshold (its tie group is
// taken), where the byte select's v is the first key not taken.  need <= 0
// takes nothing: the threshold is the byte select's for a budget of 0, one
// above the largest key of all (kSelNothing; the bin is the highest that holds
// a segment, found from the counts, since a segment may have no quanta).  A
// need the total does not reach (qtarget -1) takes every segment, K = 0.
template <bool D>
__device__ __forceinline__ void select_bins(const SelectArgs &a, SelBins &sh, int g) {
    const int tid = threadIdx.x, L = a.layers;
    const unsigned long long *hbytes = a.hbytes + (size_t)g * kPcrdBins;
    const uint32_t *hcount = a.hcount + (size_t)g * kPcrdBins;
    uint64_t *csfx = sh.csfx;
    int *lbin = sh.lbin, *lli = sh.lli, *list_bin = sh.list_bin;
    int64_t *lneed = sh.lneed;
    uint32_t *list_off = sh.list_off;
    {
        uint64_t s = 0;
#pragma unroll
        for (int i = 0; i < kSelPer; i++) s += hbytes[kSelPer * tid + i];
        uint64_t tot;
        const uint64_t pre = wg_excl_scan64<kSelThreads>(s, sh.wsum, tot);
        csfx[tid] = tot - pre;
        if (tid == 0) csfx[kSelThreads] = 0;
        if (D) {
            int top = -1;
#pragma unroll
            for (int i = 0; i < kSelPer; i++) top = hcount[kSelPer * tid + i] ? kSelPer * tid + i : top;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
            if ((tid & 63) == 0) sh.wtop[tid >> 6] = top;
        }
    }
    __syncthreads();
    if (tid < L) {
        int64_t T;
        bool nothing = false;
        if (D) {
            const int64_t total = (int64_t)csfx[0], tgt = a.qtarget[tid];
            const int64_t need = tgt < 0 ? total + 1 : total - tgt;
            nothing = need <= 0;
            T = need - 1;
        } else {
            // (a negative budget takes nothing, as 0 does: every segment has bytes)
            const int64_t B = a.init_on == 1 ? (a.init.budget < 0 ? 0 : a.init.budget) >> (L - 1 - tid)
                              : a.lossless ? (int64_t)((a.gtot[g] * (unsigned long long)a.frac[tid]) >> 16)
                                           : a.budget[(size_t)g * kMaxLayers + tid];
            T = B < 0 ? 0 : B;
        }
        int b = -1;
        int64_t above = 0;  // S(b + 1)
        if (D && nothing) {
#pragma unroll
            for (int w = 0; w < kSelThreads / 64; w++) b = max(b, sh.wtop[w]);
        } else if ((int64_t)csfx[0] > T) {
            // the largest chunk whose suffix sum exceeds T ...
            int lo = 0, hi = kSelThreads - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((int64_t)csfx[mid] > T) lo = mid;
                else hi = mid - 1;
            }
            // ... then its largest bin b with S(b) > T
            uint64_t S = csfx[lo + 1];
            for (int i = kSelPer - 1; i >= 0; i--) {
                const uint64_t Sb = S + hbytes[kSelPer * lo + i];
                if ((int64_t)Sb > T) {
                    b = kSelPer * lo + i;
                    break;
                }
                S = Sb;
            }
            above = (int64_t)S;
        }
        lbin[tid] = b;
        lneed[tid] = b < 0 ? 0 : (D && nothing) ? kSelNothing : T - above;
    }
    __syncthreads();
    if (tid == 0) {  // one candidate list per distinct bin
        int n = 0;
        uint32_t o = 0;
        for (int l = 0; l < L; l++) {
            if (lbin[l] < 0) continue;
            int i = 0;
            while (i < n && list_bin[i] != lbin[l]) i++;
            if (i == n) {
                list_bin[n] = lbin[l];
                list_off[n] = o;
                o += hcount[lbin[l]];
                n++;
            }
            lli[l] = i;
        }
        list_off[n] = o;
        sh.nlist = n;
    }
    __syncthreads();
}

template <bool D>
__global__ void __launch_bounds__(kSelThreads) k_select(SelectArgs a) {
    __shared__ SelBins sh;
    const int tid = threadIdx.x, lane = tid & 63, g = blockIdx.y;
    if (!a.init_on && a.halt && *a.halt) return;
    const int gb0 = a.grp_b0[g], gb1 = a.grp_b0[g + 1];
    if (a.init_on && blockIdx.x == 0 && g == 0 && tid == 0) {  // the rate loop's state (rate_step continues it)
        RateState r = a.init;
        r.it = 0;
        r.halt = 0;
        r.safety = 0;
        r.iters = 0;
        r.cs_bytes = 0;
        if (r.budget < 0) r.budget = 0;
        *a.rs = r;
        if (a.init_on == 1) rate_budgets(r, a.layers, a.budget_w);
        else
            for (int l = 0; l < a.layers; l++) a.budget_w[l] = a.budget[l];
    }
    if (gb0 + (int)blockIdx.x * kSelThreads >= gb1) return;  // (the whole workgroup)
    select_bins<D>(a, sh, g);
    const uint32_t *list_off = sh.list_off;
    const int *list_bin = sh.list_bin;
    const int nlist = sh.nlist;
    const uint32_t seg0 = a.grp_seg0[g];
    uint32_t *ctl = a.ctl + (size_t)g * (kMaxLayers + 1);
    // 2. candidates of those bins, thread per code-block of the group
    if (nlist > 0)
        for (int b = gb0 + blockIdx.x * kSelThreads + tid; b < gb1; b += gridDim.x * kSelThreads) {
            const int nh = a.nhull[b];
            const uint8_t *hp = a.hpass + (size_t)b * (kMaxPasses + 1);
            const uint64_t *hk = a.hkey + (size_t)b * (kMaxPasses + 1);
            const int32_t *R = a.rates + (size_t)b * kMaxPasses;
            for (int i0 = 1; i0 < nh; i0 += 8) {  // 8 keys' loads in flight together
                uint64_t k8[8];
#pragma unroll
                for (int j = 0; j < 8; j++) k8[j] = hk[min(i0 + j, nh - 1)];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int i = i0 + j;
                    const uint64_t key = k8[j];
                    int li = -1;
                    if (i < nh) {
                        const int bn = pcrd_bin(key);
                        for (int q = 0; q < nlist; q++) li = list_bin[q] == bn ? q : li;
                    }
                    // one fill atomic per wave and list (a list's lanes take
                    // consecutive slots): same-word atomics serialise in L2
                    uint64_t todo = __ballot(li >= 0);
                    while (todo) {
                        const int lead = __builtin_ctzll(todo);
                        const int lj = __shfl(li, lead, 64);
                        const uint64_t grp = __ballot(li == lj);
                        uint32_t base = 0;
                        if (lane == lead) base = atomicAdd(&ctl[1 + lj], (uint32_t)__popcll(grp));
                        base = (uint32_t)__shfl((int)base, lead, 64);
                        if (li == lj) {
                            const uint32_t at =
                                seg0 + list_off[lj] + base + (uint32_t)__popcll(grp & ((1ull << lane) - 1ull));
                            a.lkey[at] = key;
                            if (D) {
                                const HullPt *hs = (const HullPt *)a.hdist + (size_t)b * (kMaxPasses + 1);
                                a.lsize64[at] = (uint64_t)distortion_quantum(
                                    a.weight[b], hs[i].d - (i > 1 ? hs[i - 1].d : 0), a.qbits);
                            } else {
                                a.lsize[at] = (uint32_t)(R[hp[i] - 1] - (hp[i - 1] ? R[hp[i - 1] - 1] : 0));
                            }
                        }
                        todo &= ~grp;
                    }
                }
            }
        }
}

// 3. each layer in a workgroup of its own (grid = layers): the largest
// candidate key v with (bytes above the bin) + (candidate bytes with key >= v)
// > budget is the first key not taken, K' = v + 1.  Workgroup 0 also zeroes
// the list fill counters for the next k_select (the device rate loop runs
// several).  (Folded into k_select -- its group's last workgroup to finish
// resolving the layers, after a device-scope release/acquire count -- the
// pair took 104.5 us alone instead of 53 + 23 with the layers in turn, and
// 116.9 with a wave per layer, 4x longer candidate walks per wave; the C2
// bench did not move: profiles/r05/ab_select_fold.txt.)
// D: the sizes are quanta (64 bits), the threshold is v itself, and a layer
// that takes nothing (kSelNothing) gets one above its list's largest key.
template <bool D>
__global__ void __launch_bounds__(kSelThreads) k_select_resolve(SelectArgs a) {
    using SizeT = typename std::conditional<D, uint64_t, uint32_t>::type;
    const SizeT *lsize = D ? (const SizeT *)a.lsize64 : (const SizeT *)a.lsize;
    __shared__ SelBins sh;
    // the narrowing state and the survivors
    __shared__ uint64_t rlo, rhi, rmax;
    __shared__ int64_t rneed;
    __shared__ uint32_t rcount;
    __shared__ uint64_t bkey[kSelBrute];
    __shared__ SizeT bsize[kSelBrute];
    __shared__ uint64_t hist[kResBins];
    __shared__ uint32_t hcnt[kResBins];
    const int tid = threadIdx.x, lane = tid & 63, l = blockIdx.x, g = blockIdx.y;
    if (a.halt && *a.halt) return;  // (k_select has reset it on a first iteration)
    select_bins<D>(a, sh, g);
    uint64_t *wsum = sh.wsum;
    const int *lbin = sh.lbin, *lli = sh.lli;
    const int64_t *lneed = sh.lneed;
    const uint32_t *list_off = sh.list_off;
    const int nlist = sh.nlist;
    const uint32_t seg0 = a.grp_seg0[g];
    uint64_t *Kg = a.K + (size_t)g * kMaxLayers, *Kcg = a.Kc + (size_t)g * kMaxLayers;
    if (l == 0 && tid <= nlist) a.ctl[(size_t)g * (kMaxLayers + 1) + tid] = 0u;  // (k_select has finished: stream order)
    if (a.dbg && l == 0 && g == 0 && tid == 0) {
        a.dbg[0] = nlist;
        for (int i = 0; i < nlist; i++) a.dbg[1 + i] = list_off[i + 1] - list_off[i];
    }
    // The key range is narrowed by
    // 1 024-way histograms (bytes and counts) over the candidates in range --
    // a bin is 2^47 keys wide, one round leaves a handful (a round starts
    // from the bin's own bounds and count: no pass for them) -- until at most
    // kSelBrute remain, whose totals are then summed directly.
    {
        if (lbin[l] < 0) {
            if (tid == 0) Kg[l] = Kcg[l] = 0ull;  // every segment fits
            return;
        }
        const int li = lli[l];
        const uint32_t i0 = seg0 + list_off[li], i1 = seg0 + list_off[li + 1];
        const int bn = lbin[l];
        if (tid == 0) {
            rcount = i1 - i0;
            rneed = lneed[l];
            if (bn > 0 && bn < kPcrdBins - 1 && !(D && lneed[l] == kSelNothing)) {
                rlo = (uint64_t)(bn + kPcrdBinBase) << 47;
                rhi = rlo + ((1ull << 47) - 1ull);
            } else {  // a clamped end bin: the candidates' own key range
                rlo = ~0ull;
                rhi = 0ull;
            }
        }
        __syncthreads();
        if (rlo > rhi) {
            uint64_t mn = ~0ull, mx = 0ull;
            for (uint32_t i = i0 + tid; i < i1; i += kSelThreads) {
                const uint64_t k = a.lkey[i];
                mn = min(mn, k);
                mx = max(mx, k);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                mn = min(mn, (uint64_t)__shfl_xor((long long)mn, o, 64));
                mx = max(mx, (uint64_t)__shfl_xor((long long)mx, o, 64));
            }
            if (lane == 0) {
                atomicMin((unsigned long long *)&rlo, (unsigned long long)mn);
                atomicMax((unsigned long long *)&rhi, (unsigned long long)mx);
            }
            __syncthreads();
        }
        if (D && lneed[l] == kSelNothing) {  // (rhi: the largest key of the highest bin that holds a segment)
            if (tid == 0) Kg[l] = Kcg[l] = rhi + 1;
            return;
        }
        for (int round = 0;; round++) {
            const uint64_t flo = rlo, fhi = rhi;
            const uint32_t cnt = rcount;
            const int64_t need = rneed;
            if (flo == fhi || cnt <= (uint32_t)kSelBrute) {
                // survivors: v = the largest key whose total exceeds need
                __syncthreads();
                if (tid == 0) {
                    rcount = 0;
                    rmax = flo;  // (one key value left: it is v)
                }
                __syncthreads();
                if (flo != fhi) {
                    if (tid == 0) rmax = 0ull;
                    for (uint32_t i = i0 + tid; i < i1; i += kSelThreads) {
                        const uint64_t k = a.lkey[i];
                        if (k >= flo && k <= fhi) {
                            const uint32_t at = atomicAdd(&rcount, 1u);
                            bkey[at] = k;  // (cnt <= kSelBrute candidates lie in range)
                            bsize[at] = lsize[i];
                        }
                    }
                    __syncthreads();
                    const uint32_t c = rcount;
                    if (tid < (int)c) {
                        const uint64_t k = bkey[tid];
                        int64_t g = 0;
                        for (uint32_t j = 0; j < c; j++) g += bkey[j] >= k ? (int64_t)bsize[j] : 0;
                        if (g > need) atomicMax((unsigned long long *)&rmax, (unsigned long long)k);
                    }
                }
                __syncthreads();
                if (tid == 0) {
                    Kg[l] = Kcg[l] = D ? rmax : rmax + 1;
                    if (a.dbg && g == 0) {
                        a.dbg[33 + l] = round;
                        a.dbg[65 + l] = cnt;
                    }
                }
                break;
            }
            // bytes and counts per 1/4096 of the key range; the sub-range the
            // budget falls in
            const int shift = max(0, 64 - __builtin_clzll(fhi - flo) - kResLog2);
            for (int i = tid; i < kResBins; i += kSelThreads) {
                hist[i] = 0ull;
                hcnt[i] = 0u;
            }
            __syncthreads();
            for (uint32_t i = i0 + tid; i < i1; i += kSelThreads) {
                const uint64_t k = a.lkey[i];
                if (k >= flo && k <= fhi) {
                    const uint32_t sb = (uint32_t)((k - flo) >> shift);
                    atomicAdd((unsigned long long *)&hist[sb], (unsigned long long)lsize[i]);
                    atomicAdd(&hcnt[sb], 1u);
                }
            }
            __syncthreads();
            {
                uint64_t v[kResPer], sm = 0;
#pragma unroll
                for (int i = 0; i < kResPer; i++) sm += (v[i] = hist[kResPer * tid + i]);
                uint64_t tot;
                const uint64_t pre = wg_excl_scan64<kSelThreads>(sm, wsum, tot);
                uint64_t S = tot - pre;  // bytes of the sub-ranges >= kResPer tid
#pragma unroll
                for (int i = 0; i < kResPer; i++) {
                    // the largest sub-range s with S(s) > need: S(s) > need >= S(s + 1)
                    const uint64_t Sn = S - v[i];
                    if ((int64_t)S > need && (int64_t)Sn <= need) {
                        const uint64_t lo = flo + ((uint64_t)(kResPer * tid + i) << shift);
                        rlo = lo;
                        rhi = lo + ((1ull << shift) - 1ull) > fhi ? fhi : lo + ((1ull << shift) - 1ull);
                        rneed = need - (int64_t)Sn;
                        rcount = hcnt[kResPer * tid + i];
                    }
                    S = Sn;
                }
            }
            __syncthreads();
        }
    }
}

// Split path only (GpuEncoder::segments): every hull segment listed
// (key, bytes), for the host-side exact exchange.  Segment counts (hull
// points - 1) and their exclusive scan, one workgroup; rounds of 32
// consecutive blocks per thread, their 32 byte loads in flight together
constexpr int kSegThreads = 1024, kSegPer = 32;
__global__ void __launch_bounds__(kSegThreads) k_seg_offsets(int nblocks, const uint8_t *nhull, int32_t *nseg,
                                                             int32_t *segoff) {
    __shared__ uint32_t wsum[kSegThreads / 64 + 1];
    uint32_t base = 0;
    for (int r0 = 0; r0 < nblocks; r0 += kSegThreads * kSegPer) {
        const int b0 = r0 + (int)threadIdx.x * kSegPer;
        uint8_t n[kSegPer];
        uint32_t c = 0, tot;
        const bool whole = b0 + kSegPer <= nblocks;  // 16-byte loads / stores (b0 is 32-aligned)
        if (whole) {
            const uint4 v0 = *(const uint4 *)(nhull + b0), v1 = *(const uint4 *)(nhull + b0 + 16);
            const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int i = 0; i < kSegPer; i++) n[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
        } else {
#pragma unroll
            for (int i = 0; i < kSegPer; i++) n[i] = nhull[min(b0 + i, nblocks - 1)];
#pragma unroll
            for (int i = 0; i < kSegPer; i++)
                if (b0 + i >= nblocks) n[i] = 0;
        }
        int32_t k[kSegPer], off[kSegPer];
#pragma unroll
        for (int i = 0; i < kSegPer; i++) {
            k[i] = n[i] ? n[i] - 1 : 0;
            c += (uint32_t)k[i];
        }
        uint32_t o = base + wg_excl_scan<kSegThreads>(c, wsum, tot);
#pragma unroll
        for (int i = 0; i < kSegPer; i++) {
            off[i] = (int32_t)o;
            o += (uint32_t)k[i];
        }
        if (whole) {
#pragma unroll
            for (int i = 0; i < kSegPer; i += 4) {
                *(int4 *)(nseg + b0 + i) = make_int4(k[i], k[i + 1], k[i + 2], k[i + 3]);
                *(int4 *)(segoff + b0 + i) = make_int4(off[i], off[i + 1], off[i + 2], off[i + 3]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kSegPer; i++)
                if (b0 + i < nblocks) {
                    nseg[b0 + i] = k[i];
                    segoff[b0 + i] = off[i];
                }
        }
        base += tot;
    }
}

// segments of each block's hull at its offset; entries past the real count
// (up to the bound `nbound`) get key 0 and size 0
__global__ void __launch_bounds__(256) k_seg_emit(int nblocks, const uint8_t *nhull, const uint8_t *hpass,
                                                  const uint64_t *hkey, const int32_t *rates,
                                                  const int32_t *segoff, uint64_t *keys, int64_t *vals,
                                                  const int64_t *hdist, const double *weight, int qbits) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    int nh = nhull[b];
    const uint8_t *hp = hpass + (size_t)b * (kMaxPasses + 1);
    const uint64_t *hk = hkey + (size_t)b * (kMaxPasses + 1);
    const int32_t *R = rates + (size_t)b * kMaxPasses;
    int o = segoff[b];
    for (int i = 1; i < nh; i++) {
        keys[o + i - 1] = hk[i];
        if (qbits) {  // by PSNR targets: the segment's quantum, not its bytes
            const HullPt *hs = (const HullPt *)hdist + (size_t)b * (kMaxPasses + 1);
            vals[o + i - 1] = distortion_quantum(weight[b], hs[i].d - (i > 1 ? hs[i - 1].d : 0), qbits);
        } else {
            vals[o + i - 1] = (int64_t)(R[hp[i] - 1] - (hp[i - 1] ? R[hp[i - 1] - 1] : 0));
        }
    }
}

// last hull index whose key >= K (0 = nothing); hull keys strictly decrease
__device__ __forceinline__ int hull_pick(const uint64_t *hk, int nh, uint64_t K) {
    int lo = 1, hi = nh;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (hk[mid] >= K) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

struct ApplyArgs {
    const int *halt;  // device rate loop: nothing to do once it has stopped
    int nblocks, layers, lossless;
    int ngroups;
    const int32_t *grp_b0;  // the block's rate-control group: its thresholds at K + group * kMaxLayers
    const uint8_t *nhull, *hpass, *npasses;
    const uint64_t *hkey, *K;
    const int32_t *rates;
    uint8_t *nl;      // [block][layers]
    int32_t *lrate;   // [block][layers]
};

__global__ void __launch_bounds__(256) k_apply(ApplyArgs a) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nblocks || (a.halt && *a.halt)) return;
    const int L = a.layers;
    const uint8_t *hp = a.hpass + (size_t)b * (kMaxPasses + 1);
    const uint64_t *hk = a.hkey + (size_t)b * (kMaxPasses + 1);
    const int32_t *R = a.rates + (size_t)b * kMaxPasses;
    int nh = a.nhull[b];
    const uint64_t *K = a.K + (size_t)block_group(a.grp_b0, a.ngroups, b) * kMaxLayers;
    for (int l = 0; l < L; l++) {
        int n = (a.lossless && l == L - 1) ? (int)a.npasses[b] : (int)hp[hull_pick(hk, nh, K[l])];
        a.nl[(size_t)b * L + l] = (uint8_t)n;
        a.lrate[(size_t)b * L + l] = n ? R[n - 1] : 0;
    }
}

// Caller-given thresholds (select_keys): the same L keys for every
// rate-control group, into the K half and the Kc half of `thr`.  The keys
// travel as the kernel's argument: no copy is queued.
struct KeyArgs {
    int ngroups, layers;
    uint64_t key[kMaxLayers];
    uint64_t *thr;  // [2][group][kMaxLayers]
};
__global__ void __launch_bounds__(64) k_fill_keys(KeyArgs a) {
    const int l = threadIdx.x, n = 2 * a.ngroups;
    if (l >= kMaxLayers) return;
    for (int g = blockIdx.x; g < n; g += gridDim.x) a.thr[(size_t)g * kMaxLayers + l] = l < a.layers ? a.key[l] : 0ull;
}

// The layer report's distortion (jp2hip_layer_report): per layer the squared
// error the layer leaves, summed over the code-blocks -- the block's weight
// times the distortion decrease of the passes the layer does not hold, total
// less what the hull's stack recorded at the layer's point (HullPt::d).
// Thread per block; per layer the wave's 64 values are added by a butterfly,
// the workgroup's waves in wave order, and the workgroup's sum is stored at
// part[workgroup][layer]; k_layer_dist_sum adds those in workgroup order.  No
// floating-point atomics: the same launch gives the same bits.
struct DistArgs {
    int nblocks, layers, lossless, ngroups, nparts;
    const int32_t *grp_b0;
    const uint8_t *nhull, *npasses;
    const uint64_t *hkey, *K;
    const int64_t *dists, *hdist;
    const double *weight;
    double *part;  // [nparts][kMaxLayers]
    double *out;   // [kMaxLayers]
};
constexpr int kDistThreads = 256;
__global__ void __launch_bounds__(kDistThreads) k_layer_dist(DistArgs a) {
    __shared__ double ws[kDistThreads / 64][kMaxLayers];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x * kDistThreads + tid, L = a.layers;
    const bool live = b < a.nblocks;
    const int bb = live ? b : 0;  // (idle lanes read block 0 and contribute 0)
    const int np = live ? a.npasses[bb] : 0, nh = live ? a.nhull[bb] : 1;
    const uint64_t *hk = a.hkey + (size_t)bb * (kMaxPasses + 1);
    const HullPt *hs = (const HullPt *)a.hdist + (size_t)bb * (kMaxPasses + 1);
    const int64_t *Dd = a.dists + (size_t)bb * kMaxPasses;
    const uint64_t *K = a.K + (size_t)(live ? block_group(a.grp_b0, a.ngroups, bb) : 0) * kMaxLayers;
    const double wgt = live ? a.weight[bb] : 0.0;
    int64_t total = 0;
    for (int i = 0; i < np; i++) total += Dd[i];
    for (int l = 0; l < L; l++) {
        int64_t through = 0;
        if (a.lossless && l == L - 1) {
            through = total;
        } else if (live) {
            const int at = hull_pick(hk, nh, K[l]);
            through = at ? hs[at].d : 0;
        }
        double v = wgt * (double)(total - through);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) ws[wv][l] = v;
    }
    __syncthreads();
    if (tid < L) {
        double s = ws[0][tid];
        for (int w = 1; w < kDistThreads / 64; w++) s += ws[w][tid];
        a.part[(size_t)blockIdx.x * kMaxLayers + tid] = s;
    }
}
__global__ void __launch_bounds__(64) k_layer_dist_sum(DistArgs a) {
    const int l = threadIdx.x;
    if (l >= kMaxLayers) return;
    double s = 0.0;
    if (l < a.layers)
        for (int p = 0; p < a.nparts; p++) s += a.part[(size_t)p * kMaxLayers + l];
    a.out[l] = s;
}

// --------------------------------------------------------------------------
// The GpuEncoder members that launch the kernels above
// --------------------------------------------------------------------------
// the largest rate-control group (its blocks set the grid's x extent)
static int grp_max_blocks(const Plan &plan) {
    int m = 0;
    for (int g = 0; g < plan.ngroups(); g++) m = std::max(m, plan.grp_b0[(size_t)g + 1] - plan.grp_b0[(size_t)g]);
    return std::max(m, 1);
}

// S6a hulls + their slope-bin histogram (k_select resolves thresholds); then
// reserves the candidate lists of the selection that follows
bool GpuEncoder::hull_launch(const Plan &plan, std::string &err) {
    const int nb = (int)plan.blocks.size(), G = plan.ngroups();
    HullArgs ha;
    ha.nblocks = nb;
    ha.npasses = (const uint8_t *)npasses.ptr;
    ha.rates = (const int32_t *)rates.ptr;
    ha.dists = (const int64_t *)dists.ptr;
    ha.weight = (const double *)weight.ptr;
    ha.nhull = (uint8_t *)nhull.ptr;
    ha.hpass = (uint8_t *)hpass.ptr;
    ha.hkey = (uint64_t *)hkey.ptr;
    ha.hdist = (int64_t *)hdist.ptr;
    ha.hbytes = (unsigned long long *)pcrd_hb.ptr;
    ha.hcount = (uint32_t *)pcrd_hc.ptr;
    ha.lengths = (const int32_t *)lengths.ptr;
    ha.acc = (const unsigned long long *)ordkey.ptr;
    ha.pmin = (const uint8_t *)pmin.ptr;
    ha.sum = (T2Summary *)t2sum.ptr;
    ha.grp_b0 = (const int32_t *)grptab.ptr;
    ha.gtot = (unsigned long long *)gtot.ptr;
    ha.hquanta = nullptr;
    ha.qbits = psnr_bits;
    const dim3 grid((grp_max_blocks(plan) + kHullThreads - 1) / kHullThreads, G);
    if (psnr_bits) {
        // an encode by PSNR targets: the histogram of quanta beside the bytes'
        // (a buffer no other encode allocates), zeroed here in stream order
        if (!ensure<unsigned long long>(pcrd_hq, (size_t)std::max(G, 1) * kPcrdBins, err)) return false;
        HIPCHECK(hipMemsetAsync(pcrd_hq.ptr, 0, (size_t)std::max(G, 1) * kPcrdBins * sizeof(unsigned long long), stream));
        ha.hquanta = (unsigned long long *)pcrd_hq.ptr;
        // (no REPEAT_IF: the stage-repeat builds time the benchmark's path,
        // and a repeat would add every quantum again -- the histogram is
        // zeroed above, not by k_quant as the bytes' is.  A tile-split rank
        // builds the histogram too although only segments() reads quanta on
        // that route: one launch argument serves both routes)
        if (nb) hipLaunchKernelGGL(k_hull<true>, grid, dim3(kHullThreads), 0, stream, ha);
    } else {
        REPEAT_IF(4) if (nb) hipLaunchKernelGGL(k_hull<false>, grid, dim3(kHullThreads), 0, stream, ha);
    }
    HIPCHECK(hipGetLastError());
    // candidate lists: room for every hull segment (the bound sum(3 Mb - 2))
    int64_t nseg_bound = 0;
    for (int i = 0; i < nb; i++) nseg_bound += std::max(0, 3 * (int)plan.blocks[i].Mb - 2);
    nseg = (int)nseg_bound;
    // (by PSNR targets a candidate's size is its quantum: 64 bits)
    return ensure<uint64_t>(sel_key, std::max(nseg, 1), err) &&
           (psnr_bits ? ensure<uint64_t>(sel_size, std::max(nseg, 1), err)
                      : ensure<uint32_t>(sel_size, std::max(nseg, 1), err)) &&
           ensure<uint64_t>(thr, 2 * (size_t)G * kMaxLayers, err);
}

// k_select per rate-control group: lossless budgets from each group's tier-1
// bytes, else from `budget` (the device rate loop's) -- thresholds of group g
// -> thr[g * kMaxLayers ..), Kc -> thr[(G + g) * kMaxLayers ..)
void GpuEncoder::select_launch(const Plan &plan, const int *halt, const RateState *init, RateState *rs,
                               bool by_rates, const int64_t *qtarget) {
    const int nb = (int)plan.blocks.size(), G = plan.ngroups();
    if (!nb) return;
    SelectArgs sa;
    std::memset(&sa, 0, sizeof sa);
    sa.halt = halt;
    sa.nblocks = nb;
    sa.layers = plan.rc.layers;
    sa.nhull = (const uint8_t *)nhull.ptr;
    sa.hpass = (const uint8_t *)hpass.ptr;
    sa.hkey = (const uint64_t *)hkey.ptr;
    sa.rates = (const int32_t *)rates.ptr;
    sa.hbytes = (const unsigned long long *)pcrd_hb.ptr;
    sa.hcount = (const uint32_t *)pcrd_hc.ptr;
    sa.budget = (const int64_t *)budget.ptr;
    sa.lkey = (uint64_t *)sel_key.ptr;
    sa.lsize = (uint32_t *)sel_size.ptr;
    sa.ctl = (uint32_t *)sel_ctl.ptr;
    sa.K = (uint64_t *)thr.ptr;
    sa.Kc = (uint64_t *)thr.ptr + (size_t)G * kMaxLayers;
    sa.grp_b0 = (const int32_t *)grptab.ptr;
    sa.grp_seg0 = (const uint32_t *)grptab.ptr + G + 1;
    sa.lossless = plan.rc.rate_bpp <= 0.0 && !by_rates;  // (by rates: budgets, whatever the top layer is)
    sa.gtot = (const unsigned long long *)gtot.ptr;
    for (int l = 0; l < plan.rc.layers; l++) sa.frac[l] = lossless_layer_frac(l, plan.rc.layers);
    sa.init_on = init ? (by_rates ? 2 : 1) : 0;
    if (init) sa.init = *init;
    // by rates, first iteration: the first budgets rates_load placed behind the targets
    if (init && by_rates) sa.budget = (const int64_t *)ltarget.ptr + kMaxLayers;
    sa.rs = rs;
    sa.budget_w = (int64_t *)budget.ptr;
    sa.dbg = nullptr;
#ifdef JP2HIP_DEBUG_DUMPS
    if (getenv("JP2HIP_DUMP_DIR")) {
        std::string e;
        if (ensure<int64_t>(dbgsel, 128, e)) sa.dbg = (int64_t *)dbgsel.ptr;
    }
#endif
    const dim3 grid((grp_max_blocks(plan) + kSelThreads - 1) / kSelThreads, G);
    if (qtarget) {
        // by PSNR targets: the distortion instantiations over the histogram of
        // quanta; no budgets, no loop state
        sa.hbytes = (const unsigned long long *)pcrd_hq.ptr;
        sa.lossless = 0;
        std::memcpy(sa.qtarget, qtarget, sizeof(int64_t) * plan.rc.layers);
        sa.lsize64 = (uint64_t *)sel_size.ptr;
        sa.hdist = (const int64_t *)hdist.ptr;
        sa.weight = (const double *)weight.ptr;
        sa.qbits = psnr_bits;
        hipLaunchKernelGGL(k_select<true>, grid, dim3(kSelThreads), 0, stream, sa);
        hipLaunchKernelGGL(k_select_resolve<true>, dim3(plan.rc.layers, G), dim3(kSelThreads), 0, stream, sa);
        return;
    }
    hipLaunchKernelGGL(k_select<false>, grid, dim3(kSelThreads), 0, stream, sa);
    hipLaunchKernelGGL(k_select_resolve<false>, dim3(plan.rc.layers, G), dim3(kSelThreads), 0, stream, sa);
}

// lossless "-rate -": each -flush_period stripe (rate-control group) keeps
// per layer the passes that fit lossless_layer_frac of its own tier-1 bytes
// (k_hull summed them per group); the last layer takes every pass
bool GpuEncoder::select_lossless(const Plan &plan, std::string &err) {
    HIPCHECK(hipSetDevice(device));
    HIPCHECK(hipEventRecord(ev[kEvSelectBegin], stream));
    select_launch(plan, nullptr);
    HIPCHECK(hipGetLastError());
    return apply_thresholds(plan, nullptr, err);
}

// by PSNR targets (jp2hip_set_layer_psnr): per layer the highest threshold
// that leaves at most target[l] quanta (layer_psnr_targets); what follows is
// the fixed-slope encode at those keys (k_apply, tier-2, the report)
bool GpuEncoder::select_psnr(const Plan &plan, const int64_t *target, std::string &err) {
    HIPCHECK(hipSetDevice(device));
    if (!psnr_bits || !pcrd_hq.ptr) {
        err = "select_psnr: the hulls were built without the histogram of quanta";
        return false;
    }
    HIPCHECK(hipEventRecord(ev[kEvSelectBegin], stream));
    select_launch(plan, nullptr, nullptr, nullptr, false, target);
    HIPCHECK(hipGetLastError());
    return apply_thresholds(plan, nullptr, err);
}

bool GpuEncoder::select_keys(const Plan &plan, const std::vector<uint64_t> &K, std::string &err) {
    HIPCHECK(hipSetDevice(device));
    const int G = plan.ngroups(), L = plan.rc.layers;
    if ((int)K.size() < L || L > kMaxLayers) {
        err = "select_keys: a key per layer expected";
        return false;
    }
    HIPCHECK(hipEventRecord(ev[kEvSelectBegin], stream));
    KeyArgs ka;
    ka.ngroups = G;
    ka.layers = L;
    for (int l = 0; l < kMaxLayers; l++) ka.key[l] = l < L ? K[(size_t)l] : 0ull;
    ka.thr = (uint64_t *)thr.ptr;  // (hull_launch reserved 2 G kMaxLayers keys)
    if (G > 0) hipLaunchKernelGGL(k_fill_keys, dim3(std::min(2 * G, 1024)), dim3(64), 0, stream, ka);
    HIPCHECK(hipGetLastError());
    return apply_thresholds(plan, nullptr, err);
}

// the layer report's distortion for the thresholds in `thr` (the final
// selection's), one host wait; d: kMaxLayers values, layers .. are 0
bool GpuEncoder::layer_dist(const Plan &plan, double *d, std::string &err) {
    HIPCHECK(hipSetDevice(device));
    const int nb = (int)plan.blocks.size();
    std::fill(d, d + kMaxLayers, 0.0);
    if (!nb) return true;
    const int nparts = (nb + kDistThreads - 1) / kDistThreads;
    if (!ensure<double>(ldist, ((size_t)nparts + 1) * kMaxLayers, err)) return false;
    if (!h_dist) HIPCHECK(hipHostMalloc((void **)&h_dist, kMaxLayers * sizeof(double), hipHostMallocDefault));
    DistArgs da;
    da.nblocks = nb;
    da.layers = plan.rc.layers;
    da.lossless = plan.rc.rate_bpp <= 0.0;
    da.ngroups = plan.ngroups();
    da.nparts = nparts;
    da.grp_b0 = (const int32_t *)grptab.ptr;
    da.nhull = (const uint8_t *)nhull.ptr;
    da.npasses = (const uint8_t *)npasses.ptr;
    da.hkey = (const uint64_t *)hkey.ptr;
    da.K = (const uint64_t *)thr.ptr;
    da.dists = (const int64_t *)dists.ptr;
    da.hdist = (const int64_t *)hdist.ptr;
    da.weight = (const double *)weight.ptr;
    da.part = (double *)ldist.ptr;
    da.out = (double *)ldist.ptr + (size_t)nparts * kMaxLayers;
    hipLaunchKernelGGL(k_layer_dist, dim3(nparts), dim3(kDistThreads), 0, stream, da);
    hipLaunchKernelGGL(k_layer_dist_sum, dim3(1), dim3(64), 0, stream, da);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(h_dist, da.out, kMaxLayers * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (!host_wait(err)) return false;
    std::memcpy(d, h_dist, kMaxLayers * sizeof(double));
    return true;
}

// per-block layer tables for the thresholds in `thr` (kEvSelectBegin already recorded)
bool GpuEncoder::apply_thresholds(const Plan &plan, const int *halt, std::string &err) {
    const int nb = (int)plan.blocks.size();
    const int L = plan.rc.layers;
    ApplyArgs aa;
    aa.halt = halt;
    aa.nblocks = nb;
    aa.layers = L;
    aa.lossless = plan.rc.rate_bpp <= 0.0;
    aa.nhull = (const uint8_t *)nhull.ptr;
    aa.hpass = (const uint8_t *)hpass.ptr;
    aa.npasses = (const uint8_t *)npasses.ptr;
    aa.hkey = (const uint64_t *)hkey.ptr;
    aa.K = (const uint64_t *)thr.ptr;
    aa.rates = (const int32_t *)rates.ptr;
    aa.nl = (uint8_t *)nl.ptr;
    aa.lrate = (int32_t *)lrate.ptr;
    aa.ngroups = plan.ngroups();
    aa.grp_b0 = (const int32_t *)grptab.ptr;
    // (k_t2_wave assigns the layers itself in its sizing pass)
    if (nb && !t2_wave) hipLaunchKernelGGL(k_apply, dim3((nb + 255) / 256), dim3(256), 0, stream, aa);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(ev[kEvSelectEnd], stream));
    return true;
}

// An encode by per-layer rates: kMaxLayers targets, then kMaxLayers first
// budgets (layer_rate_targets), which the loop's first k_select and every step read
bool GpuEncoder::rates_load(const int64_t *target, const int64_t *first_budget, std::string &err) {
    HIPCHECK(hipSetDevice(device));
    int64_t tb[2 * kMaxLayers];
    std::memcpy(tb, target, sizeof(int64_t) * kMaxLayers);
    std::memcpy(tb + kMaxLayers, first_budget, sizeof(int64_t) * kMaxLayers);
    return ensure<int64_t>(ltarget, 2 * kMaxLayers, err) && h2d(ltarget.ptr, tb, sizeof tb, err);
}

// Device rate loop (RateState, jp2hip_internal.h): the first k_select of a
// restart writes the initial state; the step itself is rate_step in
// device_common.h, run by the sizing totals (t2_total_body: the last
// workgroup of k_t2_wave<false>, or k_t2_total)
bool GpuEncoder::rate_loop(const Plan &plan, const RateState &init, bool restart, int batch, bool profile,
                           StageTimes &st, RateState &rs, T2Summary &sum, std::string &err, bool by_rates) {
    HIPCHECK(hipSetDevice(device));
    if (!ensure<RateState>(rstate, 1, err)) return false;
    if (!h_rs) {  // host-mapped: k_rate_step writes the state and summary here
        HIPCHECK(hipHostMalloc((void **)&h_rs, sizeof(RateState) + sizeof(T2Summary), hipHostMallocMapped));
        HIPCHECK(hipHostGetDevicePointer((void **)&d_rs_out, h_rs, 0));
    }
    RateState *d = (RateState *)rstate.ptr;
    const int *halt = &d->halt;
    HIPCHECK(hipEventRecord(ev[kEvSelectBegin], stream));
    for (int i = 0; i < batch; i++) {
        // (the first k_select of a restart also initialises the loop's state)
        select_launch(plan, halt, (restart && i == 0) ? &init : nullptr, d, by_rates);
        if (!apply_thresholds(plan, halt, err)) return false;
        t2_size_launch(plan, true, halt, d, d_rs_out, by_rates);  // (the summary lands behind the state)
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(ev[kEvT2End], stream));
    if (!host_wait(err)) return false;
#ifdef JP2HIP_DEBUG_DUMPS
    if (const char *dd = getenv("JP2HIP_DUMP_DIR"))
        if (dbgsel.ptr && !dump(dd, "seldbg.bin", dbgsel, 128 * 8, err)) return false;
#endif
    std::atomic_thread_fence(std::memory_order_acquire);
    std::memcpy(&sum, h_rs + 1, sizeof sum);
    std::memcpy(&rs, h_rs, sizeof rs);
    if (profile) {
        float t;
        HIPCHECK(hipEventElapsedTime(&t, ev[kEvSelectBegin], ev[kEvT2End]));
        st.t2 += t;
    }
    return true;
}

bool GpuEncoder::segments(const Plan &plan, std::vector<uint64_t> &keys, std::vector<int64_t> &cum,
                          std::string &err, bool quanta) {
    HIPCHECK(hipSetDevice(device));
    // every hull segment (key, bytes), listed on the device, sorted here by
    // key, descending (the tile-split exchange's input; the single-image path
    // never needs the whole order: k_select)
    const int nb = (int)plan.blocks.size();
    keys.clear();
    cum.clear();
    if (!nb) return true;
    if (!ensure<int32_t>(segcnt, nb, err) || !ensure<int32_t>(segoff, nb, err) ||
        !ensure<uint64_t>(segkey, std::max(nseg, 1), err) || !ensure<int64_t>(segval, std::max(nseg, 1), err))
        return false;
    hipLaunchKernelGGL(k_seg_offsets, dim3(1), dim3(kSegThreads), 0, stream, nb, (const uint8_t *)nhull.ptr,
                       (int32_t *)segcnt.ptr, (int32_t *)segoff.ptr);
    hipLaunchKernelGGL(k_seg_emit, dim3((nb + 255) / 256), dim3(256), 0, stream, nb, (const uint8_t *)nhull.ptr,
                       (const uint8_t *)hpass.ptr, (const uint64_t *)hkey.ptr, (const int32_t *)rates.ptr,
                       (const int32_t *)segoff.ptr, (uint64_t *)segkey.ptr, (int64_t *)segval.ptr,
                       (const int64_t *)hdist.ptr, (const double *)weight.ptr, quanta ? psnr_bits : 0);
    HIPCHECK(hipGetLastError());
    int32_t *tail = (int32_t *)(h_tot + 5);  // pinned
    tail[0] = tail[1] = 0;
    HIPCHECK(hipMemcpyAsync(&tail[0], (int32_t *)segoff.ptr + nb - 1, 4, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(&tail[1], (int32_t *)segcnt.ptr + nb - 1, 4, hipMemcpyDeviceToHost, stream));
    if (!host_wait(err)) return false;
    const int n = tail[0] + tail[1];
    std::vector<uint64_t> k((size_t)n);
    std::vector<int64_t> v((size_t)n);
    if (n > 0) {
        HIPCHECK(hipMemcpyAsync(k.data(), segkey.ptr, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipMemcpyAsync(v.data(), segval.ptr, sizeof(int64_t) * n, hipMemcpyDeviceToHost, stream));
    }
    if (!host_wait(err)) return false;
    std::vector<int> idx((size_t)n);
    for (int i = 0; i < n; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int x, int y) { return k[x] > k[y]; });
    keys.resize((size_t)n);
    cum.resize((size_t)n);
    int64_t acc = 0;
    for (int i = 0; i < n; i++) {
        keys[i] = k[idx[i]];
        acc += v[idx[i]];
        cum[i] = acc;
    }
    return true;
}

}  // namespace jp2hip
