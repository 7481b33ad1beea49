// CPU unit test of the pinned output pool's rules (csrc/pinned_pool.h), with
// counting malloc / free in place of hipHostMalloc / hipHostFree.
#include "pinned_pool.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                              \
        }                                                            \
    } while (0)

static std::map<void *, size_t> g_pinned;  // pinned and not yet unpinned: bytes
static std::vector<size_t> g_pin_log, g_unpin_log;
static void *pin(size_t n) {
    void *p = std::malloc(n);
    g_pinned[p] = n;
    g_pin_log.push_back(n);
    return p;
}
static void unpin(void *p) {
    g_unpin_log.push_back(g_pinned.at(p));
    g_pinned.erase(p);
    std::free(p);
}
static size_t cap_of(size_t n) { return n + n / 8 + 4096; }

int main() {
    using jp2hip::PinnedPool;
    const size_t MiB = (size_t)1 << 20;
    {
        PinnedPool lib(pin, unpin);  // the library's floor
        CHECK(lib.idle_cap() == (size_t)4 << 30);
    }
    PinnedPool P(pin, unpin, 40000);
    auto settled = [&] { return P.idle_bytes() <= P.idle_cap(); };
    // a miss pins n + n/8 + 4096 bytes; n = 0 counts as 1
    uint8_t *z = P.alloc(0);
    CHECK(z && g_pin_log.back() == 1 + 4096);
    z[0] = 1;
    uint8_t *a = P.alloc(3 * MiB);
    const size_t ca = cap_of(3 * MiB);
    CHECK(a && g_pin_log.back() == ca && g_pin_log.size() == 2);
    a[ca - 1] = 1;
    // a pointer the pool never issued goes to free(), not to unpin
    P.free(std::malloc(16));
    CHECK(g_unpin_log.empty() && P.idle_count() == 0);
    P.free(nullptr);
    // the cap: peak_live (2) * max_cap lifts it above the floor
    CHECK(P.idle_cap() == 2 * ca);
    P.free(a);
    CHECK(P.idle_count() == 1 && P.idle_bytes() == ca && settled());
    // reuse for n when n <= cap <= 2n + 1 MiB, and not outside that window
    const size_t lo = (ca - MiB) / 2;  // 2 * lo + 1 MiB == cap
    CHECK(2 * lo + MiB == ca);
    uint8_t *under = P.alloc(lo - 1), *over = P.alloc(ca + 1);
    CHECK(under != a && g_pin_log.size() == 4 && g_pin_log[2] == cap_of(lo - 1));
    CHECK(over != a && g_pin_log[3] == cap_of(ca + 1));
    CHECK(P.alloc(lo) == a && g_pin_log.size() == 4 && P.idle_count() == 0);
    P.free(a);
    CHECK(P.alloc(ca) == a && g_pin_log.size() == 4);
    P.free(a);
    // the smallest fitting buffer is chosen: `a` and `over` both hold 2 MB
    // within the window, `under` and z are too small
    P.free(z);
    P.free(over);
    P.free(under);
    CHECK(P.idle_count() == 4 && settled());
    uint8_t *s = P.alloc(2000000), *m = P.alloc(2000000);
    CHECK(s == a && m == over && g_pin_log.size() == 4);
    P.free(m);
    P.free(s);
    CHECK(P.idle_count() == 4 && settled() && g_unpin_log.empty());

    // eviction: the largest idle buffer goes first
    PinnedPool Q(pin, unpin, 40000);
    const size_t pins0 = g_pin_log.size();
    Q.free(Q.alloc(10000));  // 15 346, kept
    Q.free(Q.alloc(15347));  // misses (larger than the idle one): 21 361, kept: 36 707 <= 40 000
    CHECK(Q.idle_count() == 2 && Q.idle_bytes() == cap_of(10000) + cap_of(15347) && g_unpin_log.empty());
    CHECK(Q.idle_cap() == 40000);
    uint8_t *c = Q.alloc(21362), *d = Q.alloc(30000);  // both miss; 2 live at once
    CHECK(g_pin_log.size() == pins0 + 4 && Q.idle_cap() == 2 * cap_of(30000));
    Q.free(d);  // 74 553 <= 75 692
    CHECK(g_unpin_log.empty() && Q.idle_count() == 3);
    Q.free(c);  // 102 681: the largest goes, not the buffer just returned
    CHECK(g_unpin_log.size() == 1 && g_unpin_log[0] == cap_of(30000));
    CHECK(Q.idle_count() == 3 && Q.idle_bytes() == cap_of(10000) + cap_of(15347) + cap_of(21362));
    CHECK(Q.idle_bytes() <= Q.idle_cap());
    // every pin is unpinned or idle
    CHECK(g_pin_log.size() - pins0 == g_unpin_log.size() + Q.idle_count());
    // one buffer live at a time: the floor is the cap, and holds
    PinnedPool R(pin, unpin, 40000);
    for (size_t n : {10000, 15347, 21362}) {  // each misses: larger than what is idle
        uint8_t *b = R.alloc(n);
        CHECK(b != nullptr && g_pin_log.back() == cap_of(n));
        R.free(b);
        CHECK(R.idle_cap() == 40000 && R.idle_bytes() <= R.idle_cap());
    }
    CHECK(g_unpin_log.size() == 2 && g_unpin_log[1] == cap_of(21362));  // 64 835 > 40 000
    CHECK(R.idle_count() == 2 && R.idle_bytes() == cap_of(10000) + cap_of(15347));
    CHECK(g_pinned.size() == P.idle_count() + Q.idle_count() + R.idle_count());
    for (auto &kv : g_pinned) std::free(kv.first);  // the pools are never destroyed in the library
    if (failures) return 1;
    std::printf("PINNED POOL OK\n");
    return 0;
}
