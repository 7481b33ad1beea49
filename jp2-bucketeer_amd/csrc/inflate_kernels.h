// inflate_kernels.h -- k_inflate and k_inflate_links, included by unpack.hip
// only (inside namespace jp2hip, after unpack_args.h).  It includes nothing
// itself: tests/test_inflate_host.py compiles the same text for the host,
// behind the shims of tests/host/inflate_main.cpp.
//
// Deflate (RFC 1951) in a zlib wrapper (RFC 1950): TIFF compression 8
// (Adobe Deflate) and 32946 (the older Deflate code), in two phases.
//
// k_inflate, one wave per strip: a Huffman stream has no positions known
// before decoding it, so the symbol decode is one serial chain per strip.
// The wave runs it with wave-uniform control flow (the state in scalar
// registers) and keeps that chain short: it does not build the output.  Each
// output byte p gets a 32-bit link instead -- kLinkByte | value for a
// literal (or a stored-block byte), or the position of an earlier byte with
// the same value for a match byte (an overlapping match, dist < length,
// points before the match start: byte p0 + x -> p0 - dist + x mod dist) --
// written by the lanes with plain stores (no window, no read-back, no
// barrier).  Length and distance bases come from closed forms (scalar
// arithmetic), so a literal costs one table lookup and a match two.  The
// lanes are used where the work is parallel: the compressed bytes reach an LDS
// ring 1 KiB per vector load, one chunk ahead; the code tables are built by
// the lanes (ranks within a code length by ballot); a match's links and a
// stored block's bytes are written a lane per byte.
// k_inflate_links then resolves the links of every strip in parallel:
// pointer doubling (link[p] = link[link[p]], in place -- a link read while
// another thread rewrites it is still a valid link of the same value), then
// each byte follows what is left of its chain and is written out.
// kInfLanes is the wave width (the host build of tests/test_inflate_host.py
// runs the same text with one lane).
#ifndef JP2HIP_INF_LANES
#define JP2HIP_INF_LANES 64
#endif
constexpr int kInfLanes = JP2HIP_INF_LANES;
constexpr uint32_t kInChunkWords = 4 * kInfLanes;       // words per ring refill (16 bytes a lane)
constexpr uint32_t kInRingWords = 2 * (kInChunkWords > 16 ? kInChunkWords : 16);  // >= two chunks
constexpr int kInfLB = 12, kInfDB = 9;                  // direct-lookup bits: literal/length, distance
constexpr uint32_t kLinkByte = 0x80000000u;             // link of a byte whose value is known
// the literal/length direct lookup's entry for a longer code: bit 8 set like
// every non-literal's, so "literal" is one bit test (entries: len << 9 | sym)
constexpr uint32_t kInfNoFast = 0x100u;
constexpr int kLinkDoublings = 5;                       // pointer-doubling rounds before the chase

__constant__ uint8_t kInfClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// RFC 1951 3.2.5 in closed form: length code i = sym - 257 (0..28) and
// distance code d (0..29) -> (base, extra bits)
__device__ __forceinline__ uint32_t inf_len_extra(uint32_t i) { return i < 8u || i == 28u ? 0u : (i - 4u) >> 2; }
__device__ __forceinline__ uint32_t inf_len_base(uint32_t i) {
    return i == 28u ? 258u : (i < 8u ? 3u + i : ((4u + (i & 3u)) << inf_len_extra(i)) + 3u);
}
__device__ __forceinline__ uint32_t inf_dist_extra(uint32_t d) { return d < 4u ? 0u : (d >> 1) - 1u; }
__device__ __forceinline__ uint32_t inf_dist_base(uint32_t d) {
    return d < 4u ? d + 1u : ((2u + (d & 1u)) << inf_dist_extra(d)) + 1u;
}

__device__ __forceinline__ uint32_t inf_uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t inf_uni64(uint64_t v) {
    return ((uint64_t)inf_uni((uint32_t)(v >> 32)) << 32) | inf_uni((uint32_t)v);
}

struct InfShared {
    uint32_t ring[kInRingWords];          // compressed stream words
    uint16_t lfast[1 << kInfLB], dfast[1 << kInfDB];
    uint16_t lcnt[16], dcnt[16], lsym[288], dsym[32];
    uint8_t lens[320];
    uint32_t scr[64];                     // table-build scratch
};

// Bit reader over the strip's 16-byte-aligned words, fed from the LDS ring,
// addressed by absolute bit position P (bit 0 = bit 0 of the aligned base
// word; the stream starts at head_bits).  Words past the stream read as zero
// (never loaded): decoding runs on to the end of the strip's output or of the
// block, and a stream read past its end (P > end_bits) is reported corrupt at
// the end -- no per-read bookkeeping on the hot path.
struct InfIn {
    const uint32_t *w;                 // aligned base of the stream
    uint32_t nw;                       // words holding stream bytes
    uint64_t loaded;                   // words written to the ring
    uint64_t P;                        // next bit to read
    uint64_t head_bits, end_bits;      // where the stream starts / ends (bits)
    uint4 pre;                         // this lane's 16 bytes of the chunk after them
    uint32_t *ring;
    int lane;
    __device__ __forceinline__ uint4 chunk(uint64_t c) const {  // this lane's part of chunk c
        const uint64_t w0 = c * kInChunkWords + 4u * (uint32_t)lane;
        if (w0 + 4 <= nw) return *(const uint4 *)(w + w0);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (w0 + 0 < nw) v.x = w[w0 + 0];
        if (w0 + 1 < nw) v.y = w[w0 + 1];
        if (w0 + 2 < nw) v.z = w[w0 + 2];
        return v;
    }
    __device__ __forceinline__ void top_up() {  // the prefetched chunk into the ring, the next one in flight
        const uint64_t c = loaded / kInChunkWords;
        ((uint4 *)ring)[(c * kInfLanes + (uint32_t)lane) % (kInRingWords / 4)] = pre;
        loaded += kInChunkWords;
        pre = chunk(c + 1);
    }
    // the ring holds at least 8 words (256 bits) from P's word on: called once
    // per window / symbol / code length (each reads < 64 bits from P)
    __device__ __forceinline__ void ensure() {
        const uint64_t k = P >> 5;
        if (k + 8 >= loaded) {
            if (k >= loaded) {  // a jump (past a stored block): restart the ring at P's chunk
                loaded = (k / kInChunkWords) * kInChunkWords;
                pre = chunk(loaded / kInChunkWords);
            }
            do top_up(); while (k + 8 >= loaded);  // (once per 1 KiB on the GPU)
            __builtin_amdgcn_wave_barrier();
            // wave-uniform, after the lane-dependent loads: the decode keeps
            // running on the scalar unit
            loaded = inf_uni64(loaded);
        }
    }
    __device__ __forceinline__ void init(const uint8_t *in, uint64_t n, uint32_t *r, int ln) {
        const uint64_t addr = (uint64_t)(uintptr_t)in, head = addr & 15;
        w = (const uint32_t *)(uintptr_t)(addr - head);
        nw = (uint32_t)((head + n + 3) >> 2);
        ring = r;
        lane = ln;
        loaded = 0;
        pre = chunk(0);
        head_bits = 8 * head;
        end_bits = 8 * (head + n);
        P = head_bits;
        ensure();
    }
    // n <= 32 bits at bit position q (wave-uniform; the ring must hold them)
    __device__ __forceinline__ uint32_t bits_at(uint64_t q, int n) const {
        const uint64_t k = q >> 5;
        const uint32_t lo = inf_uni(ring[k % kInRingWords]), hi = inf_uni(ring[(k + 1) % kInRingWords]);
        const uint32_t v = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(q & 31));
        return n >= 32 ? v : v & ((1u << n) - 1u);
    }
    __device__ __forceinline__ uint32_t get(int n) {  // n <= 32
        const uint32_t v = bits_at(P, n);
        P += (uint64_t)n;
        return v;
    }
    __device__ __forceinline__ uint64_t consumed() const { return P - head_bits; }
    __device__ __forceinline__ void align() { P = (P + 7) & ~7ull; }  // to the next byte
};

// Canonical code of a length-walk (codes longer than the direct lookup),
// from bit position q; returns the symbol and sets *len (0: invalid)
__device__ int inf_walk_at(const InfIn &b, uint64_t q, const uint16_t *cnt, const uint16_t *sym, int *len) {
    int code = 0, first = 0, index = 0;
    const uint32_t v = b.bits_at(q, 16);
    for (int l = 1; l <= 15; l++) {
        code |= (int)((v >> (l - 1)) & 1u);
        const int count = (int)inf_uni(cnt[l]);
        if (code - count < first) {
            *len = l;
            return (int)inf_uni(sym[index + (code - first)]);
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    *len = 0;
    return -1;
}

// One symbol from P with the 2^FB-entry direct lookup (code-length tables)
template <int FB>
__device__ __forceinline__ int inf_decode(InfIn &b, const uint16_t *fast, const uint16_t *cnt, const uint16_t *sym) {
    const uint32_t e = inf_uni(fast[b.bits_at(b.P, FB)]);
    if (e) {
        b.P += e >> 9;
        return (int)(e & 511u);
    }
    int l;
    const int s = inf_walk_at(b, b.P, cnt, sym, &l);
    b.P += (uint64_t)l;
    return s;
}

// Canonical Huffman table from n code lengths, built by the lanes: 16
// per-length counts (LDS atomics), each length's first code and first symbol
// slot (one uniform pass over the 15 lengths), every symbol's rank among the
// lower-numbered symbols of its length (a ballot per length and chunk of
// kInfLanes symbols), then the symbols in code order and the 2^FB-entry
// direct lookup ((len << 9) | sym, 0: a longer code), a symbol per lane.
// `scr`: 64 words of LDS.  false: over-subscribed lengths (an incomplete
// code is accepted; its unused codes fail in inf_walk).
__device__ __forceinline__ uint32_t inf_ballot_below(bool p, int lane, uint32_t &tot) {
#if JP2HIP_INF_LANES > 1
    const uint64_t m = __ballot(p);
    tot = (uint32_t)__popcll(m);
    return (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
#else
    tot = p ? 1u : 0u;
    return 0u;
#endif
}
template <int FB, uint32_t EMPTY = 0u>
__device__ bool inf_build(uint16_t *cnt, uint16_t *sym, uint16_t *fast, const uint8_t *len, int n, int lane,
                          uint32_t *scr) {
    uint32_t *cl = scr, *offs = scr + 16, *next = scr + 32, *seen = scr + 48;
    for (int i = lane; i < 64; i += kInfLanes) scr[i] = 0u;
    const uint32_t e2 = EMPTY * 0x10001u;
    for (int i = lane; i < (1 << FB) / 8; i += kInfLanes) ((uint4 *)fast)[i] = make_uint4(e2, e2, e2, e2);
    __builtin_amdgcn_wave_barrier();
    for (int s = lane; s < n; s += kInfLanes)
        if (len[s]) atomicAdd(&cl[len[s]], 1u);
    __builtin_amdgcn_wave_barrier();
    int left = 1;
    uint32_t code = 0, off = 0;
    for (int l = 1; l < 16; l++) {
        const uint32_t c = inf_uni(cl[l]);
        left = (left << 1) - (int)c;
        if (lane == 0) {
            offs[l] = off;
            next[l] = code;
            cnt[l] = (uint16_t)c;
        }
        off += c;
        code = (code + c) << 1;
    }
    if (lane == 0) cnt[0] = 0;
    if (left < 0) return false;
    __builtin_amdgcn_wave_barrier();
    for (int s0 = 0; s0 < n; s0 += kInfLanes) {
        const int s = s0 + lane;
        const uint32_t l = s < n ? len[s] : 0u;
        uint32_t rank = 0;
        for (int q = 1; q < 16; q++) {
            uint32_t tot;
            const uint32_t below = inf_ballot_below(l == (uint32_t)q, lane, tot);
            if (tot) {
                if (l == (uint32_t)q) rank = seen[q] + below;
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) seen[q] += tot;
            }
        }
        if (l) {
            sym[offs[l] + rank] = (uint16_t)s;
            if ((int)l <= FB) {
                const uint32_t r = __builtin_bitreverse32(next[l] + rank) >> (32 - l);  // stream order: code MSB first
                for (uint32_t i = r; i < (1u << FB); i += 1u << l) fast[i] = (uint16_t)((l << 9) | (uint32_t)s);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    return true;
}

// The symbols of one Huffman block, a window of kInfLanes bit offsets at a
// time: lane l looks up the codes that would start at bit P + l (the
// literal/length table and the distance table, one LDS read each for the
// whole wave), then the walk follows the actual symbol boundaries through
// those lookups by readlane -- offset o, o + code length, ... -- with no
// memory access until the walk leaves the window.  Literals take a tight
// loop; a match's parts (length extra bits, distance code, distance extra
// bits) move to the next window whenever they start past this one.
// A run of literals is stored by the lanes that hold them (each lane's own
// table entry), at their ranks in the run; a match's links are stored by the
// lanes.
// Returns false on a corrupt stream; full = the strip is full.
__device__ __attribute__((noinline)) int inf_walk_slow(const InfIn &b, uint64_t q, const uint16_t *cnt,
                                                       const uint16_t *sym, int *len) {
    return inf_walk_at(b, q, cnt, sym, len);
}
__device__ bool inf_block(InfIn &b, InfShared &S, uint32_t *L, uint32_t cap, uint32_t &pos, bool &full, int lane) {
    uint32_t X = 0, Le = 0, De = 0, o = 0;
    // the window at P: this lane's 32 bits from P + lane and the two table
    // entries there
    auto window = [&]() {
        b.P += o;
        o = 0;
        b.ensure();
        const uint64_t q = b.P + (uint64_t)lane;
        const uint32_t kw = (uint32_t)(q >> 5) % kInRingWords;
        X = __builtin_amdgcn_alignbit(b.ring[(kw + 1) % kInRingWords], b.ring[kw], (uint32_t)(q & 31));
        Le = S.lfast[X & ((1u << kInfLB) - 1u)];
        De = S.dfast[X & ((1u << kInfDB) - 1u)];
    };
    window();
    for (;;) {
        // the walk's state is wave-uniform; say so (the compiler's divergence
        // analysis loses it through the stores of the lanes that hold literals)
        pos = inf_uni(pos);
        if (o >= (uint32_t)kInfLanes) {
            window();
            if (b.P > b.end_bits + 64) return false;  // far past the stream's end: truncated
        }
        // a run of literals inside this window: the walk only marks where
        // each starts (bit o of `run`); the lane at that offset already holds
        // the literal in its own table entry, and stores it at its rank in the
        // run (at most kInfLanes literals: each code is at least one bit)
        uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)Le, (int)o);
        if (!(e & 0x100u) && cap - pos >= (uint32_t)kInfLanes) {
            uint64_t run = 0;
            do {
                run |= 1ull << o;
                o += e >> 9;
                if (o >= (uint32_t)kInfLanes) break;
                e = (uint32_t)__builtin_amdgcn_readlane((int)Le, (int)o);
            } while (!(e & 0x100u));
            run = inf_uni64(run);
#if JP2HIP_INF_LANES > 1
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(run >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)run, 0u));
#else
            const uint32_t rank = 0u;
#endif
            if ((run >> lane) & 1ull) L[pos + rank] = kLinkByte | (Le & 255u);
            pos += (uint32_t)__popcll(run);
            if (o >= (uint32_t)kInfLanes) continue;
        } else if (!(e & 0x100u)) {  // near the strip's end: one literal at a time
            if (pos >= cap) {  // strip full: trailing data ignored
                full = true;
                b.P += o + (e >> 9);
                return true;
            }
            L[pos] = kLinkByte | (e & 255u);  // every lane stores the same word
            pos++;
            o += e >> 9;
            continue;
        }
        if (e == kInfNoFast) e = 0;  // (the walk below looks for 0)
        uint32_t cl = e >> 9, sy = e & 511u;
        if (!e) {  // a code longer than the direct lookup: walk it bit by bit
            int l;
            // (a call's results are per lane to the compiler: say they are uniform)
            const int ws = (int)inf_uni((uint32_t)inf_walk_slow(b, b.P + o, S.lcnt, S.lsym, &l));
            if (ws < 0) return false;
            cl = inf_uni((uint32_t)l);
            sy = (uint32_t)ws;
            if (sy < 256u) {  // (rare) a long literal code
                if (pos >= cap) {
                    full = true;
                    b.P += o + cl;
                    return true;
                }
                L[pos] = kLinkByte | sy;  // every lane stores the same word
                pos++;
                o += cl;
                continue;
            }
        }
        o += cl;
        if (sy == 256u) {  // end of block
            b.P += o;
            return true;
        }
        const uint32_t li = sy - 257u;
        if (li >= 29u) return false;
        if (o >= (uint32_t)kInfLanes) window();
        const uint32_t nl = inf_len_extra(li);
        uint32_t len = inf_len_base(li) + ((uint32_t)__builtin_amdgcn_readlane((int)X, (int)o) & ((1u << nl) - 1u));
        o += nl;
        if (o >= (uint32_t)kInfLanes) window();
        uint32_t ed = (uint32_t)__builtin_amdgcn_readlane((int)De, (int)o), dc = ed & 511u, dl = ed >> 9;
        if (!ed) {
            int l;
            const int ws = (int)inf_uni((uint32_t)inf_walk_slow(b, b.P + o, S.dcnt, S.dsym, &l));
            if (ws < 0) return false;
            dl = inf_uni((uint32_t)l);
            dc = (uint32_t)ws;
        }
        if (dc >= 30u) return false;
        o += dl;
        if (o >= (uint32_t)kInfLanes) window();
        const uint32_t nd = inf_dist_extra(dc);
        const uint32_t dist = inf_dist_base(dc) + ((uint32_t)__builtin_amdgcn_readlane((int)X, (int)o) & ((1u << nd) - 1u));
        o += nd;
        if (dist > pos) return false;
        bool cut = false;
        if (len > cap - pos) {  // the strip ends inside this match: keep what fits
            len = cap - pos;
            cut = true;
        }
        // each byte links to one before the match start (period dist when
        // the match overlaps itself)
        const uint32_t src = pos - dist;
        if (dist >= len) {
            for (uint32_t x = (uint32_t)lane; x < len; x += kInfLanes) L[pos + x] = src + x;
        } else {  // byte x repeats byte x mod dist before the match: one division per match
            uint32_t r = (uint32_t)lane % dist;
            const uint32_t step = (uint32_t)kInfLanes % dist;
            for (uint32_t x = (uint32_t)lane; x < len; x += kInfLanes) {
                L[pos + x] = src + r;
                r += step;
                r = r >= dist ? r - dist : r;
            }
        }
        pos += len;
        if (cut) {
            b.P += o;
            full = true;
            return true;
        }
    }
}

__global__ void __launch_bounds__(kInfLanes) k_inflate(UnpackArgs a) {
    __shared__ __attribute__((aligned(16))) InfShared S;
    const int s = blockIdx.x, lane = (int)threadIdx.x;
    if (s >= a.nstrips) return;
    // the strip's geometry as wave-uniform (scalar) values: everything the
    // decode derives from them stays scalar, and its branches too
    const uint8_t *in0 = a.src + inf_uni64(a.off[s]);
    const uint64_t n0 = inf_uni64(a.cnt[s]);
    const uint64_t cap64 = inf_uni64(strip_out_bytes(a, s));
    uint32_t *L = a.lnk + (uint64_t)s * a.stride;  // this strip's links
    if (cap64 >= (1ull << 31)) {  // a strip / tile of 2 GiB or more: not a TIFF the host parser accepts
        if (lane == 0) atomicOr(a.err, 2);
        return;
    }
    const uint32_t cap = (uint32_t)cap64;
    uint32_t pos = 0;
    const uint32_t h0 = inf_uni(n0 >= 1 ? in0[0] : 0u), h1 = inf_uni(n0 >= 2 ? in0[1] : 0u);
    bool bad = n0 < 2 || (h0 & 15) != 8 || (h0 >> 4) > 7 || ((h0 << 8) | h1) % 31 || (h1 & 0x20);
    InfIn b;
    b.init(in0, n0, S.ring, lane);
    b.P += 16;  // zlib CMF, FLG (checked above)
    bool last = false;
    while (!bad && !last) {
        b.ensure();
        last = b.get(1);
        const int type = (int)b.get(2);
        if (type == 0) {  // stored: to the byte boundary, LEN, ~LEN, then LEN bytes copied by the lanes
            b.align();
            uint32_t len = b.get(16);
            const uint32_t nlen = b.get(16);
            if (len != (~nlen & 0xFFFFu)) { bad = true; break; }
            const uint64_t at = b.consumed() / 8;  // the block's first byte in the stream
            if (at + len > n0) { bad = true; break; }     // truncated
            if (len > cap - pos) { len = cap - pos; last = true; }  // strip full: stop here
            for (uint32_t i = (uint32_t)lane; i < len; i += kInfLanes) L[pos + i] = kLinkByte | in0[at + i];
            pos += len;
            b.P += 8ull * len;
            continue;
        }
        if (type == 1) {  // fixed codes
            for (int i = lane; i < 318; i += kInfLanes)
                S.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
            __builtin_amdgcn_wave_barrier();
            inf_build<kInfLB, kInfNoFast>(S.lcnt, S.lsym, S.lfast, S.lens, 288, lane, S.scr);
            inf_build<kInfDB>(S.dcnt, S.dsym, S.dfast, S.lens + 288, 30, lane, S.scr);
        } else if (type == 2) {  // dynamic codes
            const int nlen = (int)b.get(5) + 257, ndist = (int)b.get(5) + 1, ncode = (int)b.get(4) + 4;
            if (nlen > 286 || ndist > 30) { bad = true; break; }
            b.ensure();
            for (int i = 0; i < 19; i++) {
                const uint32_t v = i < ncode ? b.get(3) : 0u;
                if (lane == 0) S.lens[kInfClOrder[i]] = (uint8_t)v;
            }
            __builtin_amdgcn_wave_barrier();
            if (!inf_build<7>(S.lcnt, S.lsym, S.lfast, S.lens, 19, lane, S.scr)) { bad = true; break; }
            int i = 0;
            while (i < nlen + ndist) {
                b.ensure();
                const int sy = inf_decode<7>(b, S.lfast, S.lcnt, S.lsym);
                if (sy < 0) { bad = true; break; }
                if (sy < 16) {
                    if (lane == 0) S.lens[i] = (uint8_t)sy;
                    i++;
                    continue;
                }
                uint32_t v = 0;
                int rep;
                if (sy == 16) {
                    if (i == 0) { bad = true; break; }
                    v = inf_uni(S.lens[i - 1]);
                    rep = 3 + (int)b.get(2);
                } else if (sy == 17) rep = 3 + (int)b.get(3);
                else rep = 11 + (int)b.get(7);
                if (i + rep > nlen + ndist) { bad = true; break; }
                for (int j = lane; j < rep; j += kInfLanes) S.lens[i + j] = (uint8_t)v;
                i += rep;
            }
            __builtin_amdgcn_wave_barrier();
            if (bad || inf_uni(S.lens[256]) == 0) { bad = true; break; }
            if (!inf_build<kInfLB, kInfNoFast>(S.lcnt, S.lsym, S.lfast, S.lens, nlen, lane, S.scr) ||
                !inf_build<kInfDB>(S.dcnt, S.dsym, S.dfast, S.lens + nlen, ndist, lane, S.scr)) {
                bad = true;
                break;
            }
        } else { bad = true; break; }
        __builtin_amdgcn_wave_barrier();
        bool full = false;
        if (!inf_block(b, S, L, cap, pos, full, lane)) { bad = true; break; }
        if (full) last = true;
    }
    bad = bad || b.P > b.end_bits;  // read past the end of the stream: truncated
    if (bad || pos != cap) {
        if (lane == 0) atomicOr(a.err, 2);
        // a strip that stopped short: its remaining links become known bytes
        // (0), so k_inflate_links never follows a stale or unwritten slot
        for (uint32_t i = pos + (uint32_t)lane; i < cap; i += kInfLanes) L[i] = kLinkByte;
    }
}

// Resolves every decoded strip's links (k_inflate) into its bytes: grid
// (chunks of kLinkChunk bytes, strips).  Rounds of pointer doubling first,
// one launch each (round < kLinkDoublings), then the last launch chases what
// is left of each chain and writes the bytes.  Links only point backwards
// within their strip, so every chain ends at a byte of known value.
constexpr int kLinkChunk = 4096;
__global__ void __launch_bounds__(256) k_inflate_links(UnpackArgs a, int chase) {
    const int s = blockIdx.y;
    const uint64_t cap64 = strip_out_bytes(a, s);
    if (cap64 >= (1ull << 31)) return;  // k_inflate refused the strip (error already set)
    const uint32_t cap = (uint32_t)cap64;
    uint32_t *L = a.lnk + (uint64_t)s * a.stride;
    uint8_t *out = a.dst + (uint64_t)s * a.stride;
    const uint32_t p0 = blockIdx.x * (uint32_t)kLinkChunk;
    // a well-formed link points strictly backwards; anything else (a corrupt
    // strip's slot) ends the chain, so every chase terminates in bounds
    for (uint32_t p = p0 + threadIdx.x; p < min(cap, p0 + (uint32_t)kLinkChunk); p += 256) {
        uint32_t v = L[p];
        if (!chase) {
            if (!(v & kLinkByte) && v < p) {
                const uint32_t u = L[v];
                if (u != v) L[p] = u;
            }
            continue;
        }
        uint32_t at = p;
        while (!(v & kLinkByte)) {
            if (v >= at) { v = kLinkByte; break; }
            at = v;
            v = L[v];
        }
        out[p] = (uint8_t)v;
    }
}

