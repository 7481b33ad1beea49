// dwt_fetch.h -- k_dwt_l1s's pixel fetch: which bytes of the source one
// access brings for a chunky pixel, and which of them are its samples.
// GPU-free (host and device): the kernel and the CPU test
// (tests/host/test_dwt_fetch.cpp, under ASan / UBSan) share these functions.
//
// A chunky pixel's NC samples are contiguous, so one access of
// px_load_bytes(NC, bps) bytes brings them all: 4 bytes for RGB8 (one more
// than the pixel) and RGBA8, 8 for RGB16 (two more) and RGBA16, the pixel
// itself for 1 and 2 components.  No access may end beyond `src_end`, the end
// of the last byte the per-sample path reads (source_end), or begin before
// the buffer: a pixel whose access would overrun is loaded from
// px_pullback() bytes earlier and the word shifted down by as many bytes.
// Only rows flagged by row_needs_pullback() take that path, so the others
// pay nothing per pixel.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JP2HIP_HD __host__ __device__ __forceinline__
#else
#define JP2HIP_HD inline
#endif

namespace jp2hip {

// bytes one access loads for a chunky pixel of nc samples of bps bytes
JP2HIP_HD constexpr int px_load_bytes(int nc, int bps) { return nc == 3 ? 4 * bps : nc * bps; }
// ... of which the pixel's own
JP2HIP_HD constexpr int px_bytes(int nc, int bps) { return nc * bps; }

// A row of row_bytes bytes at byte offset `off` of the source holds a pixel
// whose access would end beyond src_end.
JP2HIP_HD bool row_needs_pullback(uint64_t off, uint64_t row_bytes, int nc, int bps, uint64_t src_end) {
    return off + row_bytes + (uint64_t)(px_load_bytes(nc, bps) - px_bytes(nc, bps)) > src_end;
}
// Bytes by which the access of the pixel at byte offset `addr` moves back so
// that it ends at src_end (0: it fits).  Needs src_end >= load bytes (the
// caller keeps the per-sample path for smaller sources: px_fetch_usable).
JP2HIP_HD int px_pullback(uint64_t addr, int load_bytes, uint64_t src_end) {
    return addr + (uint64_t)load_bytes > src_end ? (int)(addr + (uint64_t)load_bytes - src_end) : 0;
}
JP2HIP_HD bool px_fetch_usable(uint64_t src_end) { return src_end >= 8; }

// The pixel at `p` as one or two little-endian words (w[1] only for 8-byte
// loads), read with a single access of LB bytes from p - back and shifted so
// byte k of the pixel is byte k of the words.  __builtin_memcpy: the compiler
// picks the (unaligned) load.
template <int LB>
JP2HIP_HD void px_load(const uint8_t *p, int back, uint32_t &w0, uint32_t &w1) {
    w1 = 0;
    if constexpr (LB == 1) {
        w0 = p[0];
    } else if constexpr (LB == 2) {
        uint16_t t;
        __builtin_memcpy(&t, p - back, 2);
        w0 = (uint32_t)t >> (8 * back);
    } else if constexpr (LB == 4) {
        uint32_t t;
        __builtin_memcpy(&t, p - back, 4);
        w0 = t >> (8 * back);
    } else {
        uint64_t t;
        __builtin_memcpy(&t, p - back, 8);
        t >>= 8 * back;
        w0 = (uint32_t)t;
        w1 = (uint32_t)(t >> 32);
    }
}

// The fetch of the chunky pixel at byte offset `addr` of `src`; `pull`: its
// row is flagged (row_needs_pullback).
template <int NC, int BPS>
JP2HIP_HD void px_fetch(const uint8_t *src, uint64_t addr, bool pull, uint64_t src_end, uint32_t &w0, uint32_t &w1) {
    constexpr int LB = px_load_bytes(NC, BPS);
    px_load<LB>(src + addr, pull ? px_pullback(addr, LB, src_end) : 0, w0, w1);
}

// sample c of the loaded pixel: the stored integer (8 bits, or 16 in the
// source's byte order -- the big-endian swap is a byte select)
JP2HIP_HD uint32_t px_sample8(uint32_t w0, int c) { return (w0 >> (8 * c)) & 0xFFu; }
JP2HIP_HD uint32_t px_sample16(uint32_t w0, uint32_t w1, int c, bool big_endian) {
    const uint32_t w = (c & 2) ? w1 : w0;
    const uint32_t h = (c & 1) ? w >> 16 : w & 0xFFFFu;
    return big_endian ? ((h & 0xFFu) << 8) | (h >> 8) : h;
}
// The level-shifted sample as f32.  (float)u - (float)off and
// (float)(int32_t)(u - off) are the same float: u, off and their difference
// are integers below 2^24, which f32 holds exactly, so the subtraction does
// not round (and -ffp-contract=off leaves it a subtraction).
JP2HIP_HD float px_shift_f32(uint32_t u, float off) { return (float)u - off; }

// End of the last byte the rows [row0, row1) of an image read from
// uncompressed strips (per-sample path): the bound every wider access stays
// under.  strip_off: the layout's table (planar 2: spp_strips entries per
// component); row_bytes: bytes of one row of a plane.
inline uint64_t source_end(const uint64_t *strip_off, int64_t rps, int64_t spp_strips, int planes, int64_t row0,
                           int64_t row1, uint64_t row_bytes) {
    uint64_t end = 0;
    if (row1 <= row0 || rps <= 0) return 0;
    for (int64_t s = row0 / rps; s <= (row1 - 1) / rps; s++) {
        const int64_t last = (s + 1) * rps < row1 ? (s + 1) * rps : row1;  // rows of strip s read: up to `last`
        for (int p = 0; p < planes; p++) {
            const uint64_t e = strip_off[p * spp_strips + s] + (uint64_t)(last - s * rps) * row_bytes;
            if (e > end) end = e;
        }
    }
    return end;
}

}  // namespace jp2hip
