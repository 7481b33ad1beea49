// unpack_args.h -- arguments of the TIFF strip decoders (unpack.hip, lzw.hip).
// The host build of the inflate kernels (tests/test_inflate_host.py) includes
// this file too, so it needs nothing but <cstdint>.  Both include it inside
// namespace jp2hip (after <cstdint> has been seen outside it).
#pragma once

#include <cstdint>

// compressed strips / tiles -> uncompressed staging copy (unpack.hip, lzw.hip)
struct UnpackArgs {
    const uint8_t *src;
    const uint64_t *off, *cnt;  // per strip (tile): byte offset and compressed size
    int nstrips, per_plane, rps, h;
    uint64_t row_bytes, stride;  // decoded row and strip stride (bytes)
    uint64_t unit_bytes;         // tiles: every unit decodes to this many bytes
    uint8_t *dst;
    const int *only;  // k_unlzw (lzw.hip): decode only strips with only[s] != 0 (nullptr: all)
    int *err;
    uint32_t *lnk;    // k_inflate: a link per output byte, strip s at lnk + s * stride
};
__host__ __device__ inline uint64_t strip_out_bytes(const UnpackArgs &a, int s) {
    if (a.unit_bytes) return a.unit_bytes;
    const int y0 = (s % a.per_plane) * a.rps;
    return (uint64_t)(a.rps < a.h - y0 ? a.rps : a.h - y0) * a.row_bytes;
}
