// store_run.h -- a lane's run of output bytes, held in registers, stored as
// widely as its address allows (k_expand, k_orient_flip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace jp2hip {

// d[] holds 4 * NDW bytes, of which the first nbytes go to p: whole 16-byte
// stores where p is 16-byte aligned, dwords where it is 4-byte aligned, single
// bytes up to the next dword boundary, aligned dwords and single bytes after
// the last one otherwise, and byte by byte for a short (ragged) run.
template <int NDW>
__device__ __forceinline__ void store_run(uint8_t *p, const uint32_t (&d)[NDW], int nbytes) {
    const uintptr_t ap = (uintptr_t)p;
    if (nbytes == 4 * NDW && (ap & 15) == 0) {
#pragma unroll
        for (int i = 0; i < NDW; i += 4) *(uint4 *)(p + 4 * i) = make_uint4(d[i], d[i + 1], d[i + 2], d[i + 3]);
    } else if (nbytes == 4 * NDW && (ap & 3) == 0) {
#pragma unroll
        for (int i = 0; i < NDW; i++) *(uint32_t *)(p + 4 * i) = d[i];
    } else if (nbytes == 4 * NDW) {
        // a whole run m = 1..3 bytes past a dword boundary: 4 - m bytes up to
        // the boundary, NDW - 1 aligned dwords taken across d[k] | d[k + 1],
        // then the last m bytes
        const uint32_t m = (uint32_t)(ap & 3), sh = 8 * (4 - m);
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (i < (int)(4 - m)) p[i] = (uint8_t)(d[0] >> (8 * i));
        uint8_t *q = p + (4 - m);
#pragma unroll
        for (int k = 0; k < NDW - 1; k++)
            *(uint32_t *)(q + 4 * k) = (uint32_t)((((uint64_t)d[k + 1] << 32) | d[k]) >> sh);
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (i < (int)m) q[4 * (NDW - 1) + i] = (uint8_t)(d[NDW - 1] >> (sh + 8 * i));
    } else {
#pragma unroll
        for (int b = 0; b < 4 * NDW; b++)  // (unrolled: d[] stays in registers)
            if (b < nbytes) p[b] = (uint8_t)(d[b >> 2] >> (8 * (b & 3)));
    }
}

}  // namespace jp2hip
