// orient.hip -- S1c orientation: a source whose TIFF Orientation is not 1
// becomes the upright image in HBM, so that ingest and everything after it
// see what they always saw (k_orient_flip, k_orient_transpose, and
// GpuEncoder::orient_samples, which enqueues one of them).  The map from an
// upright pixel to the stored one is orient_map.h's, here and on the host.
#include <hip/hip_runtime.h>

#include <string>

#include "gpu_encoder.h"
#include "hip_check.h"
#include "orient_map.h"
#include "store_run.h"

namespace jp2hip {

// Elements move whole (a 16-bit sample keeps its byte order, a pixel its
// component order): 1, 2, 3, 4, 6 or 8 bytes, handled as N units of type U.
template <int ES> struct OrientElem;
template <> struct OrientElem<1> { using U = uint8_t; };
template <> struct OrientElem<2> { using U = uint16_t; };
template <> struct OrientElem<3> { using U = uint8_t; };
template <> struct OrientElem<4> { using U = uint32_t; };
template <> struct OrientElem<6> { using U = uint16_t; };
template <> struct OrientElem<8> { using U = uint64_t; };

// where stored row y of plane p starts (strips may lie anywhere in the source)
__device__ __forceinline__ const uint8_t *orient_row(const OrientArgs &a, int p, int y, uint64_t row_bytes) {
    const int s = y / a.rps;
    return a.src + a.off[(size_t)p * a.spp_strips + s] + (uint64_t)(y - s * a.rps) * row_bytes;
}

// --------------------------------------------------------------------------
// o = 2, 3, 4: rows keep their length.  A lane owns a run of 48 destination
// bytes -- a whole number of elements of every size -- of one upright row,
// reads the run of the stored row that mirrors it (o = 4: the same run of the
// mirrored row), reverses the elements in registers and stores the run as
// k_expand does (store_run: as wide as the address allows).  The last run of
// a row may be short; it goes byte by byte.  No LDS.
// --------------------------------------------------------------------------
constexpr int kFlipRun = 48;

template <int ES>
__global__ void __launch_bounds__(256) k_orient_flip(OrientArgs a) {
    static_assert(kFlipRun % ES == 0, "a run holds whole elements");
    constexpr int NE = kFlipRun / ES;
    const uint64_t row_bytes = (uint64_t)a.w * ES;
    const uint64_t runs = (row_bytes + kFlipRun - 1) / kFlipRun;  // lanes per row
    const uint64_t rows = (uint64_t)(a.row1 - a.row0);
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= runs * rows * (uint64_t)a.planes) return;
    const int p = (int)(idx / (runs * rows));
    const uint64_t rem = idx % (runs * rows);
    const int r = (int)(rem / runs);
    const uint64_t b0 = (rem % runs) * kFlipRun;
    const int n = (int)min((uint64_t)kFlipRun, row_bytes - b0);  // bytes of this run
    const int uy = a.row0 + r;
    const int y = orient_flips_y(a.o) ? a.h - 1 - uy : uy;
    const bool flip = orient_flips_x(a.o);
    // the stored bytes the run is made from: the mirrored run ends where this one starts
    const uint8_t *sp = orient_row(a, p, y, row_bytes) + (flip ? row_bytes - b0 - (uint64_t)n : b0);
    uint32_t d[kFlipRun / 4];
    if (n == kFlipRun) {
        uint32_t s[kFlipRun / 4];
        __builtin_memcpy(s, sp, kFlipRun);  // (a strip may start at any byte)
        if (flip) {
#pragma unroll
            for (int q = 0; q < kFlipRun / 4; q++) {
                uint32_t v = 0;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int j = 4 * q + t, sj = (NE - 1 - j / ES) * ES + j % ES;
                    v |= ((s[sj >> 2] >> (8 * (sj & 3))) & 0xFFu) << (8 * t);
                }
                d[q] = v;
            }
        } else {
#pragma unroll
            for (int q = 0; q < kFlipRun / 4; q++) d[q] = s[q];
        }
    } else {
        const int ne = n / ES;
#pragma unroll
        for (int q = 0; q < kFlipRun / 4; q++) {
            uint32_t v = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int j = 4 * q + t;
                if (j < n) v |= (uint32_t)sp[flip ? (ne - 1 - j / ES) * ES + j % ES : j] << (8 * t);
            }
            d[q] = v;
        }
    }
    store_run<kFlipRun / 4>(a.dst + ((uint64_t)p * rows + (uint64_t)r) * row_bytes + b0, d, n);
}

// --------------------------------------------------------------------------
// o = 5..8: an upright row is a stored column.  A workgroup moves a tile of
// 64 x 64 elements through LDS: wave k loads stored rows k, k + 4, ... of the
// tile, a lane per element, so a wave reads one run of 64 elements; after the
// barrier lane l of every wave owns stored row l of the tile and the waves
// walk its columns, so a wave writes one run of 64 elements of an upright
// row (downwards where the orientation mirrors that axis: the same bytes).
// The column walk reads LDS a tile row apart per lane: the row pitch is the
// tile's 64 elements plus 4 bytes (8 for 8-byte elements, whose reads must
// stay 8-byte aligned), an odd number of dwords -- 65 dword pairs' worth for
// the 8-byte case, which a ds_read_b64 half-wave spreads over all 64 banks --
// so the 32 lanes of a half-wave fall on 32 different banks.  The largest
// tile, 64 x 520 bytes, is all the LDS the kernel has.  Edge tiles check
// every element against the image (and the band's columns).  c0, c1: the
// stored columns the upright rows [row0, row1) are (orient_source_cols).
// --------------------------------------------------------------------------
template <int ES>
__global__ void __launch_bounds__(256) k_orient_transpose(OrientArgs a, int c0, int c1) {
    using U = typename OrientElem<ES>::U;
    constexpr int T = kOrientTile, US = (int)sizeof(U), N = ES / US;
    constexpr int PITCH = (T * ES + (ES == 8 ? 8 : 4)) / US;  // units per tile row
    static_assert((T * ES + (ES == 8 ? 8 : 4)) % US == 0 && (size_t)T * PITCH * US <= 40 * 1024, "tile pitch");
    __shared__ U tile[T * PITCH];
    const int tx = threadIdx.x & (T - 1), ty = threadIdx.x / T;  // ty: the wave
    const int sx0 = c0 + (int)blockIdx.x * T, sy0 = (int)blockIdx.y * T, p = (int)blockIdx.z;
    const uint64_t row_bytes = (uint64_t)a.w * ES;
    {
        const int x = sx0 + tx;
        for (int r = ty; r < T; r += 256 / T) {
            const int y = sy0 + r;
            if (x < c1 && y < a.h) {
                const uint8_t *sp = orient_row(a, p, y, row_bytes) + (uint64_t)x * ES;
#pragma unroll
                for (int i = 0; i < N; i++) {
                    U u;
                    __builtin_memcpy(&u, sp + i * US, US);  // (a strip may start at any byte)
                    tile[r * PITCH + tx * N + i] = u;
                }
            }
        }
    }
    __syncthreads();
    const int y = sy0 + tx;
    if (y >= a.h) return;
    const uint64_t out_row_bytes = (uint64_t)a.h * ES, rows = (uint64_t)(a.row1 - a.row0);
    const uint64_t ux = (uint64_t)(orient_flips_y(a.o) ? a.h - 1 - y : y);
    for (int c = ty; c < T; c += 256 / T) {
        const int x = sx0 + c;
        if (x >= c1) break;
        const uint64_t r = (uint64_t)((orient_flips_x(a.o) ? a.w - 1 - x : x) - a.row0);
        // (the destination is this context's own buffer and every element
        // lies a multiple of ES bytes into it: U-aligned)
        U *dp = (U *)(a.dst + ((uint64_t)p * rows + r) * out_row_bytes + ux * ES);
#pragma unroll
        for (int i = 0; i < N; i++) dp[i] = tile[tx * PITCH + c * N + i];
    }
}

template <int ES>
static bool launch_orient_es(const OrientArgs &a, hipStream_t st) {
    if (!orient_swaps(a.o)) {
        const uint64_t runs = ((uint64_t)a.w * ES + kFlipRun - 1) / kFlipRun;
        const uint64_t nblk = (runs * (uint64_t)(a.row1 - a.row0) * (uint64_t)a.planes + 255) / 256;
        if (nblk > 0x7FFFFFFFull) return false;
        hipLaunchKernelGGL((k_orient_flip<ES>), dim3((unsigned)nblk), dim3(256), 0, st, a);
    } else {
        int64_t c0, c1;
        orient_source_cols(a.w, a.o, a.row0, a.row1, c0, c1);
        const int64_t gx = (c1 - c0 + kOrientTile - 1) / kOrientTile, gy = ((int64_t)a.h + kOrientTile - 1) / kOrientTile;
        if (gx > 0x7FFFFFFFll || gy > 65535 || a.planes > 65535) return false;
        hipLaunchKernelGGL((k_orient_transpose<ES>), dim3((unsigned)gx, (unsigned)gy, (unsigned)a.planes), dim3(256), 0,
                           st, a, (int)c0, (int)c1);
    }
    return hipGetLastError() == hipSuccess;
}

bool launch_orient(const OrientArgs &a, int es, hipStream_t st) {
    if (a.o < 2 || a.o > 8 || a.w <= 0 || a.h <= 0 || a.rps <= 0 || a.planes <= 0 || a.row0 < 0 || a.row1 <= a.row0 ||
        a.row1 > (orient_swaps(a.o) ? a.w : a.h))
        return false;
    switch (es) {
    case 1: return launch_orient_es<1>(a, st);
    case 2: return launch_orient_es<2>(a, st);
    case 3: return launch_orient_es<3>(a, st);
    case 4: return launch_orient_es<4>(a, st);
    case 6: return launch_orient_es<6>(a, st);
    case 8: return launch_orient_es<8>(a, st);
    default: return false;
    }
}

// `lay` describes the whole stored image as uncompressed strips of 8- or
// 16-bit samples in d_src (its table's entries for the stored rows that
// upright rows [row0, row1) are made from are valid, prepare_source.cpp); those
// upright rows are written into this context's `oriented` buffer, plane after
// plane.  The strip table goes through the pinned staging like every host ->
// device copy of an encode; nothing here waits for the GPU.
bool GpuEncoder::orient_samples(const void *d_src, const jp2hip_layout &lay, int o, int row0, int row1, bool profile,
                                const void **d_out, std::string &err) {
    HIPCHECK(hipSetDevice(device));
    const int planes = lay.planar == 2 ? lay.components : 1;
    const int es = (lay.planar == 2 ? 1 : lay.components) * (lay.bits >> 3);
    if ((lay.bits != 8 && lay.bits != 16) || lay.compression > 1 || lay.tile_width > 0 || lay.rows_per_strip <= 0) {
        err = "layout: the orientation needs uncompressed strips of 8- or 16-bit samples";
        return false;
    }
    const int64_t spp = ((int64_t)lay.height + lay.rows_per_strip - 1) / lay.rows_per_strip;
    if (spp * planes > lay.nstrips) {
        err = "layout: too few strips";
        return false;
    }
    int64_t ow, oh;
    orient_size(lay.width, lay.height, o, ow, oh);
    const size_t out_bytes = (size_t)planes * (size_t)(row1 - row0) * (size_t)ow * (size_t)es;
    if (!ensure<uint8_t>(oriented, out_bytes, err) || !ensure<uint64_t>(oroff, (size_t)(spp * planes), err)) return false;
    if (!h2d(oroff.ptr, lay.strip_offsets, sizeof(uint64_t) * (size_t)(spp * planes), err)) return false;
    OrientArgs a;
    a.src = (const uint8_t *)d_src;
    a.off = (const uint64_t *)oroff.ptr;
    a.w = lay.width;
    a.h = lay.height;
    a.o = o;
    a.rps = lay.rows_per_strip;
    a.spp_strips = (int)spp;
    a.planes = planes;
    a.row0 = row0;
    a.row1 = row1;
    a.dst = (uint8_t *)oriented.ptr;
    if (profile) HIPCHECK(hipEventRecord(ev[kEvOrientBegin], stream));
    if (!launch_orient(a, es, stream)) {
        err = std::string("orientation launch failed: ") + hipGetErrorString(hipGetLastError());
        return false;
    }
    if (profile) HIPCHECK(hipEventRecord(ev[kEvOrientEnd], stream));
    orient_timed = profile;
    *d_out = oriented.ptr;
    return true;
}

}  // namespace jp2hip
