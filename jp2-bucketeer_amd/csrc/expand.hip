// expand.hip -- S1b sample expansion: bilevel, 2- and 4-bit grey and
// palette-colour sources become ordinary 8-bit samples in HBM, so that ingest
// and everything after it see what they always saw (k_expand, and
// GpuEncoder::expand_samples, which enqueues it).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gpu_encoder.h"
#include "hip_check.h"
#include "store_run.h"

namespace jp2hip {

// --------------------------------------------------------------------------
// One lane expands 16 pixels of one row: 2 * BITS source bytes, which lie in
// one unit because a row of a strip or of a tile starts on a byte boundary
// and tile widths are multiples of 16 pixels.  Grey: v of BITS bits becomes
// v * 255 / (2^BITS - 1), 16 output bytes.  Palette: the index selects a dword
// (R | G << 8 | B << 16) of the table in LDS, 48 output bytes.  The expansion
// is also the untiling: the lane's unit is found from (x, y) as k_untile does.
// Output rows are w (3 w) bytes, so a lane's run is 16-byte aligned only when
// its row's start is; it is stored as whole 16-byte stores where it is, as
// dwords where it is 4-byte aligned, as single bytes up to the next dword
// boundary, aligned dwords and single bytes after the last one otherwise, and
// byte by byte in the ragged last run of a row.
// --------------------------------------------------------------------------
constexpr int kExpandPx = 16;  // pixels per lane

template <int BITS, bool PALETTE>
__global__ void __launch_bounds__(256) k_expand(ExpandArgs a) {
    static_assert(BITS == 1 || BITS == 2 || BITS == 4 || (BITS == 8 && PALETTE), "sample depth");
    __shared__ uint32_t s_lut[PALETTE ? (1 << BITS) : 1];
    if (PALETTE) {
        for (int i = threadIdx.x; i < (1 << BITS); i += 256) s_lut[i] = a.lut[i];
        __syncthreads();
    }
    const uint32_t groups = ((uint32_t)a.w + kExpandPx - 1) / kExpandPx;  // lanes per row
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (uint64_t)groups * (uint32_t)a.rows) return;
    const uint32_t y = (uint32_t)(idx / groups), x0 = (uint32_t)(idx % groups) * kExpandPx;
    const int n = min(kExpandPx, a.w - (int)x0);  // pixels of this run
    const uint32_t u = (y / (uint32_t)a.unit_h) * (uint32_t)a.across + x0 / (uint32_t)a.unit_w;
    const uint32_t bo = (x0 % (uint32_t)a.unit_w) * BITS / 8;  // byte of the unit row where the run starts
    const uint8_t *sp = a.src + a.off[u] + (uint64_t)(y % (uint32_t)a.unit_h) * a.row_bytes + bo;
    constexpr int SB = 2 * BITS;  // source bytes of a whole run
    const int nb = min(SB, (int)(a.row_bytes - bo));  // (a row's last run may be shorter)
    uint32_t v[kExpandPx];
    if (BITS == 8) {
#pragma unroll
        for (int i = 0; i < kExpandPx; i++) v[i] = i < nb ? sp[i] : 0;
    } else {
        uint64_t acc = 0;  // the run's bits, first pixel highest
#pragma unroll
        for (int k = 0; k < SB; k++) {
            uint32_t b = k < nb ? sp[k] : 0;
            if (a.lsb_first) b = __builtin_bitreverse8((uint8_t)b);
            acc = (acc << 8) | b;
        }
#pragma unroll
        for (int i = 0; i < kExpandPx; i++) v[i] = (uint32_t)(acc >> (8 * SB - BITS * (i + 1))) & ((1u << BITS) - 1);
    }
    if (PALETTE) {
        uint32_t d[12];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t c0 = s_lut[v[4 * q]], c1 = s_lut[v[4 * q + 1]], c2 = s_lut[v[4 * q + 2]],
                           c3 = s_lut[v[4 * q + 3]];
            d[3 * q] = c0 | (c1 << 24);
            d[3 * q + 1] = (c1 >> 8) | (c2 << 16);
            d[3 * q + 2] = (c2 >> 16) | (c3 << 8);
        }
        store_run<12>(a.dst + ((uint64_t)y * (uint32_t)a.w + x0) * 3, d, 3 * n);
    } else {
        constexpr uint32_t scale = 255u / ((1u << BITS) - 1);  // 255, 85, 17
        uint32_t d[4];
#pragma unroll
        for (int q = 0; q < 4; q++)
            d[q] = ((v[4 * q] | (v[4 * q + 1] << 8) | (v[4 * q + 2] << 16) | (v[4 * q + 3] << 24)) * scale) ^ a.invert;
        store_run<4>(a.dst + (uint64_t)y * (uint32_t)a.w + x0, d, n);
    }
}

bool launch_expand(const ExpandArgs &a, int bits, bool palette, hipStream_t st) {
    const uint64_t lanes = (uint64_t)((a.w + kExpandPx - 1) / kExpandPx) * (uint64_t)a.rows;
    const uint64_t nblk = (lanes + 255) / 256;
    if (a.w <= 0 || a.rows <= 0 || a.unit_w <= 0 || a.unit_h <= 0 || nblk > 0x7FFFFFFFull) return false;
    const dim3 g((unsigned)nblk), b(256);
    if (palette) {
        if (bits == 1) hipLaunchKernelGGL((k_expand<1, true>), g, b, 0, st, a);
        else if (bits == 2) hipLaunchKernelGGL((k_expand<2, true>), g, b, 0, st, a);
        else if (bits == 4) hipLaunchKernelGGL((k_expand<4, true>), g, b, 0, st, a);
        else if (bits == 8) hipLaunchKernelGGL((k_expand<8, true>), g, b, 0, st, a);
        else return false;
    } else {
        if (bits == 1) hipLaunchKernelGGL((k_expand<1, false>), g, b, 0, st, a);
        else if (bits == 2) hipLaunchKernelGGL((k_expand<2, false>), g, b, 0, st, a);
        else if (bits == 4) hipLaunchKernelGGL((k_expand<4, false>), g, b, 0, st, a);
        else return false;
    }
    return hipGetLastError() == hipSuccess;
}

// `lay` describes uncompressed units (strips or tiles of grid `g`, one sample
// per pixel) in d_src; its rows are expanded into this context's `expanded`
// buffer.  lut: 2^bits dwords for a palette, else nullptr.  The offset table
// and the colour table go through the pinned staging like every host ->
// device copy of an encode; nothing here waits for the GPU.
bool GpuEncoder::expand_samples(const void *d_src, const jp2hip_layout &lay, const UnitGrid &g, const uint32_t *lut,
                                bool profile, const void **d_out, std::string &err) {
    HIPCHECK(hipSetDevice(device));
    const bool palette = lut != nullptr;
    const int rows = lay.height, unit_w = (int)g.unit_w, unit_h = (int)g.unit_h, units = (int)g.needed;
    if (g.planes != 1 || units > lay.nstrips || lay.bits > 8 || (g.tiled && unit_w % kExpandPx)) {
        err = "layout: sample expansion needs one unit per strip / tile of its rows and tile widths in multiples of 16";
        return false;
    }
    const size_t out_bytes = (size_t)lay.width * rows * (palette ? 3 : 1);
    if (!ensure<uint8_t>(expanded, out_bytes, err) || !ensure<uint64_t>(exoff, units, err) ||
        !ensure<uint32_t>(exlut, 256, err))
        return false;
    if (!h2d(exoff.ptr, lay.strip_offsets, sizeof(uint64_t) * units, err)) return false;
    if (palette && !h2d(exlut.ptr, lut, sizeof(uint32_t) << lay.bits, err)) return false;
    ExpandArgs a;
    a.src = (const uint8_t *)d_src;
    a.off = (const uint64_t *)exoff.ptr;
    a.w = lay.width;
    a.rows = rows;
    a.unit_w = unit_w;
    a.unit_h = unit_h;
    a.across = (int)g.across;
    a.row_bytes = (uint32_t)g.row_bytes;
    a.lsb_first = lay.fill_order == 2 && lay.bits < 8;
    a.invert = lay.photometric == JP2HIP_PHOTO_WHITE_IS_ZERO ? 0xFFFFFFFFu : 0u;
    a.lut = (const uint32_t *)exlut.ptr;
    a.dst = (uint8_t *)expanded.ptr;
    if (profile) HIPCHECK(hipEventRecord(ev[kEvExpandBegin], stream));
    if (!launch_expand(a, lay.bits, palette, stream)) {
        err = std::string("sample expansion launch failed: ") + hipGetErrorString(hipGetLastError());
        return false;
    }
    if (profile) HIPCHECK(hipEventRecord(ev[kEvExpandEnd], stream));
    expand_timed = profile;
    *d_out = expanded.ptr;
    return true;
}

}  // namespace jp2hip
