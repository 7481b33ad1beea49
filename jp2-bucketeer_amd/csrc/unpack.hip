// unpack.hip -- compressed TIFF strips and tiles decoded in HBM before ingest:
// PackBits (k_unpackbits), Deflate (k_inflate, k_inflate_links; their text is
// inflate_kernels.h, which the CPU suite also compiles for the host),
// Predictor 2 (k_unpredict), tiles -> strips (k_untile), and
// GpuEncoder::unpack_strips, which enqueues them.  LZW is lzw.hip.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gpu_encoder.h"
#include "hip_check.h"

namespace jp2hip {

// --------------------------------------------------------------------------
// S1a: compressed strips (TIFF 6.0 sections 9, 13, 14; Deflate per the TIFF
// Technical Notes).  The strips of an LZW, Deflate or PackBits TIFF are
// decoded in HBM before ingest: one lane per strip (each strip is an
// independent byte stream), output strip s at s * stride of a
// staging buffer, so ingest then reads an uncompressed layout.  Horizontal
// differencing (Predictor 2) is undone afterwards, one lane per row.
// --------------------------------------------------------------------------

// PackBits: n in 0..127 copies n+1 literal bytes, -127..-1 repeats the next
// byte 1-n times, -128 is a no-op.  One strip per wave: every lane walks the
// same run headers (uniform control flow), and a run's bytes are written by
// the 64 lanes together.
__global__ void __launch_bounds__(64) k_unpackbits(UnpackArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= a.nstrips) return;
    const uint8_t *in = a.src + a.off[s];
    const uint64_t n = a.cnt[s], cap = strip_out_bytes(a, s);
    uint8_t *out = a.dst + (uint64_t)s * a.stride;
    uint64_t ip = 0, pos = 0;
    bool bad = false;
    while (ip < n && pos < cap) {
        const int c = (int8_t)in[ip++];
        // a run past the strip's end is cut at cap (libtiff keeps what fits)
        if (c >= 0) {
            if (ip + c + 1 > n) { bad = true; break; }
            const uint64_t m = min((uint64_t)c + 1, cap - pos);
            for (uint64_t i = lane; i < m; i += 64) out[pos + i] = in[ip + i];
            ip += c + 1;
            pos += m;
        } else if (c != -128) {
            if (ip >= n) { bad = true; break; }
            const uint8_t v = in[ip++];
            const uint64_t m = min((uint64_t)(1 - c), cap - pos);
            for (uint64_t i = lane; i < m; i += 64) out[pos + i] = v;
            pos += m;
        }
    }
    if (lane == 0 && (bad || pos != cap)) atomicOr(a.err, 2);
}

#include "inflate_kernels.h"  // Deflate: k_inflate, k_inflate_links

// Predictor 2: each sample adds the same component of the pixel to its left
// (modulo 2^bits, in the file's byte order for 16-bit samples).
__global__ void __launch_bounds__(256) k_unpredict(uint8_t *dst, int nrows, int rows_per_strip_buf, int rps, int h,
                                                    int per_plane, uint64_t stride, int w, int spp, int bits,
                                                    int big_endian) {
    const int r = blockIdx.x * 256 + threadIdx.x;  // global decoded row: strip * rps + row in strip
    if (r >= nrows) return;
    const int s = r / rows_per_strip_buf, y = r % rows_per_strip_buf;
    if ((s % per_plane) * rps + y >= h || y >= rps) return;
    const uint64_t rb = (uint64_t)w * spp * (bits >> 3);
    uint8_t *row = dst + (uint64_t)s * stride + (uint64_t)y * rb;
    if (bits == 8) {
        for (int i = spp; i < w * spp; i++) row[i] = (uint8_t)(row[i] + row[i - spp]);
    } else {
        auto rd = [&](int i) -> uint32_t {
            return big_endian ? ((uint32_t)row[2 * i] << 8) | row[2 * i + 1] : row[2 * i] | ((uint32_t)row[2 * i + 1] << 8);
        };
        for (int i = spp; i < w * spp; i++) {
            const uint32_t v = (rd(i) + rd(i - spp)) & 0xFFFFu;
            if (big_endian) { row[2 * i] = (uint8_t)(v >> 8); row[2 * i + 1] = (uint8_t)v; }
            else { row[2 * i] = (uint8_t)v; row[2 * i + 1] = (uint8_t)(v >> 8); }
        }
    }
}

// Tiled TIFF -> one row-major strip per plane: thread per pixel of a row.
// Tile t of plane p starts at base + (toff ? toff[t] : t * tstride).
__global__ void __launch_bounds__(256) k_untile(const uint8_t *base, const uint64_t *toff, uint64_t tstride, int w,
                                                 int h, int tw, int th, int across, int per_plane, int px_bytes,
                                                 uint8_t *out) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, p = blockIdx.z;
    if (x >= w) return;
    const int t = p * per_plane + (y / th) * across + x / tw;
    const uint8_t *src = base + (toff ? toff[t] : (uint64_t)t * tstride) +
                         ((uint64_t)(y % th) * tw + (x % tw)) * px_bytes;
    uint8_t *dst = out + (uint64_t)p * w * h * px_bytes + ((uint64_t)y * w + x) * px_bytes;
    for (int i = 0; i < px_bytes; i++) dst[i] = src[i];
}

bool GpuEncoder::unpack_strips(const void *d_src, const jp2hip_layout &lay, const UnitGrid &g, jp2hip_layout &out,
                               std::vector<uint64_t> &out_offs, const void **d_out, std::string &err,
                               bool untile) {
    HIPCHECK(hipSetDevice(device));
    const int ns = (int)g.needed;  // strips, or tiles
    const bool tiled = g.tiled;
    const int spp_row = lay.planar == 2 ? 1 : lay.components;
    const int px_bytes = spp_row * (lay.bits / 8);  // (0 below 8 bits: such tiles are not untiled here)
    const int unit_w = (int)g.unit_w, unit_h = (int)g.unit_h, planes = (int)g.planes, per_plane = (int)g.per_plane;
    const uint64_t row_bytes = g.row_bytes;
    if (lay.bits < 8 && ((tiled && untile) || lay.predictor == 2)) {
        err = "layout: samples below 8 bits are neither untiled nor un-differenced here";
        return false;
    }
    const uint64_t stride = (g.unit_bytes + 255) & ~255ull;
    const bool decode = lay.compression > 1;
    if (!ensure<uint64_t>(soff, (size_t)ns * 2, err) || !ensure<int>(this->err, 4, err)) return false;
    if (decode && !ensure<uint8_t>(stage, stride * ns, err)) return false;
    if (!h2d(soff.ptr, lay.strip_offsets, sizeof(uint64_t) * ns, err) ||
        !h2d((uint64_t *)soff.ptr + ns, lay.strip_bytes, sizeof(uint64_t) * ns, err))
        return false;
    HIPCHECK(hipMemsetAsync(this->err.ptr, 0, sizeof(int), stream));
    if (decode) {
        UnpackArgs ua;
        ua.src = (const uint8_t *)d_src;
        ua.off = (const uint64_t *)soff.ptr;
        ua.cnt = (const uint64_t *)soff.ptr + ns;
        ua.nstrips = ns;
        ua.per_plane = per_plane;
        ua.rps = lay.rows_per_strip;
        ua.h = lay.height;
        ua.row_bytes = row_bytes;
        ua.stride = stride;
        ua.unit_bytes = tiled ? g.unit_bytes : 0;
        ua.dst = (uint8_t *)stage.ptr;
        ua.only = nullptr;
        ua.lnk = nullptr;
        ua.err = (int *)this->err.ptr;
        if (lay.compression == 5) {  // segment-parallel (lzw.hip)
            std::vector<uint64_t> slice;
            const uint64_t segs = lzw_slices(lay.strip_bytes, ns, slice);
            if (!ensure<uint8_t>(lzwseg, lzw_scratch_bytes(ns, segs), err) ||
                !h2d(lzwseg.ptr, slice.data(), sizeof(uint64_t) * ns, err))
                return false;
            if (!launch_lzw(ua, segs, lzwseg.ptr, stream)) {
                err = std::string("LZW launch failed: ") + hipGetErrorString(hipGetLastError());
                return false;
            }
        }
        else if (lay.compression == 8 || lay.compression == 32946) {
            // decode to links (a strip per wave), then resolve the links
            // (every strip's bytes in parallel; k_inflate_links)
            if (!ensure<uint32_t>(inflnk, stride * ns, err)) return false;
            ua.lnk = (uint32_t *)inflnk.ptr;
            hipLaunchKernelGGL(k_inflate, dim3(ns), dim3(kInfLanes), 0, stream, ua);
            const dim3 grid((unsigned)((g.unit_bytes + kLinkChunk - 1) / kLinkChunk), (unsigned)ns);
            for (int r = 0; r <= kLinkDoublings; r++)
                hipLaunchKernelGGL(k_inflate_links, grid, dim3(256), 0, stream, ua, r == kLinkDoublings ? 1 : 0);
        }
        else hipLaunchKernelGGL(k_unpackbits, dim3(ns), dim3(64), 0, stream, ua);
        HIPCHECK(hipGetLastError());
        if (lay.predictor == 2) {  // per decoded row of a strip / of a tile
            const int nrows = ns * unit_h;
            hipLaunchKernelGGL(k_unpredict, dim3((nrows + 255) / 256), dim3(256), 0, stream, (uint8_t *)stage.ptr,
                               nrows, unit_h, unit_h, tiled ? unit_h : lay.height, tiled ? 1 : per_plane, stride,
                               unit_w, spp_row, lay.bits, lay.big_endian);
            HIPCHECK(hipGetLastError());
        }
    } else if (lay.predictor == 2) {
        err = "tiff: Predictor 2 on uncompressed data is not supported";
        return false;
    }
    const void *res = decode ? stage.ptr : d_src;
    out = lay;
    out_offs.resize(tiled && untile ? planes : ns);
    if (tiled && untile) {  // tiles -> one row-major strip per plane
        const uint64_t plane_bytes = (uint64_t)lay.width * lay.height * px_bytes;
        if (!ensure<uint8_t>(untiled, plane_bytes * planes, err)) return false;
        hipLaunchKernelGGL(k_untile, dim3((lay.width + 255) / 256, lay.height, planes), dim3(256), 0, stream,
                           (const uint8_t *)res, decode ? nullptr : (const uint64_t *)soff.ptr, stride, lay.width,
                           lay.height, lay.tile_width, lay.tile_height, (int)g.across, per_plane, px_bytes,
                           (uint8_t *)untiled.ptr);
        HIPCHECK(hipGetLastError());
        for (int p = 0; p < planes; p++) out_offs[p] = (uint64_t)p * plane_bytes;
        out.rows_per_strip = lay.height;
        out.nstrips = planes;
        out.tile_width = out.tile_height = 0;
        res = untiled.ptr;
    } else {
        for (int i = 0; i < ns; i++) out_offs[i] = (uint64_t)i * stride;
    }
    HIPCHECK(hipMemcpyAsync(h_tot + 4, this->err.ptr, sizeof(int), hipMemcpyDeviceToHost, stream));
    if (!host_wait(err)) return false;
    const int herr = *(const int *)(h_tot + 4);
    if (herr & 4) {
        err = "tiff: old-style (pre-TIFF 6.0, LSB-first) LZW strips are not supported";
        return false;
    }
    if (herr) {
        err = "tiff: corrupt compressed strip";
        return false;
    }
    out.strip_offsets = out_offs.data();
    out.compression = 1;
    out.predictor = 1;
    out.strip_bytes = nullptr;
    *d_out = res;
    return true;
}

}  // namespace jp2hip
