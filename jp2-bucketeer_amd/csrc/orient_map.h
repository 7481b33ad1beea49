// orient_map.h -- TIFF Orientation (tag 274) as a pixel map: the size of the
// upright image, where each of its pixels lies in the stored one, and which
// stored rows a band of upright rows is made from.  GPU-free (host and
// device): k_orient (orient.hip), prepare_source, the tile-split and the CPU
// test (tests/host/test_orient_map.cpp, under ASan / UBSan) share this file.
//
// For a stored image a (h rows of w pixels) the upright image is
//   1 a              2 a[:, ::-1]      3 a[::-1, ::-1]              4 a[::-1]
//   5 a transposed   6 a turned 90 degrees clockwise
//   7 a[::-1, ::-1] transposed         8 a turned 90 degrees counter-clockwise
// so 5..8 swap width and height.  Every value is a choice of three bits:
// the axes swap, the stored x runs backwards, the stored y runs backwards.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JP2HIP_HD __host__ __device__ __forceinline__
#else
#define JP2HIP_HD inline
#endif

namespace jp2hip {

JP2HIP_HD constexpr bool orient_valid(int o) { return o >= 1 && o <= 8; }
JP2HIP_HD constexpr bool orient_swaps(int o) { return o >= 5; }
// the stored x falls while the upright coordinate it follows rises
JP2HIP_HD constexpr bool orient_flips_x(int o) { return o == 2 || o == 3 || o == 7 || o == 8; }
JP2HIP_HD constexpr bool orient_flips_y(int o) { return o == 3 || o == 4 || o == 6 || o == 7; }
// the value that takes the upright image back to the stored one
JP2HIP_HD constexpr int orient_inverse(int o) { return o == 6 ? 8 : (o == 8 ? 6 : o); }

// The upright image of a stored w x h one is ow x oh.
JP2HIP_HD void orient_size(int64_t w, int64_t h, int o, int64_t &ow, int64_t &oh) {
    ow = orient_swaps(o) ? h : w;
    oh = orient_swaps(o) ? w : h;
}

// Upright pixel (ux, uy) is stored pixel (x, y) of the w x h stored image.
JP2HIP_HD void orient_source(int o, int64_t w, int64_t h, int64_t ux, int64_t uy, int64_t &x, int64_t &y) {
    const int64_t fx = orient_swaps(o) ? uy : ux, fy = orient_swaps(o) ? ux : uy;
    x = orient_flips_x(o) ? w - 1 - fx : fx;
    y = orient_flips_y(o) ? h - 1 - fy : fy;
}

// The stored rows [s0, s1) that upright rows [row0, row1) are made from (the
// range clipped to the upright image; an empty one gives s0 = s1): the same
// rows, the mirrored range, or -- the axes swap, an upright row is a stored
// column -- every row.
JP2HIP_HD void orient_source_rows(int64_t h, int64_t w, int o, int64_t row0, int64_t row1, int64_t &s0, int64_t &s1) {
    const int64_t oh = orient_swaps(o) ? w : h;
    const int64_t r0 = row0 < 0 ? 0 : row0, r1 = row1 > oh ? oh : row1;
    if (r1 <= r0) {
        s0 = s1 = 0;
    } else if (orient_swaps(o)) {
        s0 = 0;
        s1 = h;
    } else if (orient_flips_y(o)) {
        s0 = h - r1;
        s1 = h - r0;
    } else {
        s0 = r0;
        s1 = r1;
    }
}

// The stored columns [c0, c1) those upright rows are made from when the axes
// swap (the transposing kernel's grid covers them and every stored row).
JP2HIP_HD void orient_source_cols(int64_t w, int o, int64_t row0, int64_t row1, int64_t &c0, int64_t &c1) {
    c0 = orient_flips_x(o) ? w - row1 : row0;
    c1 = orient_flips_x(o) ? w - row0 : row1;
}

}  // namespace jp2hip
