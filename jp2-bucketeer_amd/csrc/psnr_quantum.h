// psnr_quantum.h -- the integer unit of distortion that quality layers by
// target PSNR (jp2hip_set_layer_psnr) are selected in.  GPU-free (host and
// device): k_hull and k_select (pcrd.hip), the tile-split's segment list, the
// exported jp2hip_distortion_quantum / jp2hip_layer_psnr_targets (api.cpp) and
// the CPU test (tests/host/test_psnr_quantum.cpp, under ASan / UBSan) share
// this file.
//
// A selection must be exact and the same on every route (one GPU, a
// tile-split over any number of ranks), so distortion is not summed in
// doubles, whose sum depends on the order: every hull segment contributes an
// integer number of quanta, and integers add the same in any order.
//
// The quantum is 2^s squared sample levels with s = 2 (bits - 8) - 8: 1/256 of
// one squared level of an 8-bit image, scaled with the square of the sample
// range so that an image has about the same number of quanta at every depth.
// A segment of distortion decrease dd (HullPt::d of its end less that of its
// start; tier-1's integer unit) in a block of PCRD weight `weight` gives
//     q = floor((weight * (double)dd) * 2^-s + 0.5), saturated at 2^63 - 1,
// and 0 for a product that is not positive.  (double)dd and the product round
// to nearest; the scale is an exact power of two, so the only other rounding
// is the 0.5's, where the value is past 2^52 and has no fraction to round --
// numpy's float64 gives the same bits.  The library is built with
// -ffp-contract=off: no multiply-add fuses the steps on the device.
#pragma once

#include <cstdint>
#include <cstring>

#ifndef JP2HIP_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define JP2HIP_HD __host__ __device__ __forceinline__
#else
#define JP2HIP_HD inline
#endif
#endif

namespace jp2hip {

// s above; bits = 1 .. 16 gives -22 .. 8
JP2HIP_HD constexpr int quantum_shift(int bits) { return 2 * (bits - 8) - 8; }

// 2^e as a double, e within the normal range (built from the exponent field:
// no libm on either side)
JP2HIP_HD double quantum_pow2(int e) {
    const uint64_t u = (uint64_t)(1023 + e) << 52;
    double d;
#if defined(__HIP_DEVICE_COMPILE__)
    d = __longlong_as_double((long long)u);
#else
    std::memcpy(&d, &u, 8);
#endif
    return d;
}

JP2HIP_HD int64_t distortion_quantum(double weight, int64_t dd, int bits) {
    const double p = weight * (double)dd;
    if (!(p > 0.0)) return 0;  // (also a NaN)
    const double v = p * quantum_pow2(-quantum_shift(bits));
    if (v >= 9223372036854775808.0) return INT64_MAX;
    const double r = v + 0.5;
    // floor of a non-negative double below 2^63 + 1: the conversion truncates
    return r >= 9223372036854775808.0 ? INT64_MAX : (int64_t)r;
}

// Overflow.  An encode adds the quanta of every hull segment of an image (the
// histogram of k_hull, the suffix sums of k_select, the tile-split's inclusive
// sums, an all-reduce over ranks), so their total must stay below 2^63.  No
// bound on it follows from the geometry alone (the weights grow with the
// levels), so the encode bounds it for its own plan and refuses one it cannot
// vouch for (quanta_fit, encode.cpp): a code-block of w x h samples and Mb
// magnitude bit-planes has at most 3 Mb - 2 segments, and the distortion
// decreases of all its passes together stay below 8 w h 4^Mb (t1.hip counts
// 4x the squared error in quantiser steps: a sample of magnitude v < 2^Mb can
// gain at most its own 4 v^2 over its passes, plus the irreversible path's
// 6 * 2^p <= 6 v where it becomes significant), so the block's quanta are
// below weight * 8 w h 4^Mb * 2^-s + (3 Mb - 2), a half for every segment's
// rounding included.  The bound's sum over the blocks must be below 2^63.
constexpr double kQuantaLimit = 9223372036854775808.0;  // 2^63
// (a layer's target saturates far below: it is compared with sums under the limit)
constexpr int64_t kQuantaTargetMax = (int64_t)1 << 62;

}  // namespace jp2hip
