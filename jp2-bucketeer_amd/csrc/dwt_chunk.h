// dwt_chunk.h -- column chunks of a DWT level whose rows do not fit in LDS:
// which columns a workgroup stages, which it keeps, and where its outputs go.
// GPU-free (host and device): the kernels (dwt.hip, the CHUNK instances of
// k_dwt_l1 and k_dwt_band) and the CPU test (tests/host/test_dwt_chunk.cpp,
// under ASan / UBSan) share these functions.
//
// Chunk k of a row of W samples keeps the C columns [k C, k C + C), clipped to
// the row, and stages kDwtChunkHalo more on each side, clipped as well.  The
// horizontal lifting updates a sample from its two neighbours, 4 steps for
// 9/7 and 2 for 5/3, so a kept sample depends on at most 4 samples on each
// side: every one of them is staged, or lies beyond a true row end (0 or
// W - 1), where the symmetric extension reflects it onto a staged one.  The
// kept samples therefore see the operands, expressions and order of
// whole-row lifting, and come out bit-identical.  C is a multiple of 16, so a
// chunk starts on an even sample (parity is the row's), on a boundary of the
// 16-sample segments hlift_seg lifts, and its 8 + 8 de-interleaved outputs
// per segment stay 16-byte aligned wherever the whole row's are.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JP2HIP_HD __host__ __device__ __forceinline__
#else
#define JP2HIP_HD inline
#endif

namespace jp2hip {

constexpr int kDwtChunkHalo = 4;  // >= lifting steps (9/7: 4, 5/3: 2)
// kept columns per workgroup: level 1 with ingest, every component of a tile
// (k_dwt_l1<.., CHUNK>), and levels >= 2 (k_dwt_band<.., CHUNK>).  504 staged
// columns are two passes of a 256-thread workgroup.
constexpr int kL1ChunkW = 496;
constexpr int kBandChunkW = 496;
static_assert(kL1ChunkW % 16 == 0 && kBandChunkW % 16 == 0, "chunks start on 16-sample segment boundaries");

struct DwtChunk {
    int c0, c1;  // kept columns [c0, c1)
    int s0, s1;  // staged columns [s0, s1): the kept ones and the halo, inside the row
    int lo0, nlo;  // low-pass outputs lo0 .. lo0 + nlo - 1 of the row's ceil(W / 2)
    int hi0, nhi;  // high-pass outputs hi0 .. hi0 + nhi - 1 of its floor(W / 2), stored after the low ones
};

JP2HIP_HD constexpr int dwt_chunk_count(int W, int C) { return W > 0 ? (W + C - 1) / C : 0; }

// chunk k (0 <= k < dwt_chunk_count(W, C)) of a row of W samples
JP2HIP_HD DwtChunk dwt_chunk(int W, int C, int k) {
    DwtChunk c;
    c.c0 = k * C;
    c.c1 = c.c0 + C < W ? c.c0 + C : W;
    c.s0 = c.c0 - kDwtChunkHalo > 0 ? c.c0 - kDwtChunkHalo : 0;
    c.s1 = c.c1 + kDwtChunkHalo < W ? c.c1 + kDwtChunkHalo : W;
    c.lo0 = c.c0 >> 1;                 // c0 is even: sample c0 + 2 j -> low c0 / 2 + j
    c.nlo = (c.c1 - c.c0 + 1) >> 1;
    c.hi0 = c.c0 >> 1;                 // sample c0 + 2 j + 1 -> high c0 / 2 + j
    c.nhi = (c.c1 - c.c0) >> 1;
    return c;
}

// LDS words a staged row takes at most: the kept columns and both halos
JP2HIP_HD constexpr int dwt_chunk_staged(int C) { return C + 2 * kDwtChunkHalo; }

}  // namespace jp2hip
