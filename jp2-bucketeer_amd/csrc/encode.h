// encode.h -- what the host sources behind the C ABI call in each other.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "jp2hip.h"

struct jp2hip_ctx;

namespace jp2hip {
struct UnitGrid;

// api.cpp: the pinned output pool (pinned_pool.h) and the clock of the stats
uint8_t *out_alloc(size_t n);
void out_free(void *p);
double now_ms();
// prepare_source.cpp
bool prepare_source(jp2hip_ctx *ctx, const UnitGrid &g, const void *&d_src, size_t src_len, const jp2hip_layout *&lay,
                    int row0, int row1, jp2hip_layout &ulay, std::vector<uint64_t> &uoffs, std::string &err,
                    int orient = 0);
// encode.cpp (the caller holds ctx->mu)
void default_recipe(jp2hip_recipe *r, int conversion);
jp2hip_recipe recipe_of(const jp2hip_recipe *recipe, int conversion);
// jp2hip_set_layer_slopes' thresholds: a NaN, a negative value and a sequence
// that increases are refused; with rc (the encode's recipe) also n other than
// rc->layers and, lossless, a last entry other than 0.  err names the entry.
bool check_layer_slopes(const double *slopes, int n, const jp2hip_recipe *rc, std::string &err);
// jp2hip_set_layer_rates' rates likewise: a NaN, an infinity, a negative value
// and a sequence that decreases (a last 0 after positive rates is the lossless
// top layer, no decrease) are refused; with rc also n other than rc->layers, a
// last entry other than 0 under rate_bpp <= 0 and a 0 entry under rate_bpp > 0.
bool check_layer_rates(const double *rates, int n, const jp2hip_recipe *rc, std::string &err);
// jp2hip_set_layer_psnr's targets (dB) under the rules of the rates: a NaN, an
// infinity, a negative value and a sequence that decreases (a last 0 is the
// lossless top layer) are refused; with rc also n other than rc->layers, a last
// entry other than 0 under rate_bpp <= 0 and a 0 entry under rate_bpp > 0.
bool check_layer_psnr(const double *psnr_db, int n, const jp2hip_recipe *rc, std::string &err);
// The quanta (psnr_quantum.h) each layer may leave in a width x height image
// of `components` samples of `bits` bits a pixel: floor(peak^2 N 2^-s /
// 10^(psnr / 10)), saturated at 2^62; a last entry of 0 (the lossless top
// layer) gives -1.  The one conversion from dB every encode route uses.
void layer_psnr_targets(int width, int height, int components, int bits, const double *psnr_db, int n,
                        int64_t *targets);
struct Plan;
// Whether an encode of this plan by PSNR targets is accepted: an upper bound
// on its hull segments' quanta (psnr_quantum.h) stays below 2^63.
bool quanta_fit(const Plan &plan);
// orient: the encode's source orientation, resolved (0 off, 1..8: TIFF
// Orientation; never JP2HIP_ORIENT_TIFF -- the callers that parse a TIFF read
// its tag, source_orientation())
int source_orientation(const jp2hip_ctx *ctx, const uint8_t *tiff, size_t len);
int encode_core(jp2hip_ctx *ctx, const void *d_src, size_t src_len, const jp2hip_layout *lay, int conversion,
                const jp2hip_recipe *recipe, uint8_t **out, size_t *out_len, jp2hip_stats *stats, double t_start,
                double h2d_ms, int orient);
int encode_split_core(jp2hip_ctx *ctx, const void *d_src, size_t src_len, const jp2hip_layout *lay, int conversion,
                      const jp2hip_recipe *recipe, const jp2hip_split *sp, uint8_t **out, size_t *out_len,
                      uint64_t *file_offset, uint64_t *file_len, jp2hip_stats *stats, double t_start, int orient);
// split_host.cpp
bool wants_split(const jp2hip_ctx *ctx, const jp2hip_layout &lay);
int encode_split_host(jp2hip_ctx *ctx, const uint8_t *file, size_t flen, const jp2hip_layout &lay, int conversion,
                      const jp2hip_recipe *recipe, int fd, uint8_t **out, size_t *out_len, jp2hip_stats *stats,
                      double t0, int orient);

}  // namespace jp2hip
