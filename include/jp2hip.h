/*
 * jp2hip.h -- C ABI of libjp2hip, the MI355X (gfx950) JPEG 2000 encoder that
 * replaces `kdu_compress` behind Bucketeer's converter plug-in API.
 *
 * Reference interfaces this ABI stands in for (paths relative to
 * src/main/java/edu/ucla/library/bucketeer/ in UCLALibrary/jp2-bucketeer):
 *
 *   converters/Converter.java:22
 *       File convert(String aID, File aTIFF, Conversion aConversion)
 *           -> jp2hip_encode_file(): TIFF path in, JPX path out, blocking,
 *              every failure reported as rc < 0 + jp2hip_last_error()
 *              (the Java side turns that into IOException, like
 *              AbstractConverter.java:33-35 does for a non-zero exit).
 *   converters/Conversion.java:8-10          enum {LOSSY, LOSSLESS}
 *           -> JP2HIP_LOSSY = 0, JP2HIP_LOSSLESS = 1 (same ordinals).
 *   converters/KakaduConverter.java:38-44    BASE_OPTIONS + LOSSLESS_OPTIONS /
 *                                            LOSSY_OPTION (the kdu recipe)
 *           -> jp2hip_recipe / jp2hip_recipe_init().
 *   converters/KakaduConverter.java:61-71    fork/exec of kdu_compress
 *           -> in-process call; no child process.
 *   converters/ConverterFactory.java:86-103  checkSystemKakadu() probe
 *           -> jp2hip_probe() (a device with gfx950 is visible).
 *
 * All pointers are plain host pointers unless the name says d_ (device).
 * Paths are UTF-8 bytes.  Calls on one context are serialised internally;
 * different contexts (one per GPU) run concurrently.
 */
#ifndef JP2HIP_H
#define JP2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JP2HIP_LOSSY 0    /* Conversion.LOSSY    (Conversion.java:9)  */
#define JP2HIP_LOSSLESS 1 /* Conversion.LOSSLESS (Conversion.java:9)  */

#define JP2HIP_FORMAT_J2K 0 /* raw codestream                          */
#define JP2HIP_FORMAT_JP2 1
#define JP2HIP_FORMAT_JPX 2 /* what a ".jpx" output name asks Kakadu for */

/* jp2hip_recipe.progression: the packet order inside a tile (SGcod of COD,
 * ISO/IEC 15444-1 Table A.16).  L layer, R resolution, C component, P position. */
#define JP2HIP_ORDER_LRCP 0
#define JP2HIP_ORDER_RLCP 1
#define JP2HIP_ORDER_RPCL 2 /* the Bucketeer recipe's, and jp2hip_recipe_init's */
#define JP2HIP_ORDER_PCRL 3
#define JP2HIP_ORDER_CPRL 4

typedef struct jp2hip_ctx jp2hip_ctx;

typedef struct jp2hip_config {
    int32_t device;       /* HIP device ordinal                                */
    int32_t host_threads; /* tier-2 worker threads (<=0: min(16, hw threads))  */
    int32_t profile;      /* 1: record per-stage HIP event times in stats      */
    int32_t reserved;
} jp2hip_config;

/* The kdu_compress recipe (KakaduConverter.java:38-44), field by field. */
typedef struct jp2hip_recipe {
    int32_t levels;          /* Clevels=6                                      */
    int32_t layers;          /* Clayers=6                                      */
    int32_t tile_w, tile_h;  /* Stiles={512,512}: multiples of 2^levels, each  */
                             /* at most 32768 (so a tile-component has at most */
                             /* 2^30 samples), at most 65535 tiles.  Both 0:   */
                             /* no Stiles, one tile for the whole image -- the */
                             /* smallest multiples of 2^levels not below width */
                             /* and height, written to SIZ as they are; one of */
                             /* them 0, or a negative one, is refused.  A tile */
                             /* is also refused (the message names the field)  */
                             /* where its packets outgrow a tile-part header:  */
                             /* 256 PLT segments (Zplt), 2^32 - 1 bytes (Psot) */
    int32_t cblk_w_log2;     /* Cblk={64,64}                                   */
    int32_t cblk_h_log2;
    int32_t nprecincts;      /* Cprecincts={256,256},{256,256},{128,128}:     */
    int32_t prec_w_log2[16]; /*   highest resolution first, last one repeats;  */
                             /*   0..16 entries (0: one precinct), each 0..15, */
                             /*   0 only for the lowest resolution             */
    int32_t prec_h_log2[16];
    int32_t progression;     /* Corder=RPCL: JP2HIP_ORDER_* (the COD value);   */
                             /* the order moves the packets inside a tile,     */
                             /* their Nsop and the PLT, never a packet's bytes */
    int32_t sop, eph;        /* Cuse_sop=yes Cuse_eph=yes                      */
    int32_t plt;             /* ORGgen_plt=yes                                 */
    int32_t tparts_r;        /* ORGtparts=R: a tile-part per resolution; only  */
                             /* with a resolution-major order (RLCP, RPCL),    */
                             /* refused with LRCP, PCRL, CPRL; 0: one per tile */
    int32_t guard_bits;      /* 1 (0..7: three bits of Sqcd)                   */
    int32_t reversible;      /* Creversible=yes -> 5/3 + RCT, else 9/7 + ICT   */
    int32_t mct;             /* colour transform on components 0..2            */
    double qstep;            /* irreversible base step (Kakadu Qstep=1/256):   */
                             /* finite, > 0, no band over 30 bit-planes        */
    double rate_bpp;         /* "-rate 3"; <= 0 means "-rate -" (all passes)   */
    int32_t format;          /* JP2HIP_FORMAT_*                                */
    int32_t comment;         /* emit Kakadu-style COM markers: a version       */
                             /* string and "Kdu-Layer-Info" (layer slopes and  */
                             /* bytes, test.jpx's second COM)                  */
    int32_t slope_skip;      /* rate-driven (rate_bpp > 0) only: do not code   */
                             /* bit-planes whose predicted slope lies far      */
                             /* below the rate target's, as kdu_compress's     */
                             /* block coder does under "-rate"; 0 = code all   */
    int32_t flush_period;    /* -flush_period 1024 (KakaduConverter.java:40):  */
                             /* tile-parts go out per stripe of tile rows that */
                             /* completes a flush -- resolution 0 of every     */
                             /* tile in the stripe, then resolution 1, ...     */
                             /* (test.jpx's order); <= 0: tile after tile      */
} jp2hip_recipe;

/* Code-stream organisation that is no part of the coding recipe (Kakadu's ORG
 * cluster; ORGgen_plt / ORGtparts keep living in the recipe). All zero = as before. */
typedef struct jp2hip_organisation {
    int32_t tlm;          /* ORGgen_tlm: 1 = TLM marker segments in the main header */
    int32_t reserved[3];  /* 0 */
} jp2hip_organisation;

#define JP2HIP_PHOTO_DEFAULT 0       /* BlackIsZero grey / RGB, by component count */
#define JP2HIP_PHOTO_WHITE_IS_ZERO 1 /* grey, 0 = white (bits 1, 2, 4 only)        */
#define JP2HIP_PHOTO_PALETTE 2       /* indices into `colormap` (bits 1, 2, 4, 8)  */

/* Where the samples live inside a source buffer (a baseline TIFF's strips),
 * and what the source says about them (extra_samples .. icc_bytes: carried
 * into the JP2 / JPX file header, DESIGN.md "Source metadata"; all zero =
 * a source that states nothing).
 * components and bits describe the source.  Samples of 1, 2 or 4 bits (one
 * component; rows packed MSB-first unless fill_order is 2, each row -- of the
 * image for strips, of a tile for tiles -- starting on a byte boundary) and
 * palette indices are expanded to 8-bit samples in HBM before ingest
 * (DESIGN.md "S1b sample expansion"): value v of `bits` bits becomes
 * v * 255 / (2^bits - 1), WhiteIsZero then 255 minus that, and a palette
 * index becomes three components (R, G, B).  jp2hip_encoded_format() names
 * what the code-stream carries.  The fields from `photometric` on were
 * appended: all zero means a layout as it was before them. */
typedef struct jp2hip_layout {
    int32_t width, height, components, bits; /* bits 8 or 16, unsigned; also*/
                                             /* 1, 2, 4 (one component)     */
    int32_t planar;                          /* 1 chunky, 2 planar          */
    int32_t big_endian;                      /* 16-bit sample byte order    */
    int32_t rows_per_strip;
    int32_t nstrips;                         /* entries in strip_offsets    */
    const uint64_t *strip_offsets;           /* byte offset of each strip   */
    int32_t compression;                     /* TIFF Compression: 1 (or 0)  */
                                             /* none, 5 LZW, 8 / 32946      */
                                             /* Deflate, 32773 PackBits     */
    int32_t predictor;                       /* TIFF Predictor: 1 none,     */
                                             /* 2 horizontal differencing   */
    const uint64_t *strip_bytes;             /* compressed size per strip   */
                                             /* (compression > 1)           */
    int32_t tile_width, tile_height;         /* tiled TIFF (0: strips): the */
                                             /* "strips" above are then the */
                                             /* tiles, row-major per plane  */
    int32_t extra_samples;  /* 0: not stated (last of 2 or 4 channels is opacity,
                               as before); else TIFF ExtraSamples value + 1:
                               1 unspecified (no cdef box), 2 associated
                               (premultiplied opacity), 3 unassociated opacity */
    int32_t res_unit;       /* 0, 1: no resolution; 2 inch; 3 centimetre         */
    uint32_t xres_num, xres_den, yres_num, yres_den; /* X/YResolution rationals:
                               a res box is written when all four are non-zero
                               and res_unit is 2 or 3                            */
    const uint8_t *icc;     /* host pointer to the profile bytes (NULL: none);
                               jp2hip_tiff_layout points it into `tiff`; read
                               during the encode call only                       */
    uint64_t icc_bytes;
    int32_t photometric;    /* JP2HIP_PHOTO_*                                    */
    int32_t fill_order;     /* TIFF FillOrder for bits < 8: 0, 1 the first pixel
                               of a byte is in its high bits; 2 in its low bits  */
    const uint8_t *colormap; /* JP2HIP_PHOTO_PALETTE: the ColorMap tag's data as
                               the file holds it -- 3 * 2^bits 16-bit values in
                               the byte order `big_endian` names, every red, then
                               every green, then every blue; a component is the
                               entry >> 8, or the entry itself when no entry of
                               the map exceeds 255.  A host pointer like `icc`:
                               jp2hip_tiff_layout points it into `tiff`; read
                               during the encode call only                       */
    uint64_t colormap_entries; /* 3 * 2^bits                                     */
} jp2hip_layout;

/* Stage times (ingest_ms .. t2_ms, t1_cm_ms, t1_mq_ms) come from HIP events
 * and are filled only for a context created with jp2hip_config.profile = 1
 * (0 otherwise); total_ms, h2d_ms and the counts are always filled. */
typedef struct jp2hip_stats {
    double total_ms;      /* host wall time of the call                       */
    double h2d_ms;        /* source upload (encode_file / encode_tiff only)   */
    double ingest_ms;     /* sample expansion (k_expand: sub-byte / palette   */
                          /* sources only) and orientation (k_orient: only    */
                          /* with one set); the strip gather itself is part   */
                          /* of dwt_ms (fused into the first DWT level)       */
    double dwt_ms;        /* all DWT kernels                                  */
    double quant_ms;      /* quantisation + bit-plane kernel                  */
    double t1_ms;         /* EBCOT tier-1 kernels                             */
    double pcrd_ms;       /* hull + threshold selection kernels               */
    double d2h_ms;        /* metadata + compressed bytes download             */
    double t2_ms;         /* tier-2 on the device: packet headers, tile-part  */
                          /* sizing and code-stream emission                  */
    int64_t codeblocks;
    int64_t coded_passes;
    int64_t t1_bytes;     /* MQ bytes produced by tier-1 (before truncation)  */
    int64_t out_bytes;
    int32_t rate_iterations;
    int32_t host_waits;   /* times the host blocked on the GPU during the encode */
    double t1_cm_ms;      /* tier-1 context-modelling kernel (part of t1_ms)  */
    double t1_mq_ms;      /* tier-1 MQ-coder kernel (part of t1_ms)           */
    int64_t mq_decisions; /* MQ-coded decisions (one decision-stream byte each) */
    int64_t stream_pool_bytes; /* tier-1 decision-stream pool held by the context */
    int64_t stream_need_bytes; /* ... of which this encode's coded planes took    */
    int32_t pool_grows;   /* encodes repeated because the pool was short (0..2) */
    int32_t reused;       /* what this encode found in place on its context     */
                          /* (JP2HIP_REUSED_*); it records the branches taken   */
                          /* and steers nothing                                  */
} jp2hip_stats;

/* jp2hip_stats.reused, a bit set */
#define JP2HIP_REUSED_PLAN 1         /* the plan came from the context's cache          */
#define JP2HIP_REUSED_FRONT_TABLES 2 /* the plan's tables were resident (block table,   */
                                     /* weights, tile-component sizes, group table)     */
#define JP2HIP_REUSED_T2_TABLES 4    /* the tier-2 tables were resident                 */
#define JP2HIP_REUSED_STRIPS 8       /* the strip offsets were not uploaded again       */
#define JP2HIP_AFTER_TRIM 16         /* the previous encode on this context ended by    */
                                     /* releasing its device buffers                    */
#define JP2HIP_AFTER_FAILURE 32      /* the previous call on this context failed after  */
                                     /* its encode had begun                            */

const char *jp2hip_version(void);

/* Thread-local message for the last failing call on this thread. */
const char *jp2hip_last_error(void);

/* 1 if a gfx950 device is usable (ConverterFactory.checkSystemKakadu analogue). */
int jp2hip_probe(void);

/* Number of visible HIP devices that are gfx950 (0 if none). */
int jp2hip_device_count(void);

/* The HIP ordinals of the visible gfx950 devices (what jp2hip_config.device
 * takes), at most `max` of them written to `ordinals`; returns how many there
 * are.  A converter spreads its contexts over these, not over 0..n-1 (a
 * non-gfx950 device may hold a low ordinal). */
int jp2hip_device_ordinals(int32_t *ordinals, int32_t max);

/* "" when the process environment suits the contexts alive in it, else
 * what to change: GPU_MAX_HW_QUEUES below the live context count (contexts
 * sharing a hardware queue run their kernels one after another).  It must
 * be set before the library loads; a converter logs this once after
 * creating its contexts. */
const char *jp2hip_env_check(void);

/* Fill the Bucketeer recipe for JP2HIP_LOSSY / JP2HIP_LOSSLESS. */
void jp2hip_recipe_init(jp2hip_recipe *recipe, int conversion);

int jp2hip_create(jp2hip_ctx **out, const jp2hip_config *cfg);
void jp2hip_destroy(jp2hip_ctx *ctx);

/* Device memory (bytes) held by a context's buffers, its tile-split members'
 * included.  Buffers grow to what the largest recent image needed. */
int64_t jp2hip_device_bytes(jp2hip_ctx *ctx);

/* A context's device-memory policy, its tile-split members' too.
 * soft: bytes it may keep between encodes; an encode that leaves it above
 *   releases every buffer at its end (<= 0, the default: relative to the
 *   context's usual image -- it releases when it holds more than twice the
 *   larger of the median of what its last 8 encodes needed and what the
 *   encode before this one needed, plus 256 MiB, so one outsized master
 *   does not pin HBM for the context's life, a steady run of large masters
 *   keeps its buffers, and a lasting change to larger images costs one
 *   release).
 * hard: bytes no encode may pass; an image that needs more fails with
 *   rc < 0 and a message (never a fault), and the context stays usable
 *   (<= 0: no limit but the device's).
 * When the device itself runs out of memory, the allocating encode takes
 * back the buffers of idle contexts of the same device and waits (up to
 * 30 s) for busy ones to become idle before it fails.
 * Returns 0, or < 0 for a null context. */
int jp2hip_set_memory_limits(jp2hip_ctx *ctx, int64_t soft, int64_t hard);

/* The organisation of every later encode on ctx, its tile-split peers included
 * (peers added later inherit it).  NULL = all zero.  With tlm = 1 the main
 * header ends in TLM marker segments (ISO/IEC 15444-1 A.7.1; Stlm 0x60: 16-bit
 * Ttlm, 32-bit Ptlm) that list every tile-part's tile index and length in the
 * order the tile-parts lie in the file, so a reader finds any tile-part from
 * one read of the header; their T = 6 * tile-parts + 6 * segments bytes count
 * in the jp2c box length, stats.out_bytes, a split's file_len / file_offset
 * and Kdu-Layer-Info's L(bytes).  A rate-driven encode with a TLM is the
 * encode without one whose byte target is T lower (floored at 0): the TLM is
 * part of the code-stream the target bounds.  A tile-split over a caller's
 * callback is collective in the organisation as it is in the recipe: every
 * rank sets the same one.  Not to be called while ctx is encoding.  Returns
 * 0, or < 0 with a message that names the field (tlm other than 0 / 1,
 * reserved non-zero). */
int jp2hip_set_organisation(jp2hip_ctx *ctx, const jp2hip_organisation *org);

/* Tile-part divisions besides the recipe's (Kakadu's ORGtparts takes any
 * subset of R|L|C; R stays recipe.tparts_r). */
#define JP2HIP_TPARTS_L 2 /* a new tile-part where the layer changes     */
#define JP2HIP_TPARTS_C 4 /* a new tile-part where the component changes */

/* The tile-part divisions of every later encode on ctx, its tile-split peers
 * included (peers added later inherit them): letters = 0, JP2HIP_TPARTS_L,
 * JP2HIP_TPARTS_C or both; 0 restores the output without them.  A tile sends
 * its packets in the recipe's progression order (jp2hip_packet_sequence), and
 * a new tile-part starts before every packet that differs from the one before
 * it in a flagged index: resolution (R, when recipe.tparts_r is set -- still
 * RLCP and RPCL only), layer (L), component (C).  Each tile-part has its own
 * SOT (TPsot 0, 1, ...; TNsot = the tile's count on its last tile-part, else
 * 0), PLT (when recipe.plt is set) and SOD; no packet byte or Nsop changes.
 * In the file, per -flush_period stripe, part 0 of every tile of the stripe
 * comes first, then part 1, ...: with LRCP and L a stripe holds layer 0 of
 * all its tiles, then layer 1.  Letters that cut nowhere (L with one layer)
 * give the file without them, byte for byte.  An encode whose divisions give
 * a tile more than 255 tile-parts (TNsot is 8 bits) is refused with a message
 * that names the tile, the count and the letters.
 * A rate-driven encode with letters is the encode without them whose byte
 * target is E lower (floored at 0, on top of the TLM's T), E = (14 + 5 * plt)
 * * (tile-parts with the letters - tile-parts without): the headers of the
 * added tile-parts are part of the code-stream the target bounds.  That
 * equivalence is exact where every PLT, divided or not, is one marker
 * segment, which holds when no undivided tile-part has more than 13 106
 * packets (5 bytes * 13 106 <= 65 532); beyond that the file is still a valid
 * code-stream, but its rate-driven packets are not claimed to be those of the
 * encode at the lower target.  Lossless encodes select as without letters.
 * Kdu-Layer-Info's L(bytes) and stats.out_bytes count the real headers.
 * Collective over a caller's callback, like the recipe: every rank sets the
 * same letters.  Not to be called while ctx is encoding.  Returns 0, or < 0
 * with a message: for bit 1 (R) one that points at recipe.tparts_r, for any
 * other bit one that names it. */
int jp2hip_set_tile_part_divisions(jp2hip_ctx *ctx, int32_t letters);

/* Host-only, exported for tests (like jp2hip_packet_sequence): the tile-parts
 * of tile `tile` of a width x height image under `recipe` and `letters` --
 * returns their count and writes the place in the tile's packet sequence at
 * which each starts (first[0] = 0; the first min(count, cap) of them).
 * Returns < 0 with a message for anything the encodes refuse (the recipe, the
 * letters, more than 255 tile-parts in a tile, a tile outside the image). */
int64_t jp2hip_tile_parts(int32_t width, int32_t height, int32_t components, int32_t bits,
                          const jp2hip_recipe *recipe, int32_t letters, int32_t tile, uint32_t *first,
                          int64_t cap);

/* Host-only, exported for tests (like jp2hip_packet_sequence): the TLM marker
 * segments for n tile-parts in file order -- per segment FF55, Ltlm = 4 + 6 k,
 * Ztlm 0, 1, ..., Stlm 0x60, then k <= 10921 pairs (tiles[i], lengths[i]),
 * big-endian.  Returns their byte count and writes them when cap suffices;
 * < 0 on a null argument or more tile-parts than 256 segments hold. */
int64_t jp2hip_tlm_segments(const uint16_t *tiles, const uint32_t *lengths, int64_t n,
                            uint8_t *dst, size_t cap);

/* Source orientation: TIFF tag 274 (Orientation), what kdu_compress has
 * -rotate for.  JP2 has no orientation field that image servers honour, so an
 * encode that applies the tag writes the upright pixels. */
#define JP2HIP_ORIENT_OFF 0  /* the default: the rows as they are stored, whatever the tag says */
                             /* 1 .. 8: that TIFF Orientation (1: the stored image is upright)  */
#define JP2HIP_ORIENT_TIFF 9 /* the file's own tag 274                                          */

/* The orientation every later encode on ctx applies to its source, its
 * tile-split peers included (peers added later inherit it).  For a stored
 * image a of h rows and w columns the upright image is, in numpy's terms,
 *   1 a              2 a[:, ::-1]      3 a[::-1, ::-1]      4 a[::-1]
 *   5 a.swapaxes(0, 1)                 6 rot90(a, -1)
 *   7 a[::-1, ::-1].swapaxes(0, 1)     8 rot90(a, 1)
 * (5 .. 8: h columns and w rows); pixels move whole, a 16-bit sample keeps
 * its byte order and a pixel its component order.  The file is the one an
 * encode with JP2HIP_ORIENT_OFF gives for the uncompressed TIFF of the upright
 * pixels with the same metadata, byte for byte, on every route and with every
 * setting: for 5 .. 8 the tiles, SIZ, ihdr, the rate targets and the plan
 * cache's key take the upright width and height, and the res box has X and Y
 * resolution exchanged; colr and cdef stay.  The source is decoded and
 * expanded as always and turned last, on the GPU (DESIGN.md "S1c
 * orientation"), into a copy that counts in jp2hip_device_bytes and against
 * the memory limits; JP2HIP_ORIENT_OFF and 1 launch nothing.
 * JP2HIP_ORIENT_TIFF is resolved where a TIFF is parsed -- jp2hip_encode_file,
 * jp2hip_encode_tiff, the batch queue -- to the file's tag (absent or
 * malformed: 1).  jp2hip_encode_device and jp2hip_encode_device_split take a
 * caller's layout, which names no tag: under JP2HIP_ORIENT_TIFF they are
 * refused with a message that names this function and
 * jp2hip_tiff_orientation, and the context stays usable.
 * Not part of the recipe.  Collective over a caller's callback, like the
 * organisation: every rank sets the same value.  Not to be called while ctx
 * is encoding.  Returns 0, or < 0 with a message that names the value. */
int jp2hip_set_source_orientation(jp2hip_ctx *ctx, int32_t o);

/* Host-only: tag 274 of a TIFF (classic or BigTIFF, either byte order) when it
 * is one SHORT in 1 .. 8; 1 when the tag is absent or malformed (a bad
 * metadata tag never fails a parse); < 0 only when `tiff` is no TIFF at all.
 * Only the first IFD is read (no EXIF sub-IFD). */
int32_t jp2hip_tiff_orientation(const uint8_t *tiff, size_t len);

/* Host-only: width and height of the upright image of a stored w x h one
 * (o = 0 .. 8; exchanged for 5 .. 8).  < 0 for another o or a null pointer. */
int jp2hip_oriented_size(int32_t w, int32_t h, int32_t o, int32_t *ow, int32_t *oh);

/* Host-only, exported for tests (the tile-split uses it): the stored rows
 * [*src_row0, *src_row1) that rows [row0, row1) of the upright image are made
 * from -- the same rows for o = 0, 1, 2; the mirrored range height - row1 ..
 * height - row0 for 3 and 4; every row, 0 .. height, for 5 .. 8.  The range
 * is clipped to the upright image; an empty one gives an empty one.  < 0 for
 * another o, a geometry that is not positive or a null pointer. */
int jp2hip_orientation_source_rows(int32_t height, int32_t width, int32_t o, int32_t row0, int32_t row1,
                                   int32_t *src_row0, int32_t *src_row1);

/* Fixed-slope quality layers (Kakadu's -slope s1,s2,...): with n =
 * recipe.layers thresholds set, layer 0 first, an encode has no byte target and
 * no rate loop -- layer l holds, per code-block, the passes of the block's
 * convex hull whose distortion-length slope is >= slopes[l].  A threshold is a
 * slope in the library's own units: the double whose bit pattern is the PCRD
 * slope key (squared error in sample units, weighted by the band's synthesis
 * gain, per byte); Kdu-Layer-Info prints log2 of it less 2 * bits
 * (jp2hip_slope_to_log2).  +0.0 takes the whole hull, +inf takes nothing.
 * NULL / n = 0 turns it off (the encodes are again rate-driven or lossless).
 *   - With slopes set, recipe.rate_bpp > 0 only selects the irreversible
 *     recipe's meaning of "not lossless": its value is no target.  With
 *     rate_bpp <= 0 the last layer takes every coded pass, as without slopes,
 *     and its threshold must be 0.
 *   - recipe.slope_skip is ignored: every bit-plane is coded.
 *   - stats.rate_iterations = 0; the TLM's T and the tile-part divisions' E
 *     lower nothing, no target exists.
 *   - The Kdu-Layer-Info lines print the given thresholds.
 *   - The slopes are no part of the plan cache's key.
 *   - Over a caller's callback a tile-split is collective in the slopes as it
 *     is in the organisation: every rank sets the same ones (peers of
 *     jp2hip_split_peers get them here and inherit them when added later).
 * Refused, with a message that names the entry: a NaN, a negative value, a
 * sequence that increases anywhere, n outside 0..32; at the encode, n other
 * than the recipe's layers and, with rate_bpp <= 0, a last entry other than 0
 * (the context stays usable).  Not to be called while ctx is encoding. */
int jp2hip_set_layer_slopes(jp2hip_ctx *ctx, const double *slopes, int32_t n);

/* Host-only, for tests and callers: the checks above on their own -- those of
 * the encode too when `recipe` is given.  Returns 0, or < 0 with a message
 * that names the entry. */
int jp2hip_check_layer_slopes(const double *slopes, int32_t n, const jp2hip_recipe *recipe);

/* Explicit per-layer rates (Kakadu's -rate r1,r2,..., which lists the highest
 * rate first; here layer 0 comes first): with n = recipe.layers rates set,
 * rates_bpp[l] bounds the code-stream through layer l -- main header, TLM and
 * tile-part headers included, as the single rate bounds the file's -- at
 * floor(rates_bpp[l] * width * height / 8) bytes.  The rate loop steers every
 * layer, not the last one: each has a byte budget of its own, lowered while
 * the layer is over its target (DESIGN.md 4 states the rule; budgets only ever
 * fall, so a layer may end below its target).  NULL / n = 0 turns it off.
 *   - recipe.rate_bpp is no target.  > 0 only selects the irreversible recipe's
 *     meaning of "not lossless", and every rate must be > 0.  With rate_bpp <= 0
 *     the last layer takes every coded pass and its rate must be 0: Kakadu's
 *     "-rate -,r2,...", a lossless file whose lower layers have named sizes.
 *   - recipe.slope_skip is honoured as for a single rate, against the top
 *     layer's target; with a lossless top layer it is off.
 *   - stats.rate_iterations counts the loop's iterations (at most 8).  With
 *     one layer the encode is the one recipe.rate_bpp = rates_bpp[0] gives.
 *   - A lossless recipe's plan has one rate-control group while rates are set
 *     (a byte target is the whole image's), not a group per -flush_period
 *     stripe; the plan cache's key holds that, not the rates.
 *   - Rates and fixed-slope layers exclude each other: setting one while the
 *     other is set is refused.
 *   - Collective like the slopes: peers of jp2hip_split_peers get the rates
 *     here and inherit them when added later; over a caller's callback every
 *     rank sets the same rates.
 * Refused, with a message that names the entry (or the other setter): a NaN,
 * an infinity, a negative value, a sequence that decreases anywhere (a last 0
 * is the lossless top layer, no decrease), n outside 0..32; at the encode, n
 * other than the recipe's layers, with rate_bpp <= 0 a last entry other than
 * 0, with rate_bpp > 0 an entry of 0 (the context stays usable).  Not to be
 * called while ctx is encoding. */
int jp2hip_set_layer_rates(jp2hip_ctx *ctx, const double *rates_bpp, int32_t n);

/* Host-only: the checks above on their own -- those of the encode too when
 * `recipe` is given.  Returns 0, or < 0 with a message that names the entry. */
int jp2hip_check_layer_rates(const double *rates_bpp, int32_t n, const jp2hip_recipe *recipe);

/* Host-only, exported for tests: one step of the loop above, the text the
 * device and the tile-split's host loop run, after iteration `it` (0..7) sized
 * the code-stream.  The code-stream through layer l is fixed + part_bytes less
 * layer_bytes[m] of the layers m > l; targets[l] < 0: the layer has no target
 * (a lossless top layer, whose budget INT64_MAX stays).  Returns 1: halt (every
 * targeted layer fits, or it = 7), budgets untouched; 0: the budgets of the
 * layers that are over are lowered by (over << it) + (over >> 4) + 64, floored
 * at 0, and clamped so that they never decrease with l; < 0: a bad argument. */
int jp2hip_layer_rate_step(int32_t layers, int32_t it, int64_t fixed, int64_t part_bytes,
                           const int64_t *layer_bytes, const int64_t *targets, int64_t *budgets);

/* Host-only, exported for tests: what an encode of this image by these rates
 * starts from -- targets[l] = max(0, floor(rate * W * H / 8) - T - E) and the
 * first budgets max(0, targets[l] - (16 * tile-parts + 256 + 16 * (packets /
 * layers) * (l + 1))) -- with tlm = 1 / `letters` as jp2hip_set_organisation /
 * jp2hip_set_tile_part_divisions would set them.  A lossless top layer has
 * target -1 and budget INT64_MAX.  info (may be NULL): T, E, the plan's
 * tile-part count and packet count of the header estimate.  < 0 with a
 * message for rates or a recipe the encodes refuse. */
int jp2hip_layer_rate_targets(int32_t width, int32_t height, int32_t components, int32_t bits,
                              const jp2hip_recipe *recipe, int32_t letters, int32_t tlm,
                              const double *rates_bpp, int32_t n, int64_t *targets, int64_t *budgets,
                              int64_t *info);

/* Quality layers by target PSNR (OpenJPEG's -q q1,q2,...): with n =
 * recipe.layers targets set, in dB and layer 0 first, layer l is the smallest
 * selection whose predicted PSNR is at least psnr_db[l] -- the highest slope
 * threshold, the fewest hull segments, that reaches it.  An encode has no byte
 * target and no rate loop: the thresholds are found on the device in one
 * selection, and what follows is the fixed-slope encode at those thresholds
 * (the file is the one jp2hip_set_layer_slopes gives at
 * jp2hip_layer_report.threshold).  NULL / n = 0 turns it off.
 *   - The predicted PSNR of a layer is 10 log10(peak^2 * N / D): peak =
 *     2^bits - 1, N = width * height * components of jp2hip_encoded_format
 *     (the upright size under an orientation), D the distortion the layer
 *     leaves as jp2hip_layer_report defines it -- over the code-blocks, the
 *     band's weight times the squared-error decrease of the coding passes the
 *     layer does not hold.  Like the report's, D is exact (against a decoder's
 *     summed squared error) where the transform is orthogonal -- levels = 0 --
 *     and an estimate otherwise.  The irreversible path's
 *     quantisation error is no part of it: D counts what the passes left out
 *     would have removed, so a layer that holds every pass predicts D = 0
 *     where a decoder still sees the quantiser's error.
 *   - D is summed in integer quanta, not in doubles, so that the selection is
 *     exact and the same on every route (jp2hip_distortion_quantum); a layer
 *     meets its target when the quanta it leaves are at most
 *     jp2hip_layer_psnr_targets' integer.  Only segments of the blocks' convex
 *     hulls count: passes behind a hull's last point remove nothing.
 *   - A target so low that no pass is needed takes nothing (the threshold is
 *     one above the largest slope key, as a byte budget of 0 gives); the whole
 *     hull leaves no quanta, so every target is reached by some selection, and
 *     threshold 0 is the lossless top layer's alone.
 *   - recipe.rate_bpp is no target.  > 0 only selects the irreversible
 *     recipe's meaning of "not lossless", and every target must be finite and
 *     > 0.  With rate_bpp <= 0 the last layer takes every coded pass and its
 *     entry must be 0 (a lossless top layer).
 *   - recipe.slope_skip is ignored: every bit-plane is coded, as with slopes.
 *   - stats.rate_iterations = 0; the Kdu-Layer-Info lines print the thresholds
 *     found.
 *   - A lossless recipe's plan has one rate-control group while targets are
 *     set, exactly as with layer rates (a quality target is the whole
 *     image's); the plan cache's key holds that, not the targets.
 *   - PSNR targets, fixed-slope layers and per-layer rates exclude one
 *     another: setting one while another is set is refused.
 *   - Collective like the slopes: peers of jp2hip_split_peers get the targets
 *     here and inherit them when added later; over a caller's callback every
 *     rank sets the same targets.  The ranks agree on the thresholds through
 *     jp2hip_split_psnr_thresholds; the parts concatenate to the single-GPU file.
 *   - An image whose quanta could overflow 63 bits is refused at the encode
 *     with a message (a bound over the plan's code-blocks).
 * Refused, with a message that names the entry (or the other setter): a NaN,
 * an infinity, a negative value, a sequence that decreases anywhere (a last 0
 * is the lossless top layer, no decrease), n outside 0..32; at the encode, n
 * other than the recipe's layers, with rate_bpp <= 0 a last entry other than
 * 0, with rate_bpp > 0 an entry of 0 (the context stays usable).  Not to be
 * called while ctx is encoding. */
int jp2hip_set_layer_psnr(jp2hip_ctx *ctx, const double *psnr_db, int32_t n);

/* Host-only: the checks above on their own -- those of the encode too when
 * `recipe` is given.  Returns 0, or < 0 with a message that names the entry. */
int jp2hip_check_layer_psnr(const double *psnr_db, int32_t n, const jp2hip_recipe *recipe);

/* Host-only, exported for tests: the integer one hull segment -- a distortion
 * decrease dd (tier-1's unit) in a code-block of PCRD weight `weight` --
 * contributes to the selection above, the text the kernels compile:
 *     q = floor((weight * (double)dd) * 2^-s + 0.5),  s = 2 * (bits - 8) - 8,
 * saturated at 2^63 - 1, and 0 where the product is not positive.  A quantum is
 * 2^s squared sample levels: 1/256 of a squared level at 8 bits, the same share
 * of the squared range at every depth.  (double)dd and the product round to
 * nearest; the scale is a power of two; numpy's float64 gives the same bits.
 * < 0 with a message for bits outside 1..16. */
int64_t jp2hip_distortion_quantum(double weight, int64_t dd, int32_t bits);

/* Host-only, exported for tests: the quanta each layer may leave,
 * targets[l] = floor(peak^2 * N * 2^-s / 10^(psnr_db[l] / 10)) with N = width *
 * height * components (saturated at 2^62), and -1 for a last entry of 0, the
 * lossless top layer.  The encodes use this function and nothing else to
 * convert dB.  < 0 with a message for a bad geometry or refused targets. */
int jp2hip_layer_psnr_targets(int32_t width, int32_t height, int32_t components, int32_t bits,
                              const double *psnr_db, int32_t n, int64_t *targets);

/* Host-only: 1 when an encode of this image and recipe by PSNR targets is
 * accepted, 0 when it is refused because its quanta could overflow 63 bits,
 * < 0 with a message for a geometry or recipe no encode takes.  The bound adds,
 * over the plan's code-blocks, weight * 8 * w * h * 4^Mb * 2^-s + (3 Mb - 2); it
 * is loose by the guard bits and the range margin in Mb.  With the default
 * recipes it accepts about 1.25 * 10^9 samples of an RGB image (some 418
 * megapixels, 20 000 x 20 000) and 1.8 * 10^9 of a grey one (lossless; lossy
 * 1.4 and 4.1 * 10^9), at 8 and at 16 bits alike. */
int jp2hip_layer_psnr_fits(int32_t width, int32_t height, int32_t components, int32_t bits,
                           const jp2hip_recipe *recipe);

/* Kdu-Layer-Info's number <-> a threshold for `bits`-bit samples:
 * s = 2^(v + 2 * bits). */
double jp2hip_slope_from_log2(double v, int32_t bits);
double jp2hip_slope_to_log2(double s, int32_t bits);

/* What the layers of the last successful encode on ctx came to (any encode,
 * with slopes or without).  The struct has a tag only, no typedef: the tag
 * shares its name with the function that fills it, which C and C++ allow a
 * tag but not a typedef, so it is written `struct jp2hip_layer_report`. */
struct jp2hip_layer_report {
    int32_t layers, distortion_valid;
    double  threshold[32];   /* the slope each layer was cut at (what the COM prints, before log2) */
    int64_t bytes[32];       /* code-stream bytes through the layer (the COM's L column)          */
    double  distortion[32];  /* predicted squared error left after the layer, sample units,
                                summed over the image; NaN unless enabled                         */
};
/* on = 1: every later encode on ctx (and its tile-split peers) also sums, on
 * the device and after its final selection, the distortion each layer leaves:
 * over the code-blocks, the band's weight times the squared-error decrease of
 * the coding passes the layer does not hold.  Exact (against a decoder's
 * summed squared error) where the transform is orthogonal -- levels = 0 --
 * and an estimate otherwise.  Deterministic: two runs of one
 * encode on one route give equal bits.  Default 0: nothing is launched. */
int jp2hip_set_layer_report(jp2hip_ctx *ctx, int32_t on);
/* Copies the report; < 0 when no encode on ctx has succeeded yet.  After a
 * tile-split over a caller's callback only rank 0's report is whole. */
int jp2hip_layer_report(jp2hip_ctx *ctx, struct jp2hip_layer_report *r);

/* Which SDMA engines the code-stream copies use, per GPU probed so far, and
 * every engine's measured device -> host rate ("" before the first encode):
 * engines differ several-fold on MI355X and the choice is timed once per
 * GPU, so a benchmark records it to be comparable with another run. */
const char *jp2hip_dma_engines(void);

/* Free and total memory of HIP device `device` (bytes): what a converter
 * sizes its context pool from.  Returns 0 or < 0. */
int jp2hip_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes);

/* Converter.convert(): TIFF file -> JPEG 2000 file, written atomically
 * (temp file + rename; nothing is left behind on failure).
 * recipe == NULL -> jp2hip_recipe_init(conversion).  Returns 0 or < 0. */
int jp2hip_encode_file(jp2hip_ctx *ctx, const char *tiff_path_utf8, const char *out_path_utf8,
                       int conversion, const jp2hip_recipe *recipe, jp2hip_stats *stats);

/* TIFF bytes in host memory -> encoded bytes.  *out is pinned host memory
 * (the code-stream is copied straight into it from HBM); release it with
 * jp2hip_free, never free(). */
int jp2hip_encode_tiff(jp2hip_ctx *ctx, const uint8_t *tiff, size_t len, int conversion,
                       const jp2hip_recipe *recipe, uint8_t **out, size_t *out_len,
                       jp2hip_stats *stats);

/* Parse a baseline TIFF's header into a layout (offsets into the file).
 * Strips may be uncompressed, LZW (5), Deflate (8, 32946; zlib streams) or
 * PackBits (32773), with or without
 * horizontal differencing (Predictor 2); compressed strips are decoded on
 * the GPU before ingest (LZW segment-parallel: a wave finds a strip's
 * Clear-code segments, a wave per segment resolves its codes; Deflate and
 * PackBits a wave per strip).  For a compressed file
 * `offsets` receives 2 * nstrips entries: the strip offsets, then their byte
 * counts (layout->strip_bytes points at the second half).  Tiled TIFFs
 * (TileWidth/TileLength) are described the same way, one entry per tile,
 * and always carry the byte counts; they are untiled in HBM before ingest.
 * The metadata fields come from ICCProfile (34675; layout->icc points into
 * `tiff`, so it lives as long as that buffer), ExtraSamples (338),
 * X/YResolution (282, 283) and ResolutionUnit (296); a malformed or
 * out-of-range metadata tag counts as absent and never fails the parse.
 * Pixel formats: 8- and 16-bit BlackIsZero grey and RGB (with or without an
 * extra sample); 1-, 2- and 4-bit grey, BlackIsZero or WhiteIsZero, in
 * either FillOrder (266); palette colour (PhotometricInterpretation 3) of
 * 1, 2, 4 or 8 bits with a ColorMap (320) of exactly 3 * 2^bits SHORTs that
 * lies inside the file (layout->colormap points into `tiff`).  Refused, each
 * with its own message: sub-byte samples with more than one sample per
 * pixel, other bit depths, Predictor 2 below 8 bits, a palette without a
 * (whole) ColorMap or with 16-bit indices, 8- and 16-bit WhiteIsZero, CMYK,
 * YCbCr, Lab, JPEG and CCITT compression. */
int jp2hip_tiff_layout(const uint8_t *tiff, size_t len, jp2hip_layout *layout,
                       uint64_t *offsets, int32_t max_offsets);

/* What the code-stream of this source carries: 3 components of 8 bits for a
 * palette, 1 of 8 bits for 1-, 2- and 4-bit grey, else the layout's own
 * components and bits.  Returns 0, or < 0 on a null argument. */
int jp2hip_encoded_format(const jp2hip_layout *layout, int32_t *components, int32_t *bits);

/* The bytes that precede the code-stream (signature .. jp2c box header) for
 * this source description, format and code-stream length.  Returns their
 * count (0 for JP2HIP_FORMAT_J2K) and writes them when cap suffices; < 0 on
 * a null argument.  Reads only width/height/components/bits, the pixel
 * format (the header describes jp2hip_encoded_format's components and bits)
 * and the metadata fields of the layout; no strips, no context, no device.
 *   colr: no (usable) ICC profile -> enumerated sRGB / greyscale; a matrix /
 *     TRC input or display profile -> METH 2 with the profile; any other
 *     profile -> JPX: the enumerated box, then METH 3 with the profile
 *     (a JP2 reader takes the first box); JP2: the enumerated box alone.
 *   cdef: by extra_samples (above), for 2 or 4 channels.
 *   res : one resc box (capture resolution, points per metre).
 * The layout is taken as it is: a caller describing a file encoded with a
 * source orientation of 5 .. 8 passes the upright image's layout -- width and
 * height exchanged, and xres_* with yres_* -- as the encodes do themselves. */
int64_t jp2hip_file_header(const jp2hip_layout *layout, int32_t format,
                           uint64_t codestream_bytes, uint8_t *dst, size_t cap);

/* Device-resident source: d_src holds the TIFF file (or any buffer the
 * layout describes) in HBM.  This is the entry the benchmark times. */
int jp2hip_encode_device(jp2hip_ctx *ctx, const void *d_src, size_t src_len,
                         const jp2hip_layout *layout, int conversion,
                         const jp2hip_recipe *recipe, uint8_t **out, size_t *out_len,
                         jp2hip_stats *stats);

/* Releases an *out buffer of the encode calls.  It returns to the process's
 * pool of pinned buffers, so steady-state encodes pin nothing new; the pool
 * keeps as many returned buffers as were ever handed out at once (each
 * counted at the largest size pinned), at least 4 GiB, and unpins the
 * largest beyond that. */
void jp2hip_free(void *p);

/* ------------------------------------------------------------------------
 * Tile-split path: one oversized image across GPUs.
 *
 * No reference interface exists for this (kdu_compress encodes one image in
 * one process, KakaduConverter.java:61-71); it is the north_star's "RCCL only
 * if a single oversized image is split across GPUs".  Rank r of `world`
 * encodes the contiguous band of tile rows jp2hip_split_rows() names
 * (ingest, DWT, tier-1 and hulls of its tiles only); the ranks agree on the
 * PCRD layer thresholds exactly through `allreduce_sum` (a caller-supplied
 * in-place int64 sum over ranks -- RCCL/torch.distributed on the node), so
 * the concatenation of every rank's part, in rank order, is byte-identical
 * to the single-GPU jp2hip_encode_device() output.  The only exchange is a
 * few hundred all-reduces of <= 64 int64 (threshold bisection, tier-2 sizes);
 * no pixel or coefficient crosses GPUs.
 * ---------------------------------------------------------------------- */
typedef int (*jp2hip_allreduce_fn)(void *user, int64_t *values, int32_t n); /* in-place sum; 0 ok */

typedef struct jp2hip_split {
    int32_t rank, world;
    jp2hip_allreduce_fn allreduce_sum; /* may be NULL when world == 1 */
    void *user;
} jp2hip_split;

/* Image rows [*row0, *row1) whose tiles rank `rank` encodes: whole
 * -flush_period stripes of tile rows (recipe.flush_period), so every rank's
 * tile-parts are one contiguous run of the file.  tile_h = 0 is the untiled
 * recipe (tile_w = tile_h = 0): one tile row, which is all rank 0's -- the
 * other ranks get the empty band [height, height). */
void jp2hip_split_rows(int32_t height, int32_t tile_h, int32_t flush_period, int32_t rank, int32_t world,
                       int32_t *row0, int32_t *row1);

/* This rank's part of the file: *out (jp2hip_free) goes at byte *file_offset
 * of a *file_len-byte file.  Rank 0's part starts with the file and main
 * headers, the last rank's ends with EOC.  d_src/layout describe the whole
 * TIFF, but only the strips of this rank's rows are read, so d_src may hold
 * just those (with strip offsets relative to it).  Collective: every rank
 * must call it with the same image geometry, recipe and source metadata
 * (extra_samples .. icc_bytes, the profile's bytes included; rank 0 sizes
 * and writes the file header from its own layout).
 * With a source orientation (jp2hip_set_source_orientation, collective too)
 * the bands are bands of the upright image: jp2hip_split_rows takes the
 * upright height, and the strips a rank reads are those of
 * jp2hip_orientation_source_rows of its band -- its mirrored band for 3 and
 * 4, and for 5 .. 8, where an upright row is a stored column, every strip:
 * d_src must then hold the whole source on every rank (each decodes it and
 * turns only the columns of its band). */
int jp2hip_encode_device_split(jp2hip_ctx *ctx, const void *d_src, size_t src_len,
                               const jp2hip_layout *layout, int conversion,
                               const jp2hip_recipe *recipe, const jp2hip_split *split,
                               uint8_t **out, size_t *out_len, uint64_t *file_offset,
                               uint64_t *file_len, jp2hip_stats *stats);

/* The tile-split behind Converter.convert (Converter.java:22 ->
 * jp2hip_encode_file / jp2hip_encode_tiff on ctx): gives ctx `n` peer
 * contexts, one on each HIP ordinal in `ordinals` (created here, owned by ctx;
 * an ordinal may repeat, or be ctx's own device).  From then on an image of at
 * least `min_pixels` pixels (width x height) given to ctx is encoded as a
 * tile-split over world = n + 1 ranks -- ctx is rank 0, peer i rank i + 1 --
 * each rank a thread of this call: it reads its band's strips from the TIFF
 * (mapped, not read whole), uploads them to its own GPU, and writes its part
 * at its offset of the output file; the ranks' exchanges are summed on the
 * host (no caller callback, no RCCL needed in-process).  The file is
 * byte-identical to the single-GPU encode.  Smaller images take the
 * single-GPU path.  The split divides tile rows: an untiled image (tile_w =
 * tile_h = 0) or any image of one tile row gains nothing from it -- one rank
 * encodes everything, the others only join the exchanges.  n = 0 removes the
 * peers.  Not to be called while ctx is encoding.  Returns 0 or < 0. */
int jp2hip_split_peers(jp2hip_ctx *ctx, const int32_t *ordinals, int32_t n, int64_t min_pixels);

/* Width x height of a TIFF file from its header (the file is mapped, not
 * read), or < 0 with jp2hip_last_error(): lets a converter route an
 * oversized image to its split context before converting it. */
int64_t jp2hip_tiff_pixels(const char *tiff_path_utf8);

/* Host-only: global layer thresholds from this rank's hull segments (slope
 * keys descending, inclusive byte sums) -- the exchange step of the split
 * encode, exported for tests.  K[l] = min{k : sum over ranks of bytes with
 * key >= k <= budgets[l]}. */
int jp2hip_split_thresholds(const uint64_t *keys, const int64_t *cum, int64_t nseg,
                            const int64_t *budgets, int32_t layers, const jp2hip_split *split,
                            uint64_t *K);

/* Host-only: the same exchange for quality layers by target PSNR
 * (jp2hip_set_layer_psnr), exported for tests -- this rank's hull segments as
 * slope keys descending and inclusive sums of distortion quanta
 * (jp2hip_distortion_quantum), targets as jp2hip_layer_psnr_targets gives them.
 * With need[l] = (sum over ranks of all quanta) - targets[l],
 * K[l] = max{k : sum over ranks of quanta with key >= k >= need[l]}: the tie
 * group at K[l] is taken.  need[l] <= 0 takes nothing: K[l] is one above the
 * largest key of all ranks (0 when no rank has a segment).  A need the total
 * does not reach (targets[l] < 0, the lossless top layer) gives K[l] = 0.
 * Collective: every rank calls it with the same targets, a rank without
 * segments with nseg = 0.  Returns 0, -1 for a bad argument, -2 when the
 * all-reduce failed. */
int jp2hip_split_psnr_thresholds(const uint64_t *keys, const int64_t *cum_quanta, int64_t nseg,
                                 const int64_t *targets, int32_t layers, const jp2hip_split *split,
                                 uint64_t *K);

/* Host-only: the packets of tile `tile` (raster index) of a width x height
 * image of `components` x `bits`-bit samples, in the order recipe->progression
 * sends them -- the function the encodes lay their tile-parts out with,
 * exported for tests.  Entry s names the s-th packet as p * layers + l: layer
 * l of the tile's p-th precinct counted in (resolution, precinct row, precinct
 * column, component) order, the order the packets are stored in (so RPCL
 * gives 0, 1, 2, ...).  tile_w = tile_h = 0 means what it means to an encode:
 * one tile.  Returns the tile's packet count and writes the first
 * min(count, cap) entries to seq (which may be NULL when cap is 0), or < 0
 * with jp2hip_last_error() for a recipe or geometry the encodes refuse. */
int64_t jp2hip_packet_sequence(int32_t width, int32_t height, int32_t components, int32_t bits,
                               const jp2hip_recipe *recipe, int32_t tile, uint32_t *seq, int64_t cap);

/* ------------------------------------------------------------------------
 * Batch path: one GPU's work queue for a CSV batch.
 *
 * Replaces the chain a CSV row takes through the reference
 *   LoadCsvHandler.java:250-289 -> LargeImageVerticle.java:65-108 ->
 *   ImageWorkerVerticle.java:54-110 (convert LOSSLESS, reply, then hand the
 *   JPX to S3BucketVerticle with derivative-image=true) ->
 *   S3BucketVerticle.java:88-211,286-303 (PUT, delete the JPX after a
 *   successful upload)
 * with a native pipeline per GPU: reader threads (TIFF file -> pinned host
 * buffer, header parse), one encoder thread per context (images in flight on
 * the GPU, each with its own HIP stream), and uploader threads (atomic JPX
 * write, upload callback, delete-after-upload), so file I/O and the upload
 * overlap the encodes.  Images are independent: N GPUs run N of these
 * (one process per GPU), sharded by the caller; no collective.
 * ---------------------------------------------------------------------- */
typedef struct jp2hip_batch jp2hip_batch;

/* Upload hook (S3BucketVerticle stand-in): called on an uploader thread with
 * the image id (S3 key = file name, ImageWorkerVerticle.java:69) and the
 * written JPX path.  Return 0 on success.  NULL selects the built-in stub,
 * which reads every byte of the file and succeeds (FakeS3BucketVerticle). */
typedef int (*jp2hip_upload_fn)(void *user, const char *image_id_utf8, const char *jpx_path_utf8);

typedef struct jp2hip_batch_config {
    int32_t device;              /* HIP device ordinal                               */
    int32_t contexts;            /* images in flight on the GPU (<=0: 12)            */
    int32_t reader_threads;      /* TIFF readers (<=0: 4)                            */
    int32_t uploader_threads;    /* JPX writers + uploaders (<=0: 4)                 */
    int32_t host_threads;        /* tier-2 threads per context (<=0: 16 / contexts)  */
    int32_t delete_after_upload; /* derivative-image=true: remove the JPX once sent  */
    int32_t write_output;        /* 0: keep the JPX in memory, skip the file write   */
    int32_t reserved;
} jp2hip_batch_config;

#define JP2HIP_BATCH_OK 0
#define JP2HIP_BATCH_CONVERT_FAILED (-1) /* ImageWorker replies failure (IOException) */
#define JP2HIP_BATCH_UPLOAD_FAILED (-2)  /* S3 upload failed; callback gets "false"   */

typedef struct jp2hip_batch_result {
    int64_t job;          /* the caller's job number from jp2hip_batch_submit     */
    int32_t status;       /* JP2HIP_BATCH_*                                       */
    int32_t reserved;
    int64_t in_bytes;     /* TIFF file size                                       */
    int64_t out_bytes;    /* JPX size                                             */
    int64_t pixels;       /* width * height                                       */
    double read_ms;       /* file -> pinned buffer + header parse                 */
    double encode_ms;     /* H2D + GPU encode + tier-2 (jp2hip_encode_tiff)       */
    double upload_ms;     /* file write + upload hook + delete                    */
    char message[240];    /* failure text ("" on success)                         */
} jp2hip_batch_result;

int jp2hip_batch_create(jp2hip_batch **out, const jp2hip_batch_config *cfg, jp2hip_upload_fn upload,
                        void *user);
/* jp2hip_set_organisation on every context of the queue; before the first
 * submit (< 0 after it, or for a refused organisation). */
int jp2hip_batch_set_organisation(jp2hip_batch *b, const jp2hip_organisation *org);
/* jp2hip_set_tile_part_divisions on every context of the queue; before the
 * first submit (< 0 after it, or for refused letters). */
int jp2hip_batch_set_tile_part_divisions(jp2hip_batch *b, int32_t letters);
/* jp2hip_set_layer_slopes on every context of the queue; before the first
 * submit (< 0 after it, or for refused slopes). */
int jp2hip_batch_set_layer_slopes(jp2hip_batch *b, const double *slopes, int32_t n);
/* jp2hip_set_layer_rates on every context of the queue; before the first
 * submit (< 0 after it, or for refused rates). */
int jp2hip_batch_set_layer_rates(jp2hip_batch *b, const double *rates_bpp, int32_t n);
/* jp2hip_set_layer_psnr on every context of the queue; before the first
 * submit (< 0 after it, or for refused targets). */
int jp2hip_batch_set_layer_psnr(jp2hip_batch *b, const double *psnr_db, int32_t n);
/* jp2hip_set_source_orientation on every context of the queue; before the
 * first submit (< 0 after it, or for a refused value). */
int jp2hip_batch_set_source_orientation(jp2hip_batch *b, int32_t o);
/* Queue one image: convert `tiff_path` into `jpx_path` (written atomically)
 * with `conversion` (recipe NULL -> Bucketeer recipe), then upload it under
 * `image_id`.  Never blocks on the GPU; returns < 0 after close. */
int jp2hip_batch_submit(jp2hip_batch *b, int64_t job, const char *image_id_utf8, const char *tiff_path_utf8,
                        const char *jpx_path_utf8, int conversion, const jp2hip_recipe *recipe);
/* Collect up to `max` finished jobs (uploaded or failed); waits up to
 * timeout_ms (< 0: until at least one is ready or nothing is pending).
 * Returns the number written to `results`. */
int jp2hip_batch_wait(jp2hip_batch *b, jp2hip_batch_result *results, int max, int timeout_ms);
/* Jobs submitted and not yet returned by jp2hip_batch_wait. */
int64_t jp2hip_batch_pending(jp2hip_batch *b);
/* Stop accepting jobs, finish the queued ones, join all threads. */
void jp2hip_batch_destroy(jp2hip_batch *b);

#ifdef __cplusplus
}
#endif
#endif
