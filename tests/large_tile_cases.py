"""Cases for tiles wider or taller than 4096, up to one tile per image
(tests/test_large_tiles.py on the CPU, tests/test_gpu_large_tiles.py on the
GPU).  A level whose rows do not fit in a workgroup's LDS is lifted in column
chunks (csrc/dwt_chunk.h); the constants below repeat that header's so the
cases can be laid around the chunk boundaries, and test_large_tiles.py checks
that they still equal it.

Every image stays under 1.5 MP per component.  The expected file is always the
oracle's encode of the same pixels with the same recipe (tile_w = tile_h = 0:
with the resolved sizes, `resolved`)."""
import numpy as np

import imaging as im
import jp2hip

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY

# csrc/dwt_chunk.h: kept columns per workgroup of the chunked kernels
L1_CHUNK_W = 496    # k_dwt_l1<.., CHUNK>: level 1 with ingest
BAND_CHUNK_W = 496  # k_dwt_band<.., CHUNK>: levels >= 2
CHUNK_HALO = 4
# A level keeps its whole-row kernel while 16 rows of it fit in 160 KiB of LDS
# (csrc/dwt_route.h dwt_route): up to 2496 columns.  Tile widths that send level
# lv -- and every level above it -- to the chunked kernels, multiples of 2^6
# (test_large_tiles.py asks dwt_route for both):
WHOLE_ROW_MAX_W = 2496
CHUNKED_FROM_LEVEL = {1: 4096, 2: 5120, 3: 10240}


def resolved(w, h, levels):
    """What tile_w = tile_h = 0 becomes for a w x h image: the smallest
    multiples of 2^levels not below the width and height."""
    m = 1 << levels
    return -(-w // m) * m, -(-h // m) * m


_cache = {}


def image(h, w, comps, bits, seed=7):
    """Synthetic content (imaging.synth_rgb8 / synth_u16), made once per shape."""
    k = (h, w, comps, bits, seed)
    if k not in _cache:
        if bits == 16:
            a = im.synth_u16(h, w, comps=comps, seed=seed)
        else:
            rgb = im.synth_rgb8(h, w, seed=seed)
            if comps == 1:
                a = rgb[..., 1].copy()
            elif comps == 4:
                a = np.dstack([rgb, (rgb[..., 1] // 3 + 40).astype(np.uint8)])
            else:
                a = rgb
        a.setflags(write=False)
        _cache[k] = a
    return _cache[k]


def case(name, h, w, comps, bits, convs, **ov):
    return dict(name=name, h=h, w=w, comps=comps, bits=bits, convs=convs, ov=ov)


# The numbered shapes: h x w x comps, bits; levels; tile_w x tile_h.
C1 = case("1_l1_ingest_70x4200x3", 70, 4200, 3, 8, (LL, LY), levels=6, tile_w=4224, tile_h=128)
C2 = case("2_levels23_40x8300_g16", 40, 8300, 1, 16, (LL,), levels=6, tile_w=8320, tile_h=64)
C3 = case("3_100x16500_g8_L7", 100, 16500, 1, 8, (LL,), levels=7, tile_w=16512, tile_h=128)
C4 = case("4_tall_4200x40", 4200, 40, 1, 8, (LL,), levels=6, tile_w=64, tile_h=4224)
C5 = case("5_last_chunk_1_300x4097x3", 300, 4097, 3, 8, (LL,), levels=5, tile_w=4160, tile_h=320)
C6 = case("6_three_columns_90x8400x3", 90, 8400, 3, 8, (LL,), levels=6, tile_w=4160, tile_h=64)
C7 = case("7_rate_loop_1000x5000x3", 1000, 5000, 3, 8, (LY,), levels=6, tile_w=5056, tile_h=1024)
# 79 992 packets in one tile: Nsop wraps at 65536
C9 = case("9_nsop_wraps_600x4200x3", 600, 4200, 3, 8, (LL,), levels=2, tile_w=4224, tile_h=640, layers=8,
          nprecincts=1, prec_w_log2=[5], prec_h_log2=[5], cblk_w_log2=4, cblk_h_log2=4)
C9_PACKETS = 79992

NUMBERED = [C1, C2, C3, C4, C5, C6, C7, C9]
UNTILED = [C1, C2, C4, C6]  # case 8: the same with tile_w = tile_h = 0


def chunk_edge_widths(C):
    """Tile-component widths at the chunked level that put a row's end just
    past, on and around the chunk boundaries."""
    return [C + 1, C + 2, C + 16, C + 17, 2 * C - 1, 2 * C, 2 * C + 1, 3 * C + 5]


# case 10: (kernel, its kept width, the level it runs at)
CHUNK_KERNELS = [("l1", L1_CHUNK_W, 1), ("band", BAND_CHUNK_W, 2), ("band", BAND_CHUNK_W, 3)]
CHUNK_EDGE_VARIANTS = [(h, comps, bits) for h in (9, 33) for comps in (1, 3) for bits in (8, 16)]


def chunk_edge_cases():
    """One entry per (kernel, level, width at that level): the image width
    gives exactly that width at the level, the tile width sends the level to
    the chunked kernel.  Each entry is run for every CHUNK_EDGE_VARIANTS
    (height, components, bits) in both conversions."""
    out = []
    for kern, C, lv in CHUNK_KERNELS:
        for wl in chunk_edge_widths(C):
            w = wl << (lv - 1)
            assert -(-w // (1 << (lv - 1))) == wl
            out.append(dict(name=f"{kern}_L{lv}_w{wl}", w=w, ov=dict(levels=6, tile_w=CHUNKED_FROM_LEVEL[lv], tile_h=64)))
    return out


# case 11: tile widths the plan admitted before this path existed although 16
# rows of level 1 do not fit in LDS
GAP_TILE_WIDTHS = [2560, 3072, 4096]
GAP_COMPS = [1, 3, 4]


def gap_case(tile_w, comps):
    return case(f"11_tile{tile_w}_c{comps}", 48, 4100, comps, 8, (LL, LY), levels=5, tile_w=tile_w, tile_h=64)


def source_variants(c):
    """case 12: (name, image, TIFF bytes) of other ingest routes for the
    shape and recipe of case `c`: planar samples and RGBA16 (cases 1 and 5),
    LZW strips and a tiled TIFF (case 1)."""
    rgb = image(c["h"], c["w"], 3, 8)
    rgba16 = image(c["h"], c["w"], 4, 16)
    out = [("planar", rgb, im.tiff_bytes(rgb, planar=True)),
           ("rgba16", rgba16, im.tiff_bytes(rgba16))]
    if c is C1:
        out += [("lzw", rgb, im.tiff_bytes_compressed(rgb, "tiff_lzw")),
                ("tiled_tiff", rgb, im.tiled_tiff_bytes(rgb, tile=(64, 48)))]
    return out
