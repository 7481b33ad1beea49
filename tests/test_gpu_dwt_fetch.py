"""DWT level 1 loads a chunky pixel with one access (csrc/dwt_fetch.h): RGB8
reads one byte past the pixel, RGB16 two, so the cases here are the shapes,
sample layouts and buffer placements where that access meets an edge -- the
last pixel of a source that ends with it, misaligned bases, width 1, strips
of one row -- each byte-identical to the CPU oracle in both conversions, as
in test_gpu_parity.  One more case sends odd sizes and widths that are no
multiple of 16 through levels 2-3 and the tail."""
import numpy as np
import pytest

import imaging as im
import jp2hip
import oracle_lib as ol
from devmem import DeviceBytes

pytestmark = pytest.mark.gpu

CONVS = [jp2hip.LOSSLESS, jp2hip.LOSSY]


def _rgb8(w, h, seed):
    return im.synth_rgb8(h, w, seed=seed)


def _img(kind, w, h, seed):
    if kind == "rgb16":
        return im.synth_u16(h, w, comps=3, seed=seed)
    if kind == "gray16":
        return im.synth_u16(h, w, comps=1, seed=seed)
    a = _rgb8(w, h, seed)
    if kind == "gray8":
        return a[..., 0].copy()
    if kind == "rgba8":
        return np.dstack([a, (a[..., 1] // 3 + 40).astype(np.uint8)])
    return a


def _check(encoder, img, tif, conv, **recipe):
    rc = jp2hip.recipe(conv, **recipe)
    got, _ = encoder.encode_tiff(tif, conv, rc)
    assert got == ol.encode(img, ol.copy_recipe(rc))


# width x height, tiff_bytes arguments, recipe overrides
SHAPES = [
    (48, 40, {}, {"tile_w": 32, "tile_h": 32, "levels": 5}),  # ragged tile edge (32 = 2^levels)
    (17, 9, {}, {}),
    (1, 1, {}, {}),
    (2, 1, {}, {}),
    (1, 5, {}, {}),  # width 1
    (5, 1, {}, {}),
    (33, 64, {"rows_per_strip": 1}, {}),
    (33, 64, {"rows_per_strip": 64}, {}),
]


@pytest.mark.parametrize("conv", CONVS, ids=["ll", "ly"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" + "".join(f"_{k}{v}" for k, v in {**s[2], **s[3]}.items())
                                               for s in SHAPES])
def test_rgb8_shapes(encoder, shape, conv):
    """(1x1 and 2x1 lossy also pin the rate target of 0 bytes -- 3 bpp of one
    or two pixels -- at which slope prediction still runs, as in the oracle:
    the Kdu-Layer-Info slopes come from the hulls of the planes it codes.)"""
    w, h, kw, recipe = shape
    img = _rgb8(w, h, seed=3 * w + h)
    _check(encoder, img, im.tiff_bytes(img, **kw), conv, **recipe)


LAYOUT_SIZES = ((33, 20), (1, 3))  # width x height, the default recipe
PLACEMENT_SIZE = (37, 21)
# width x height, recipe overrides: the levels above the first
LEVELS_2_UP = (200, 136, {"tile_w": 128, "tile_h": 128, "levels": 5})
BAND_EDGES = (530, 300, {})

LAYOUTS = [
    ("rgb16", {}),
    ("rgb16", {"big_endian": True}),
    ("rgba8", {}),
    ("gray8", {}),
    ("gray16", {}),
    ("gray16", {"big_endian": True}),
    ("rgb8", {"planar": True}),  # the per-sample path
]


@pytest.mark.parametrize("conv", CONVS, ids=["ll", "ly"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[k + "".join("_" + x for x in kw) for k, kw in LAYOUTS])
def test_sample_layouts(encoder, layout, conv):
    kind, kw = layout
    for w, h in LAYOUT_SIZES:
        img = _img(kind, w, h, seed=11)
        _check(encoder, img, im.tiff_bytes(img, rows_per_strip=7, **kw), conv)


@pytest.mark.parametrize("conv", CONVS, ids=["ll", "ly"])
@pytest.mark.parametrize("kind", ["rgb8", "rgb16"])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_buffer_placement(encoder, shift, kind, conv):
    """The device buffer holds exactly the file's bytes (its last byte is the
    last pixel's last sample), or the file starts 1-3 bytes into a larger
    buffer (no pixel is aligned to its access)."""
    img = _img(kind, *PLACEMENT_SIZE, seed=5)
    tif = im.tiff_bytes(img, rows_per_strip=8)
    lay, keep = jp2hip.tiff_layout(tif)
    assert lay.strip_offsets[lay.nstrips - 1] + (21 - 16) * 37 * 3 * img.dtype.itemsize == len(tif)
    rc = jp2hip.recipe(conv)
    d = DeviceBytes(b"\xEE" * shift + tif + (b"\xEE" * 5 if shift else b""))
    try:
        got, _ = encoder.encode_device(d.ptr + shift, len(tif), lay, conv, rc)
    finally:
        d.free()
    assert got == ol.encode(img, ol.copy_recipe(rc))


@pytest.mark.parametrize("conv", CONVS, ids=["ll", "ly"])
def test_levels_2_up_odd_sizes(encoder, conv):
    """200 x 136 in 128^2 tiles, 5 levels: levels 2-3 (k_dwt_band) and the
    tail see odd sizes and widths that are no multiple of 16."""
    w, h, recipe = LEVELS_2_UP
    img = _rgb8(w, h, seed=8)
    _check(encoder, img, im.tiff_bytes(img), conv, **recipe)


@pytest.mark.parametrize("conv", CONVS, ids=["ll", "ly"])
def test_band_kernel_edges(encoder, conv):
    """530 x 300 in 512^2 tiles: tile widths 512 and 18, so level 2 runs
    k_dwt_band's 256-thread form and level 3 its 128-thread form (the case
    above reaches the tail at level 2; csrc/dwt_route.h decides, and
    test_large_tiles.py checks that these shapes still get there), each with a full-width tile (the
    straight-line horizontal lifting), a narrow one, a first and a last band
    (windows that touch rows 0 and H-1) and a last band of fewer than 16 rows."""
    w, h, recipe = BAND_EDGES
    img = _rgb8(w, h, seed=9)
    _check(encoder, img, im.tiff_bytes(img), conv, **recipe)
