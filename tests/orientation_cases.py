"""TIFF Orientation (tag 274) fixtures and what the tag means, for
test_orientation.py and test_gpu_orientation.py.

`upright` is the expectation, written from the TIFF 6.0 meaning of the eight
values and nothing else: it imports nothing of the product.
test_orientation.py pins it to Pillow's reading of the same files
(ImageOps.exif_transpose).  The fixtures come from the writers the suite
already has; the tag is added with metadata_fixtures.add_tags."""
from __future__ import annotations

import ctypes
import struct

import numpy as np

import imaging as im
import metadata_fixtures as mf

ORIENTATION = 274
VALUES = tuple(range(1, 9))

# (h, w): single pixels and lines, one 64 x 64 tile of the transposing kernel
# (csrc/stages.h kOrientTile) with a pixel more and less on each side, and
# more than one tile both ways with ragged edges
SIZES = ((1, 1), (1, 77), (77, 1), (63, 65), (64, 64), (65, 63), (130, 67))


def upright(a: np.ndarray, o: int) -> np.ndarray:
    """The image a viewer shows for stored pixels `a` (h x w, samples last)
    tagged Orientation `o`."""
    out = {1: lambda: a,
           2: lambda: a[:, ::-1],
           3: lambda: a[::-1, ::-1],
           4: lambda: a[::-1],
           5: lambda: a.swapaxes(0, 1),
           6: lambda: np.rot90(a, -1),
           7: lambda: a[::-1, ::-1].swapaxes(0, 1),
           8: lambda: np.rot90(a, 1)}[o]()
    return np.ascontiguousarray(out)


def tag(tif: bytes, o: int, typ: int = mf.SHORT, count: int = 1) -> bytes:
    """`tif` with an Orientation entry of value `o` (any value: the parser
    tests write 0 and 9 too; typ / count: malformed entries)."""
    e = mf.byte_order(tif)
    payload = struct.pack(e + ("I" if typ == mf.LONG else "H"), o) * count
    return mf.add_tags(tif, [(ORIENTATION, typ, count, payload)])


def pixels(form: str, h: int, w: int, seed: int = 5) -> np.ndarray:
    """A ramp that differs along x, along y and between components, plus
    noise: no mirrored or turned copy of it equals it, and a 16-bit sample's
    two bytes differ."""
    rng = np.random.default_rng(seed + 131 * h + w)
    nc = {"grey8": 1, "rgb8": 3, "rgba8": 4, "grey16le": 1, "rgb16be": 3, "rgba16": 4, "planar_rgb8": 3,
          "planar_rgb16": 3}[form]
    wide = "16" in form
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(nc), indexing="ij")
    a = (5 * y + 11 * x + 37 * c) % 200 + rng.integers(0, 40, size=(h, w, nc))
    if wide:
        a = a * 257 + rng.integers(0, 200, size=(h, w, nc))
    a = a.astype(np.uint16 if wide else np.uint8)
    return np.ascontiguousarray(a[..., 0] if nc == 1 else a)


FORMS = ("rgb8", "grey8", "rgba8", "grey16le", "rgb16be", "rgba16", "planar_rgb8", "planar_rgb16")


def form_tiff(form: str, px: np.ndarray, rows_per_strip: int = 16) -> bytes:
    """The uncompressed strip TIFF of `px` in element form `form`."""
    return im.tiff_bytes(px, rows_per_strip=rows_per_strip, planar=form.startswith("planar"),
                         big_endian=form.endswith("be"))


def oriented_layout(lay, o: int):
    """The layout a caller describes the upright image of `lay` with (a
    jp2hip Layout; the strips stay the stored image's): for 5..8 width and
    height change places, and X with Y resolution."""
    up = type(lay)()
    ctypes.memmove(ctypes.byref(up), ctypes.byref(lay), ctypes.sizeof(up))
    up.copy_metadata(lay)
    up.copy_pixel_format(lay)
    if o >= 5:
        up.width, up.height = lay.height, lay.width
        up.xres_num, up.xres_den, up.yres_num, up.yres_den = lay.yres_num, lay.yres_den, lay.xres_num, lay.xres_den
    return up
