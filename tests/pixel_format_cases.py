"""Bilevel, 2- and 4-bit grey and palette-colour TIFF fixtures, and what
their pixels mean, for test_pixel_formats.py and test_gpu_pixel_formats.py.

The fixtures come from the writers the suite already has: the indices are
packed into bytes with numpy, written as an 8-bit grey image
(imaging.tiff_bytes / tiled_tiff_bytes / bigtiff_bytes, with their strip
codecs), and ImageWidth, BitsPerSample, PhotometricInterpretation and
TileWidth are then patched to what the bytes really are; ColorMap and
FillOrder are added with metadata_fixtures.add_tags.

`expand` is the expectation, written from the TIFF 6.0 meaning of the tags
and nothing else: it imports nothing of the product.  test_pixel_formats.py
pins it to Pillow's reading of the same files."""
from __future__ import annotations

import struct
import zlib

import numpy as np

import imaging as im
import metadata_fixtures as mf

BLACK_IS_ZERO, WHITE_IS_ZERO, PALETTE = 1, 0, 3
_REVERSE = np.array([int(f"{b:08b}"[::-1], 2) for b in range(256)], np.uint8)
CODECS = {None: (None, 1), "lzw": (im.lzw_encode, 5), "deflate": (zlib.compress, 8),
          "packbits": (im.packbits_encode, 32773)}


def expand(idx: np.ndarray, bits: int, photometric: int, colormap: np.ndarray | None = None) -> np.ndarray:
    """The 8-bit pixels a source of `bits`-bit values `idx` (h x w) stands
    for: grey (h, w), or RGB (h, w, 3) for a palette whose `colormap` is
    (3, 2^bits) uint16 -- red, green and blue rows."""
    if photometric == PALETTE:
        cm = np.asarray(colormap, np.uint16).reshape(3, 1 << bits)
        cm8 = (cm if cm.max() <= 255 else cm >> 8).astype(np.uint8)  # 8-bit maps of old writers: as they are
        return np.ascontiguousarray(np.stack([cm8[c][idx] for c in range(3)], axis=-1))
    v = idx.astype(np.uint16) * (255 // ((1 << bits) - 1))
    if photometric == WHITE_IS_ZERO:
        v = 255 - v
    return np.ascontiguousarray(v.astype(np.uint8))


def pack_rows(idx: np.ndarray, bits: int, fill_order: int = 1, pad: int = 1) -> np.ndarray:
    """(h, ceil(w * bits / 8)) bytes: every row starts on a byte boundary,
    the first pixel of a byte in its high bits (FillOrder 1) or, the whole
    byte bit-reversed, in its low bits (FillOrder 2).  The pad bits at a
    row's end are set to `pad` in every bit (readers ignore them)."""
    h, w = idx.shape
    if bits == 8:
        return np.ascontiguousarray(idx.astype(np.uint8))
    per = 8 // bits
    rb = (w + per - 1) // per
    full = np.full((h, rb * per), ((1 << bits) - 1) if pad else 0, np.uint8)
    full[:, :w] = idx
    g = full.reshape(h, rb, per)
    out = np.zeros((h, rb), np.uint8)
    for i in range(per):
        out |= (g[:, :, i] << (8 - bits * (i + 1))).astype(np.uint8)
    return np.ascontiguousarray(_REVERSE[out] if fill_order == 2 else out)


def colormap_payload(colormap: np.ndarray, big_endian: bool) -> bytes:
    cm = np.asarray(colormap, np.uint16).ravel()
    return struct.pack((">" if big_endian else "<") + "H" * cm.size, *[int(x) for x in cm])


def make_tiff(idx: np.ndarray, bits: int, photometric: int = BLACK_IS_ZERO, fill_order: int | None = None,
              colormap: np.ndarray | None = None, big_endian: bool = False, rows_per_strip: int = 16,
              codec: str | None = None, tile: tuple[int, int] | None = None, bigtiff: bool = False) -> bytes:
    """The TIFF of `idx` (h x w values of `bits` bits).  tile = (width,
    height) in pixels: a tiled file (uncompressed, "packbits" or "deflate");
    else strips, through `codec` (None, "lzw", "deflate", "packbits").
    Either way `codec` may be a (bytes -> bytes, Compression value) pair."""
    h, w = idx.shape
    packed = pack_rows(idx, bits, fill_order or 1)
    if tile is not None:
        tw, th = tile
        assert (tw * bits) % 8 == 0 and (codec in (None, "packbits", "deflate") or isinstance(codec, tuple))
        assert not bigtiff
        own = dict(codec=codec[0], compression=codec[1]) if isinstance(codec, tuple) else {}
        tif = im.tiled_tiff_bytes(packed, tile=(tw * bits // 8, th), big_endian=big_endian,
                                  packbits=codec == "packbits", deflate=codec == "deflate", **own)
        tif = im.tiff_set_tag(tif, 322, tw)
    else:
        fn, code = codec if isinstance(codec, tuple) else CODECS[codec]
        writer = im.bigtiff_bytes if bigtiff else im.tiff_bytes
        tif = writer(packed, rows_per_strip=rows_per_strip, big_endian=big_endian, strip_codec=fn, compression=code)
    tif = im.tiff_set_tag(im.tiff_set_tag(im.tiff_set_tag(tif, 256, w), 258, bits), 262, photometric)
    e = ">" if big_endian else "<"
    tags = []
    if fill_order is not None:
        tags.append((266, mf.SHORT, 1, struct.pack(e + "H", fill_order)))
    if colormap is not None:
        tags.append((320, mf.SHORT, 3 << bits, colormap_payload(colormap, big_endian)))
    return mf.add_tags(tif, tags) if tags else tif


def indices(h: int, w: int, bits: int, seed: int) -> np.ndarray:
    """Blocky random values with some noise: every value occurs, runs of
    equal values too (as in line art), and neighbours differ often enough
    that a misplaced pixel shows."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 1 << bits, size=((h + 4) // 5, (w + 6) // 7))
    a = np.kron(coarse, np.ones((5, 7), np.int64))[:h, :w]
    noise = rng.random((h, w)) < 0.2
    a[noise] = rng.integers(0, 1 << bits, size=int(noise.sum()))
    return np.ascontiguousarray(a.astype(np.uint8))


def random_colormap(bits: int, seed: int, wide: bool = True) -> np.ndarray:
    """(3, 2^bits) uint16: 16-bit entries, or (wide=False) none above 255."""
    rng = np.random.default_rng(seed)
    cm = rng.integers(0, 65536 if wide else 256, size=(3, 1 << bits)).astype(np.uint16)
    if wide:
        cm[0, 0] = 0xFF00  # (at least one entry above 255, whatever the draw)
    return cm


WIDTHS = (1, 7, 8, 9, 77, 261)


def grey_matrix():
    """bits x photometric x FillOrder x width; heights that RowsPerStrip (16)
    does not divide; byte order alternating.  FillOrder 1 is stated by the
    tag in every other case and left to the default in the rest."""
    out = []
    k = 0
    for bits in (1, 2, 4):
        for photo in (BLACK_IS_ZERO, WHITE_IS_ZERO):
            for fill in (1, 2):
                for w in WIDTHS:
                    h = 37 + (k % 3) * 5  # 37, 42, 47
                    out.append(dict(id=f"g{bits}_{'w0' if photo == WHITE_IS_ZERO else 'b0'}_f{fill}_w{w}_"
                                       f"{'be' if k % 2 else 'le'}",
                                    bits=bits, photometric=photo, h=h, w=w, seed=100 + k,
                                    kw=dict(fill_order=(fill if fill == 2 or k % 4 < 2 else None),
                                            big_endian=bool(k % 2), rows_per_strip=16)))
                    k += 1
    return out


def palette_matrix():
    """Palettes of 1, 2, 4 and 8 bits, 16-bit maps in both byte orders, and
    one map without an entry above 255 (the 8-bit-map rule)."""
    out = []
    k = 0
    for bits in (1, 2, 4, 8):
        for be in (False, True):
            w = (77, 261, 9, 7)[k % 4]
            out.append(dict(id=f"p{bits}_{'be' if be else 'le'}_w{w}", bits=bits, photometric=PALETTE, h=41, w=w,
                            seed=300 + k, cmap_seed=400 + k, wide=True,
                            kw=dict(big_endian=be, rows_per_strip=16, fill_order=(2 if bits < 8 and k % 3 == 0 else None))))
            k += 1
    out.append(dict(id="p4_8bit_map", bits=4, photometric=PALETTE, h=41, w=77, seed=350, cmap_seed=450, wide=False,
                    kw=dict(rows_per_strip=16)))
    out.append(dict(id="p8_8bit_map_be", bits=8, photometric=PALETTE, h=41, w=77, seed=351, cmap_seed=451, wide=False,
                    kw=dict(rows_per_strip=16, big_endian=True)))
    return out


def decoder_cases():
    """Decoders in front of the expansion: strips through LZW, Deflate and
    PackBits, tiles with ragged right and bottom edges, one BigTIFF."""
    out = []
    for codec in ("lzw", "deflate", "packbits"):
        out.append(dict(id=f"g1_{codec}", bits=1, photometric=WHITE_IS_ZERO, h=75, w=261, seed=500,
                        kw=dict(codec=codec, rows_per_strip=16)))
        out.append(dict(id=f"p4_{codec}", bits=4, photometric=PALETTE, h=75, w=77, seed=501, cmap_seed=601, wide=True,
                        kw=dict(codec=codec, rows_per_strip=16, big_endian=codec == "deflate")))
    for tile in ((32, 48), (16, 16)):
        for codec in (None, "packbits", "deflate"):
            name = f"{tile[0]}x{tile[1]}_{codec or 'raw'}"
            out.append(dict(id=f"g1_tiles{name}", bits=1, photometric=BLACK_IS_ZERO, h=70, w=90, seed=510,
                            kw=dict(tile=tile, codec=codec, fill_order=2 if codec is None else None)))
            out.append(dict(id=f"p8_tiles{name}", bits=8, photometric=PALETTE, h=70, w=90, seed=511, cmap_seed=611,
                            wide=True, kw=dict(tile=tile, codec=codec, big_endian=tile == (16, 16))))
    out.append(dict(id="g4_tiles32x48_w0", bits=4, photometric=WHITE_IS_ZERO, h=70, w=90, seed=512,
                    kw=dict(tile=(32, 48))))
    out.append(dict(id="g1_bigtiff", bits=1, photometric=WHITE_IS_ZERO, h=53, w=261, seed=520,
                    kw=dict(bigtiff=True, rows_per_strip=16)))
    out.append(dict(id="g2_bigtiff_lzw", bits=2, photometric=BLACK_IS_ZERO, h=53, w=77, seed=521,
                    kw=dict(bigtiff=True, codec="lzw", rows_per_strip=16)))
    return out


def build(case):
    """(tiff bytes, expected pixels, indices, colormap or None) of a case."""
    idx = indices(case["h"], case["w"], case["bits"], case["seed"])
    cm = random_colormap(case["bits"], case["cmap_seed"], case["wide"]) if case["photometric"] == PALETTE else None
    tif = make_tiff(idx, case["bits"], case["photometric"], colormap=cm, **case["kw"])
    return tif, expand(idx, case["bits"], case["photometric"], cm), idx, cm


ALL_CASES = grey_matrix() + palette_matrix() + decoder_cases()
