"""Bilevel, 2- / 4-bit grey and palette-colour TIFFs, on the CPU: the
expectation the GPU tests compare against agrees with a second reader
(Pillow), and jp2hip.tiff_layout describes these files -- or refuses them,
each for its own reason.  No device is needed."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import imaging as im
import jp2hip
import metadata_fixtures as mf
import pixel_format_cases as pf
from jp2hip import _lib

PHOTO = {pf.BLACK_IS_ZERO: _lib.PHOTO_DEFAULT, pf.WHITE_IS_ZERO: _lib.PHOTO_WHITE_IS_ZERO,
         pf.PALETTE: _lib.PHOTO_PALETTE}


@pytest.mark.parametrize("case", pf.ALL_CASES, ids=[c["id"] for c in pf.ALL_CASES])
def test_expectation_equals_pillow_and_layout_describes_the_file(case):
    tif, want, idx, cm = pf.build(case)
    palette = case["photometric"] == pf.PALETTE
    pil_tif = tif
    if palette and case["kw"].get("fill_order") == 2:
        # Pillow has no raw mode for bit-reversed palette indices: it reads the
        # FillOrder 1 twin of the file (what FillOrder 2 means is pinned by the
        # grey cases, which Pillow does read)
        pil_tif = pf.make_tiff(idx, case["bits"], pf.PALETTE, colormap=cm, **dict(case["kw"], fill_order=1))
        assert pil_tif != tif
    if palette and not case["wide"]:
        # Pillow always takes an entry's high byte; libtiff's checkcmap rule
        # (no entry above 255: the entries are 8-bit values) is the encoder's.
        # Pillow reads the twin whose entries are those values scaled to 16 bits.
        pil_tif = pf.make_tiff(idx, case["bits"], pf.PALETTE, colormap=cm * 257, **case["kw"])
        assert cm.max() <= 255
    seen = np.asarray(Image.open(io.BytesIO(pil_tif)).convert("RGB" if palette else "L"))
    assert np.array_equal(seen, want)
    lay, offs = jp2hip.tiff_layout(tif)
    kw, bits = case["kw"], case["bits"]
    assert (lay.width, lay.height, lay.components, lay.bits) == (case["w"], case["h"], 1, bits)
    assert lay.photometric == PHOTO[case["photometric"]]
    assert lay.fill_order == (0 if bits == 8 else (kw.get("fill_order") or 1))
    assert lay.big_endian == (1 if kw.get("big_endian") else 0)
    assert jp2hip.encoded_format(lay) == ((3, 8) if palette else (1, 8))
    assert lay.colormap_entries == (3 << bits if palette else 0)
    assert lay.colormap_bytes() == (pf.colormap_payload(cm, bool(kw.get("big_endian"))) if palette else b"")
    # the units and where they lie: uncompressed ones hold the packed rows
    packed = pf.pack_rows(idx, bits, kw.get("fill_order") or 1)
    rb = packed.shape[1]
    assert rb == (case["w"] * bits + 7) // 8
    codec_tag = {None: 1, "lzw": 5, "deflate": 8, "packbits": 32773}[kw.get("codec")]
    assert lay.compression == codec_tag
    if kw.get("tile"):
        tw, th = kw["tile"]
        assert (lay.tile_width, lay.tile_height) == (tw, th)
        assert lay.nstrips == -(-case["w"] // tw) * -(-case["h"] // th)
        unit = th * tw * bits // 8
        sizes = [lay.strip_bytes[i] for i in range(lay.nstrips)]
        if codec_tag == 1:
            assert sizes == [unit] * lay.nstrips
            o = lay.strip_offsets[0]
            first = np.frombuffer(tif[o:o + unit], np.uint8).reshape(th, tw * bits // 8)
            n = min(rb, tw * bits // 8)
            assert np.array_equal(first[:min(th, case["h"]), :n], packed[:th, :n])
    else:
        rps = min(kw["rows_per_strip"], case["h"])
        assert lay.rows_per_strip == rps and lay.nstrips == -(-case["h"] // rps)
        if codec_tag == 1:
            for s in range(lay.nstrips):
                o, rows = lay.strip_offsets[s], min(rps, case["h"] - s * rps)
                assert tif[o:o + rows * rb] == packed[s * rps:s * rps + rows].tobytes()
        else:
            assert all(lay.strip_bytes[s] > 0 for s in range(lay.nstrips))


def _plain(w, h, nc):
    lay = _lib.Layout()
    lay.width, lay.height, lay.components, lay.bits, lay.planar = w, h, nc, 8, 1
    return lay


@pytest.mark.parametrize("fmt", [jp2hip.FORMAT_JP2, jp2hip.FORMAT_JPX])
def test_file_header_is_the_encoded_formats(fmt):
    """ihdr and colr describe what the code-stream carries: a palette file's
    header is the plain 3 x 8 header of that size, a bilevel file's the plain
    1 x 8 one (all-zero new fields: a layout as it always was)."""
    idx = pf.indices(40, 50, 4, 1)
    pal, _ = jp2hip.tiff_layout(pf.make_tiff(idx, 4, pf.PALETTE, colormap=pf.random_colormap(4, 2)))
    assert jp2hip.file_header(pal, fmt, 1234) == jp2hip.file_header(_plain(50, 40, 3), fmt, 1234)
    bil, _ = jp2hip.tiff_layout(pf.make_tiff(idx & 1, 1, pf.WHITE_IS_ZERO))
    assert jp2hip.file_header(bil, fmt, 1234) == jp2hip.file_header(_plain(50, 40, 1), fmt, 1234)
    assert jp2hip.file_header(_plain(50, 40, 3), fmt, 1234) != jp2hip.file_header(_plain(50, 40, 1), fmt, 1234)
    assert jp2hip.encoded_format(_plain(50, 40, 4)) == (4, 8)
    img16, _ = jp2hip.tiff_layout(im.tiff_bytes(im.synth_u16(8, 8, comps=1)))
    assert jp2hip.encoded_format(img16) == (1, 16)


def test_icc_profile_is_classified_against_the_encoded_components():
    """A palette file with an RGB display profile: the profile fits the three
    encoded components (it would not fit the one index component)."""
    idx = pf.indices(20, 30, 8, 3)
    icc = mf.icc_profile()
    tif = mf.tag_source(pf.make_tiff(idx, 8, pf.PALETTE, colormap=pf.random_colormap(8, 4)), icc=icc)
    lay, _ = jp2hip.tiff_layout(tif)
    rgb = _plain(30, 20, 3)
    rgb.set_icc_profile(icc)
    hdr = jp2hip.file_header(lay, jp2hip.FORMAT_JP2, 99)
    assert hdr == jp2hip.file_header(rgb, jp2hip.FORMAT_JP2, 99)
    (colr,) = [b for t, b in mf.jp2h_boxes(hdr) if t == b"colr"]
    assert colr[0] == 2 and colr[3:] == icc  # METH 2: the restricted profile itself


def test_band_layout_carries_the_pixel_format():
    from jp2hip import split as js
    idx = pf.indices(100, 77, 4, 5)
    cm = pf.random_colormap(4, 6)
    for kw in (dict(), dict(codec="lzw"), dict(tile=(32, 48))):
        tif = pf.make_tiff(idx, 4, pf.PALETTE, colormap=cm, fill_order=2, big_endian=True, **kw)
        lay, offs = jp2hip.tiff_layout(tif)
        buf, blay, keep = js.band_strips(tif, lay, offs, 32, 64)
        for name in ("photometric", "fill_order", "colormap_entries", "bits", "components", "big_endian"):
            assert getattr(blay, name) == getattr(lay, name), name
        assert blay.colormap_bytes() == lay.colormap_bytes() == pf.colormap_payload(cm, True)
        if not kw:  # uncompressed strips: the band's packed rows, back to back (rows 32..63: strips 2 and 3)
            assert buf == pf.pack_rows(idx, 4, 2)[32:64].tobytes()
            assert [blay.strip_offsets[i] for i in (2, 3)] == [0, 16 * 39]
    assert set(_lib.Layout.PIXEL_FORMAT) == {"photometric", "fill_order", "colormap", "colormap_entries"}
    assert all(n in dict(_lib.Layout._fields_) for n in _lib.Layout.PIXEL_FORMAT)


def _grey(bits=1, photo=pf.BLACK_IS_ZERO, **kw):
    return pf.make_tiff(pf.indices(20, 33, bits, 7), bits, photo, **kw)


def _palette(bits=4, **kw):
    return pf.make_tiff(pf.indices(20, 33, bits, 8), bits, pf.PALETTE, colormap=pf.random_colormap(bits, 9), **kw)


def _drop(tif, tag):
    return mf.add_tags(tif, [], drop=(tag,))


REFUSED = {
    "subbyte_two_samples": (lambda: im.tiff_set_tag(_grey(4), 277, 2), r"4 bits/sample with 2 samples/pixel"),
    "bits_3": (lambda: im.tiff_set_tag(_grey(4), 258, 3), r"3 bits/sample is not supported"),
    "bits_12": (lambda: im.tiff_set_tag(_grey(4), 258, 12), r"12 bits/sample is not supported"),
    "predictor_below_8_bits": (lambda: mf.add_tags(_grey(4, codec="lzw"), [(317, mf.SHORT, 1, struct.pack("<H", 2))]),
                               r"predictor 2 with 4 bits/sample"),
    "palette_without_colormap": (lambda: _drop(_palette(), 320), r"Photometric.*without a ColorMap"),
    "palette_short_colormap": (lambda: mf.add_tags(_drop(_palette(), 320),
                                                   [(320, mf.SHORT, 3 * 8, b"\1\2" * 24)]),
                               r"Photometric.*ColorMap must be 3 \* 2\^4 SHORTs"),
    "palette_long_colormap": (lambda: mf.add_tags(_drop(_palette(2), 320), [(320, mf.SHORT, 3 * 16, b"\1\2" * 48)]),
                              r"Photometric.*ColorMap must be 3 \* 2\^2 SHORTs"),
    "palette_16bit_indices": (lambda: mf.add_tags(im.tiff_set_tag(im.tiff_bytes(im.synth_u16(8, 8, comps=1)), 262, 3),
                                                  [(320, mf.SHORT, 3 * 256, b"\0\1" * 768)]),
                              r"Photometric.*16-bit indices"),
    "palette_two_samples": (lambda: im.tiff_set_tag(_palette(8), 277, 2), r"Photometric.*1 sample/pixel"),
    "white_is_zero_8bit": (lambda: im.tiff_set_tag(im.tiff_bytes(im.synth_rgb8(8, 8)[..., 0].copy()), 262, 0),
                           r"WhiteIsZero"),
    "white_is_zero_16bit": (lambda: im.tiff_set_tag(im.tiff_bytes(im.synth_u16(8, 8, comps=1)), 262, 0),
                            r"WhiteIsZero"),
    "cmyk": (lambda: im.tiff_set_tag(im.tiff_bytes(np.zeros((8, 8, 4), np.uint8)), 262, 5), r"PhotometricInterpretation 5"),
    "ycbcr": (lambda: im.tiff_set_tag(im.tiff_bytes(im.synth_rgb8(8, 8)), 262, 6), r"PhotometricInterpretation 6"),
    "lab": (lambda: im.tiff_set_tag(im.tiff_bytes(im.synth_rgb8(8, 8)), 262, 8), r"PhotometricInterpretation 8"),
    "jpeg": (lambda: im.tiff_set_tag(_grey(4), 259, 7), r"compression 7"),
    "ccitt_g4": (lambda: im.tiff_set_tag(_grey(1), 259, 4), r"compression 4"),
    "fill_order_3": (lambda: _grey(1, fill_order=3), r"FillOrder 3"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_tiff_layout_refuses(name):
    make, msg = REFUSED[name]
    with pytest.raises(jp2hip.Jp2hipError, match=msg):
        jp2hip.tiff_layout(make())


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_short_strip_is_refused(bits):
    """A strip must hold rows * ceil(w * bits / 8) bytes: one byte less, by
    its byte count or by the end of the file, is refused."""
    idx = pf.indices(20, 33, bits, 11)
    tif = pf.make_tiff(idx, bits, rows_per_strip=20)
    need = 20 * ((33 * bits + 7) // 8)
    lay, _ = jp2hip.tiff_layout(tif)
    assert lay.nstrips == 1 and lay.strip_offsets[0] + need == len(tif)
    with pytest.raises(jp2hip.Jp2hipError, match="strip byte count too small"):
        jp2hip.tiff_layout(im.tiff_set_tag(tif, 279, need - 1))
    with pytest.raises(jp2hip.Jp2hipError, match="out of range"):
        jp2hip.tiff_layout(tif[:-1])
    # and the size the 8-bit reading of the same width would ask for is not demanded
    assert need < 20 * 33


def test_short_tile_is_refused():
    idx = pf.indices(40, 50, 1, 12)
    tif = pf.make_tiff(idx, 1, tile=(32, 48))
    lay, _ = jp2hip.tiff_layout(tif)
    assert [lay.strip_bytes[i] for i in range(2)] == [48 * 4] * 2
    with pytest.raises(jp2hip.Jp2hipError, match="tile byte count too small"):
        jp2hip.tiff_layout(_shrink_first_count(tif))


def _shrink_first_count(tif):
    """TileByteCounts lives out of line (several tiles): lower its first value by one."""
    e = mf.byte_order(tif)
    ifd = struct.unpack(e + "I", tif[4:8])[0]
    n = struct.unpack(e + "H", tif[ifd:ifd + 2])[0]
    for i in range(n):
        p = ifd + 2 + 12 * i
        tag, typ, cnt, off = struct.unpack(e + "HHII", tif[p:p + 12])
        if tag == 325:
            assert typ == 4 and cnt > 1
            v = struct.unpack(e + "I", tif[off:off + 4])[0]
            return tif[:off] + struct.pack(e + "I", v - 1) + tif[off + 4:]
    raise KeyError(325)


@pytest.mark.parametrize("where", ["past_the_end", "straddles_the_end", "count_too_large"])
def test_colormap_is_never_read_out_of_bounds(where):
    """A ColorMap entry whose count or offset lies about the file: refused
    (the message names the photometric form), never followed."""
    base = _drop(_palette(8), 320)
    n = 3 * 256
    if where == "past_the_end":
        tif = mf.add_tags(base, [(320, mf.SHORT, n, None, len(base) + 4096)])
    elif where == "straddles_the_end":
        tif = mf.add_tags(base, [(320, mf.SHORT, n, None, 0)])
        tif = _repoint(tif, 320, len(tif) - 2 * n + 2)
    else:
        tif = mf.add_tags(base, [(320, mf.SHORT, 1 << 30, None, 8)])
    with pytest.raises(jp2hip.Jp2hipError, match="Photometric"):
        jp2hip.tiff_layout(tif)


def _repoint(tif, tag, offset):
    e = mf.byte_order(tif)
    ifd = struct.unpack(e + "I", tif[4:8])[0]
    n = struct.unpack(e + "H", tif[ifd:ifd + 2])[0]
    for i in range(n):
        p = ifd + 2 + 12 * i
        if struct.unpack(e + "H", tif[p:p + 2])[0] == tag:
            return tif[:p + 8] + struct.pack(e + "I", offset) + tif[p + 12:]
    raise KeyError(tag)


def test_colormap_at_the_very_end_of_the_file_is_read_whole():
    """The last byte of the file is the map's last byte: accepted, and the
    copy the Layout keeps is exactly the tag's data."""
    base = _drop(_palette(2), 320)
    cm = pf.random_colormap(2, 21)
    payload = pf.colormap_payload(cm, False)
    tif = mf.add_tags(base, [(320, mf.SHORT, 12, None, 0)])
    tif = _repoint(tif, 320, len(tif)) + payload
    lay, _ = jp2hip.tiff_layout(tif)
    assert lay.colormap_bytes() == payload
