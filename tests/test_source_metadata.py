"""What a TIFF states about its pixels -- ICC profile, ExtraSamples,
resolution -- carried into the JP2 / JPX file header, on the CPU: the parse
(jp2hip_tiff_layout) and the header writer (jp2hip_file_header, the function
every encode route calls).  The code-stream is not involved; the GPU routes
are in test_gpu_source_metadata.py.

The reference's Kakadu reads these tags through libtiff (Dockerfile:15-17)
and leaves -jp2_alpha off (KakaduConverter.java:46), so alpha follows what
the TIFF declares."""
import io
import struct
from fractions import Fraction

import numpy as np
import pytest

import imaging as im
import jp2hip
import metadata_fixtures as mf
import oracle_lib as ol
from jp2hip._lib import Layout

JP2, JPX, J2K = jp2hip.FORMAT_JP2, jp2hip.FORMAT_JPX, jp2hip.FORMAT_J2K
ENUM_RGB = bytes([1, 0, 0, 0, 0, 0, 16])   # colr payload: METH 1, PREC 0, APPROX 0, EnumCS sRGB
ENUM_GREY = bytes([1, 0, 0, 0, 0, 0, 17])
RES_BOUND = 7.7e-5                          # 0.5 / 6553.5, the rounding rule's relative error


def layout(nc, bits=8, w=24, h=20, icc=None, **meta):
    lay = Layout(w, h, nc, bits)
    for k, v in meta.items():
        setattr(lay, k, v)
    if icc is not None:
        lay.set_icc_profile(icc)
    return lay


def header(nc, fmt, **kw):
    return jp2hip.file_header(layout(nc, **kw), fmt, 1000)


def colr_boxes(hdr):
    return [b for t, b in mf.jp2h_boxes(hdr) if t == b"colr"]


def source_image(nc, bits):
    img = im.synth_rgb8(20, 24, seed=5) if bits == 8 else im.synth_u16(20, 24, comps=3, seed=5)
    if nc == 1:
        return np.ascontiguousarray(img[..., 0])
    if nc == 2:
        return np.ascontiguousarray(img[..., :2])
    if nc == 4:
        return np.ascontiguousarray(np.dstack([img, img[..., :1]]))
    return img


# ---------------------------------------------------------------- the parse

def _tiff(kind, big_endian, img, **kw):
    if kind == "classic":
        return im.tiff_bytes(img, rows_per_strip=8, big_endian=big_endian, **kw)
    return im.bigtiff_bytes(img, rows_per_strip=8, big_endian=big_endian)


KINDS = [(k, be) for k in ("classic", "bigtiff") for be in (False, True)]


@pytest.mark.parametrize("kind,big_endian", KINDS)
def test_tiff_layout_reads_the_metadata_tags(kind, big_endian):
    img = source_image(3, 8)
    icc = mf.icc_profile(slack=3)
    tif = mf.tag_source(_tiff(kind, big_endian, img), icc=icc, xres=(300, 1), yres=(7200, 25), unit=3)
    lay, keep = jp2hip.tiff_layout(tif)
    assert (lay.width, lay.height, lay.components, lay.bits) == (24, 20, 3, 8)
    assert lay.big_endian == int(big_endian)
    assert (lay.res_unit, lay.xres_num, lay.xres_den, lay.yres_num, lay.yres_den) == (3, 300, 1, 7200, 25)
    assert lay.icc_bytes == len(icc)
    assert bytes(lay.icc[i] for i in range(len(icc))) == icc and lay.icc_profile() == icc
    assert lay.extra_samples == 0
    # the strips are still where they were
    o = lay.strip_offsets[0]
    assert tif[o:o + 3] == img[0, 0].tobytes()


def test_tiff_layout_without_metadata_tags_is_all_zero():
    lay, _ = jp2hip.tiff_layout(im.tiff_bytes(source_image(3, 8)))
    assert [getattr(lay, f) for f in Layout.METADATA] == [0] * 6
    assert not lay.icc and lay.icc_bytes == 0 and lay.icc_profile() == b""


def test_layout_keeps_its_profile_alive():
    """tiff_layout's callers drop everything but the Layout."""
    import gc
    icc = mf.icc_profile()
    lay = jp2hip.tiff_layout(mf.tag_source(im.tiff_bytes(source_image(3, 8)), icc=icc))[0]
    gc.collect()
    junk = [bytes(len(icc)) for _ in range(64)]  # reuse freed blocks of that size
    assert lay.icc_profile() == icc
    del junk


@pytest.mark.parametrize("kind,big_endian", KINDS)
@pytest.mark.parametrize("value,want", [(0, 1), (1, 2), (2, 3), (None, 0), (7, 1)])
def test_extra_samples(kind, big_endian, value, want):
    """ExtraSamples 0 / 1 / 2 -> 1 / 2 / 3, absent -> 0, an unknown value counts as 0."""
    img = source_image(4, 8)
    e = ">" if big_endian else "<"
    tif = mf.add_tags(_tiff(kind, big_endian, img), [] if value is None else
                      [(mf.EXTRA, mf.SHORT, 1, struct.pack(e + "H", value))], drop={mf.EXTRA})
    lay, _ = jp2hip.tiff_layout(tif)
    assert lay.components == 4 and lay.extra_samples == want


def test_extra_samples_from_the_fixture_writer():
    for alpha, want in ((None, 3), (0, 1), (1, 2), (2, 3)):
        assert jp2hip.tiff_layout(im.tiff_bytes(source_image(4, 8), alpha=alpha))[0].extra_samples == want
    assert jp2hip.tiff_layout(im.tiff_bytes(source_image(2, 8)))[0].extra_samples == 3


@pytest.mark.parametrize("xres,yres,unit,want", [
    ((300, 1), (300, 1), None, (2, 300, 1, 300, 1)),      # ResolutionUnit absent: inch
    ((300, 1), (300, 1), 2, (2, 300, 1, 300, 1)),
    ((1181, 10), (1180, 10), 3, (3, 1181, 10, 1180, 10)),
    ((300, 1), (300, 1), 1, (1, 300, 1, 300, 1)),         # "none": recorded, no res box (below)
    ((300, 1), (300, 1), 9, (0, 0, 0, 0, 0)),
    ((300, 0), (300, 1), 2, (0, 0, 0, 0, 0)),             # zero denominator
    ((300, 1), (0, 1), 2, (0, 0, 0, 0, 0)),               # zero numerator
    ((300, 1), None, 2, (0, 0, 0, 0, 0)),                 # one axis only
])
def test_resolution_tags(xres, yres, unit, want):
    tif = mf.tag_source(im.tiff_bytes(source_image(1, 8), big_endian=True), xres=xres, yres=yres, unit=unit)
    lay, _ = jp2hip.tiff_layout(tif)
    assert (lay.res_unit, lay.xres_num, lay.xres_den, lay.yres_num, lay.yres_den) == want
    has_res = mf.resc_fields(jp2hip.file_header(lay, JPX, 10)) is not None
    assert has_res == (want[0] in (2, 3))


@pytest.mark.parametrize("kind,big_endian", KINDS)
def test_out_of_range_metadata_tags_are_absent(kind, big_endian):
    """A metadata tag whose data runs past the file (or has the wrong type)
    counts as absent; the parse still succeeds and the other tags hold."""
    img = source_image(3, 8)
    e = ">" if big_endian else "<"
    base = _tiff(kind, big_endian, img)
    n = len(base)
    icc = mf.icc_profile()
    good_res = [(mf.XRES, mf.RATIONAL, 1, mf.rational(e, 72, 1)), (mf.YRES, mf.RATIONAL, 1, mf.rational(e, 72, 1))]
    # profile past the end (the new IFD adds < 400 bytes), resolution fine
    lay, _ = jp2hip.tiff_layout(mf.add_tags(base, [(mf.ICC, mf.UNDEFINED, len(icc), None, n + 400)] + good_res))
    assert not lay.icc and lay.icc_bytes == 0
    assert (lay.res_unit, lay.xres_num, lay.yres_num) == (2, 72, 72)
    # profile that starts inside the file and ends past it; one that ends with the file is read
    tif = mf.add_tags(base, [(mf.ICC, mf.UNDEFINED, 5000, None, n - 100)])
    lay, _ = jp2hip.tiff_layout(tif)
    assert not lay.icc and lay.icc_bytes == 0
    tif = mf.add_tags(base, [(mf.ICC, mf.UNDEFINED, 5000, None, n - 100)])
    fits = len(tif) - (n - 100)
    for count, ok in ((fits, True), (fits + 1, False)):
        tif = mf.add_tags(base, [(mf.ICC, mf.UNDEFINED, count, None, n - 100)])
        assert len(tif) == n - 100 + fits
        lay, _ = jp2hip.tiff_layout(tif)
        assert lay.icc_bytes == (count if ok else 0) and lay.icc_profile() == (tif[n - 100:] if ok else b"")
    # a huge count must not wrap the bounds check
    lay, _ = jp2hip.tiff_layout(mf.add_tags(base, [(mf.ICC, mf.UNDEFINED, 0xFFFFFFFF, None, 8)]))
    assert not lay.icc and lay.icc_bytes == 0
    # wrong type for a profile
    lay, _ = jp2hip.tiff_layout(mf.add_tags(base, [(mf.ICC, mf.SHORT, len(icc) // 2, icc)]))
    assert not lay.icc and lay.icc_bytes == 0
    # a rational past the end (classic: never inline), profile fine
    if kind == "classic":
        lay, _ = jp2hip.tiff_layout(mf.add_tags(base, [(mf.ICC, mf.UNDEFINED, len(icc), icc), good_res[0],
                                                       (mf.YRES, mf.RATIONAL, 1, None, n + 4000)]))
        assert lay.icc_profile() == icc and lay.res_unit == 0 and lay.xres_num == 0
    # a resolution stored as LONG is not a resolution
    lay, _ = jp2hip.tiff_layout(mf.add_tags(base, [good_res[0], (mf.YRES, mf.LONG, 1, struct.pack(e + "I", 72))]))
    assert lay.res_unit == 0
    # ExtraSamples as LONG is absent
    img4 = source_image(4, 8)
    tif4 = mf.add_tags(_tiff(kind, big_endian, img4), [(mf.EXTRA, mf.LONG, 1, struct.pack(e + "I", 1))], drop={mf.EXTRA})
    assert jp2hip.tiff_layout(tif4)[0].extra_samples == 0


def test_pillow_written_tags_parse():
    """What Pillow's libtiff writes for icc_profile= and dpi=."""
    from PIL import Image
    icc = mf.icc_profile()
    b = io.BytesIO()
    Image.fromarray(source_image(3, 8)).save(b, format="TIFF", compression="tiff_lzw", icc_profile=icc, dpi=(300, 150))
    lay, _ = jp2hip.tiff_layout(b.getvalue())
    assert lay.icc_profile() == icc and lay.res_unit == 2
    assert Fraction(lay.xres_num, lay.xres_den) == 300 and Fraction(lay.yres_num, lay.yres_den) == 150


def test_band_layouts_keep_the_files_metadata():
    """Tile-split ranks that upload only their band (jp2hip.split.band_strips)
    describe it with the file's metadata: rank 0 writes the file header."""
    from jp2hip import split as js
    img = im.synth_rgb8(300, 170, seed=2)
    icc = mf.icc_profile()
    for base in (im.tiff_bytes(img, rows_per_strip=7),
                 im.tiff_bytes(img, rows_per_strip=48, strip_codec=im.packbits_encode, compression=32773)):
        tif = mf.tag_source(base, icc=icc, xres=(300, 1), yres=(301, 1), unit=3)
        lay, offs = jp2hip.tiff_layout(tif)
        buf, blay, keep = js.band_strips(tif, lay, offs, 128, 256)
        del lay
        assert [getattr(blay, f) for f in Layout.METADATA] == [0, 3, 300, 1, 301, 1]
        assert blay.icc_profile() == icc
        assert jp2hip.file_header(blay, JPX, 99) == jp2hip.file_header(jp2hip.tiff_layout(tif)[0], JPX, 99)


# ------------------------------------------------------- the unchanged header

@pytest.mark.parametrize("fmt", [JP2, JPX], ids=["jp2", "jpx"])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("nc", [1, 2, 3, 4])
def test_header_without_metadata_is_the_oracles(nc, bits, fmt):
    img = source_image(nc, bits)
    oracle_file = ol.encode(img, ol.recipe(True, format=fmt))
    cs = im.codestream(oracle_file)
    want = oracle_file[:len(oracle_file) - len(cs)]
    assert len(want) > 40
    assert jp2hip.file_header(layout(nc, bits), fmt, len(cs)) == want
    assert jp2hip.file_header(layout(nc, bits, extra_samples=3), fmt, len(cs)) == want
    # an uninterpretable extra_samples is "not stated"
    assert jp2hip.file_header(layout(nc, bits, extra_samples=9), fmt, len(cs)) == want


def test_j2k_has_no_header():
    lay = layout(3, icc=mf.icc_profile(), res_unit=2, xres_num=300, xres_den=1, yres_num=300, yres_den=1)
    assert jp2hip.file_header(lay, J2K, 1000) == b""


def test_file_header_sizes_without_writing():
    lay = layout(3, icc=mf.icc_profile())
    want = jp2hip.file_header(lay, JPX, 77)
    L = jp2hip._lib.lib()
    from ctypes import byref, create_string_buffer
    assert L.jp2hip_file_header(byref(lay), JPX, 77, None, 0) == len(want)
    small = create_string_buffer(b"\xAA" * len(want), len(want))
    assert L.jp2hip_file_header(byref(lay), JPX, 77, small, len(want) - 1) == len(want)
    assert small.raw == b"\xAA" * len(want)  # cap too small: nothing written
    assert L.jp2hip_file_header(None, JPX, 77, None, 0) < 0
    assert L.jp2hip_file_header(byref(lay), 7, 77, None, 0) < 0
    # the jp2c box header ends the bytes and counts the code-stream
    assert want[-8:] == struct.pack(">I4s", 8 + 77, b"jp2c")


# ------------------------------------------------------------ tagged headers

@pytest.mark.parametrize("fmt", [JP2, JPX], ids=["jp2", "jpx"])
@pytest.mark.parametrize("nc,space", [(3, b"RGB "), (4, b"RGB "), (1, b"GRAY"), (2, b"GRAY")])
@pytest.mark.parametrize("cls", [b"mntr", b"scnr"])
def test_restricted_profile_is_one_meth2_colr(nc, space, cls, fmt):
    icc = mf.icc_profile(space=space, cls=cls)
    hdr = header(nc, fmt, icc=icc)
    assert colr_boxes(hdr) == [bytes([2, 0, 0]) + icc]
    kinds = [t for t, _ in mf.jp2h_boxes(hdr)]
    assert kinds == [b"ihdr", b"colr"] + ([b"cdef"] if nc in (2, 4) else [])
    # everything outside jp2h is untouched
    plain = header(nc, fmt)
    i = plain.index(b"jp2h") - 4
    assert hdr[:i] == plain[:i] and hdr[-8:] == plain[-8:]
    assert struct.unpack(">I", hdr[i:i + 4])[0] == struct.unpack(">I", plain[i:i + 4])[0] - 15 + 11 + len(icc)


ANY_PROFILES = {
    "a2b0": dict(tags=mf.RGB_MATRIX_TAGS + (b"A2B0",)),
    "lab_pcs": dict(pcs=b"Lab "),
    "output_class": dict(cls=b"prtr"),
    "no_matrix": dict(tags=(b"rTRC", b"gTRC", b"bTRC", b"desc")),
}


@pytest.mark.parametrize("name", sorted(ANY_PROFILES))
def test_any_profile_is_enumerated_then_meth3_in_jpx_only(name):
    icc = mf.icc_profile(**ANY_PROFILES[name])
    hdr = header(3, JPX, icc=icc)
    assert colr_boxes(hdr) == [ENUM_RGB, bytes([3, 1, 1]) + icc]
    assert [t for t, _ in mf.jp2h_boxes(hdr)] == [b"ihdr", b"colr", b"colr"]
    assert header(3, JP2, icc=icc) == header(3, JP2)  # Part 1 cannot carry it


def test_tag_table_past_the_profile_is_not_restricted():
    icc = bytearray(mf.icc_profile())
    icc[128:132] = struct.pack(">I", 1000)  # tag count far past the profile
    assert colr_boxes(header(3, JPX, icc=bytes(icc))) == [ENUM_RGB, bytes([3, 1, 1]) + bytes(icc)]


def test_grey_any_profile():
    icc = mf.icc_profile(space=b"GRAY", tags=(b"kTRC", b"A2B0"))
    assert colr_boxes(header(1, JPX, icc=icc)) == [ENUM_GREY, bytes([3, 1, 1]) + icc]


@pytest.mark.parametrize("kw,meth", [(dict(), 2), (dict(tags=mf.RGB_MATRIX_TAGS + (b"A2B0",)), 3)])
def test_profile_size_field_below_the_tag_count_embeds_that_many(kw, meth):
    icc = mf.icc_profile(slack=37, **kw)
    S = struct.unpack(">I", icc[:4])[0]
    assert S == len(icc) - 37
    got = colr_boxes(header(3, JPX, icc=icc))[-1]
    assert got[0] == meth and got[3:] == icc[:S]


UNUSABLE = {
    "bad_acsp": (3, mf.icc_profile(magic=b"ascp")),
    "size_past_the_tag": (3, mf.icc_profile(size_field=100000)),
    "size_below_132": (3, mf.icc_profile(size_field=131)),
    "short": (3, mf.icc_profile()[:131]),
    "rgb_profile_grey_image": (1, mf.icc_profile(space=b"RGB ")),
    "grey_profile_rgb_image": (3, mf.icc_profile(space=b"GRAY")),
    "rgb_profile_grey_alpha_image": (2, mf.icc_profile(space=b"RGB ")),
    "cmyk_profile": (4, mf.icc_profile(space=b"CMYK")),
}


@pytest.mark.parametrize("fmt", [JP2, JPX], ids=["jp2", "jpx"])
@pytest.mark.parametrize("name", sorted(UNUSABLE))
def test_unusable_profile_leaves_the_header_alone(name, fmt):
    nc, icc = UNUSABLE[name]
    assert header(nc, fmt, icc=icc) == header(nc, fmt)


def _cdef(hdr):
    got = [b for t, b in mf.jp2h_boxes(hdr) if t == b"cdef"]
    if not got:
        return None
    n = struct.unpack(">H", got[0][:2])[0]
    return [struct.unpack(">HHH", got[0][2 + 6 * i:8 + 6 * i]) for i in range(n)]


@pytest.mark.parametrize("fmt", [JP2, JPX], ids=["jp2", "jpx"])
@pytest.mark.parametrize("nc", [2, 4])
def test_cdef_follows_extra_samples(nc, fmt):
    colour = [(c, 0, c + 1) for c in range(nc - 1)]
    assert _cdef(header(nc, fmt)) == colour + [(nc - 1, 1, 0)]
    assert header(nc, fmt, extra_samples=3) == header(nc, fmt)
    assert _cdef(header(nc, fmt, extra_samples=2)) == colour + [(nc - 1, 2, 0)]  # premultiplied opacity
    assert _cdef(header(nc, fmt, extra_samples=1)) is None
    none = header(nc, fmt, extra_samples=1)
    assert [t for t, _ in mf.jp2h_boxes(none)] == [b"ihdr", b"colr"]
    assert len(none) == len(header(nc, fmt)) - (8 + 2 + 6 * nc)


@pytest.mark.parametrize("nc", [1, 3])
def test_no_cdef_for_one_or_three_channels(nc):
    for es in (0, 1, 2, 3):
        assert _cdef(header(nc, JPX, extra_samples=es)) is None


def _value(n, d, e):
    return Fraction(n, d) * Fraction(10) ** e


RES_CASES = {
    "300dpi": ((300, 1), (300, 1), 2),
    "400_per_cm": ((400, 1), (400, 1), 3),
    "72dpi": ((72, 1), (72, 1), 2),
    "1dpi": ((1, 1), (1, 1), 2),
    "u32_max_per_cm": ((4294967295, 1), (4294967295, 1), 3),
    "unequal": ((300, 1), (600, 1), 2),
    "tiny": ((1, 4294967295), (1, 4000000007), 2),
    "huge_inch": ((4294967295, 1), (4294967291, 3), 2),
    "odd_rational": ((2999999, 10007), (720001, 10001), 3),
}


@pytest.mark.parametrize("name", sorted(RES_CASES))
def test_resc_fields(name):
    (xn, xd), (yn, yd), unit = RES_CASES[name]
    hdr = header(3, JPX, res_unit=unit, xres_num=xn, xres_den=xd, yres_num=yn, yres_den=yd)
    assert [t for t, _ in mf.jp2h_boxes(hdr)] == [b"ihdr", b"colr", b"res "]
    vn, vd, hn, hd, ve, he = mf.resc_fields(hdr)
    for (num, den), (n, d, e) in (((yn, yd), (vn, vd, ve)), ((xn, xd), (hn, hd, he))):  # vertical = Y
        exact = mf.points_per_metre(num, den, unit)
        got = _value(n, d, e)
        assert abs(got - exact) <= Fraction(RES_BOUND) * exact, (float(got), float(exact))
        if exact.numerator <= 65535 and exact.denominator <= 65535:
            assert (n, d, e) == (exact.numerator, exact.denominator, 0)
        else:
            scaled = exact / Fraction(10) ** e
            assert d == 1 and Fraction(13107, 2) <= scaled < Fraction(131071, 2)
            assert n == (scaled + Fraction(1, 2)).__floor__()  # rounded half up


def test_resc_known_values():
    def fields(x, y, unit):
        return mf.resc_fields(header(1, JP2, res_unit=unit, xres_num=x[0], xres_den=x[1], yres_num=y[0], yres_den=y[1]))
    assert fields((300, 1), (300, 1), 2) == (11811, 1, 11811, 1, 0, 0)   # reads back as 299.9994 dpi
    assert fields((400, 1), (400, 1), 3) == (40000, 1, 40000, 1, 0, 0)
    assert fields((72, 1), (72, 1), 2) == (28346, 1, 28346, 1, -1, -1)
    assert fields((1, 1), (1, 1), 2) == (5000, 127, 5000, 127, 0, 0)
    assert fields((4294967295, 1), (4294967295, 1), 3) == (42950, 1, 42950, 1, 7, 7)
    assert fields((300, 1), (600, 1), 2) == (23622, 1, 11811, 1, 0, 0)   # vertical (Y) first


def test_box_order_with_everything():
    icc = mf.icc_profile(tags=mf.RGB_MATRIX_TAGS + (b"A2B0",))
    hdr = header(4, JPX, icc=icc, extra_samples=2, res_unit=3, xres_num=100, xres_den=1, yres_num=100, yres_den=1)
    assert [t for t, _ in mf.jp2h_boxes(hdr)] == [b"ihdr", b"colr", b"colr", b"cdef", b"res "]
    plain = header(4, JPX)
    i = plain.index(b"jp2h") - 4
    assert hdr[:i] == plain[:i]  # signature, ftyp, rreq byte for byte


# -------------------------------------------------------------- decode check

@pytest.fixture(scope="module")
def rgba_case():
    img = source_image(4, 8)
    cs = im.codestream(ol.encode(img, ol.recipe(True)))
    return img, cs


DECODE_CASES = {
    "restricted_jp2": (JP2, dict(icc=mf.icc_profile()), 2),
    "restricted_jpx": (JPX, dict(icc=mf.icc_profile()), 2),
    "any_jpx": (JPX, dict(icc=mf.icc_profile(tags=mf.RGB_MATRIX_TAGS + (b"A2B0",))), 2),
    "associated_alpha": (JPX, dict(), 1),
    "unspecified_extra_sample": (JPX, dict(), 0),
}


@pytest.mark.parametrize("name", sorted(DECODE_CASES))
def test_pillow_decodes_the_tagged_file(rgba_case, name):
    """The header in front of the oracle's code-stream: OpenJPEG (through
    Pillow) decodes the source pixels and reports the TIFF's resolution."""
    from PIL import Image
    img, cs = rgba_case
    fmt, kw, alpha = DECODE_CASES[name]
    tif = mf.tag_source(im.tiff_bytes(img, alpha=alpha), xres=(300, 1), yres=(600, 1), unit=2, **kw)
    lay, _ = jp2hip.tiff_layout(tif)
    assert lay.extra_samples == alpha + 1
    data = jp2hip.file_header(lay, fmt, len(cs)) + cs
    with Image.open(io.BytesIO(data)) as pil:
        dpi = pil.info["dpi"]
        got = np.array(pil)
    assert np.array_equal(got, img)
    assert abs(dpi[0] - 300) <= 1e-4 * 300 and abs(dpi[1] - 600) <= 1e-4 * 600
