"""TIFF Orientation (tag 274) without a GPU: what the eight values mean
(orientation_cases.upright against Pillow), the tag reader, the upright size,
the stored rows a band of upright rows is made from, the setters' refusals,
the file header of a turned source, and csrc/orient_map.h -- the one place
the kernel and the host take the mapping from -- on the CPU under ASan / UBSan
(tests/host/test_orient_map.cpp)."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import imaging as im
import jp2hip
import metadata_fixtures as mf
import orientation_cases as oc
from jp2hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("o", oc.VALUES)
@pytest.mark.parametrize("form", ["grey8", "rgb8"])
def test_upright_is_what_pillow_shows(o, form):
    from PIL import Image, ImageOps
    px = oc.pixels(form, 37, 52)
    shown = ImageOps.exif_transpose(Image.open(io.BytesIO(oc.tag(oc.form_tiff(form, px), o))))
    assert np.array_equal(np.array(shown), oc.upright(px, o))
    assert oc.upright(px, o).shape[:2] == ((52, 37) if o >= 5 else (37, 52))


WRITERS = {"classic_le": lambda px: im.tiff_bytes(px, rows_per_strip=16),
           "classic_be": lambda px: im.tiff_bytes(px, rows_per_strip=16, big_endian=True),
           "big_le": lambda px: im.bigtiff_bytes(px, rows_per_strip=16),
           "big_be": lambda px: im.bigtiff_bytes(px, rows_per_strip=16, big_endian=True)}


@pytest.mark.parametrize("writer", sorted(WRITERS))
def test_tiff_orientation_reads_the_tag(writer):
    tif = WRITERS[writer](oc.pixels("rgb8", 20, 30))
    assert jp2hip.tiff_orientation(tif) == 1  # absent
    for o in oc.VALUES:
        assert jp2hip.tiff_orientation(oc.tag(tif, o)) == o
    for bad in (0, 9, 65535):
        assert jp2hip.tiff_orientation(oc.tag(tif, bad)) == 1
    assert jp2hip.tiff_orientation(oc.tag(tif, 6, typ=mf.LONG)) == 1   # the wrong type
    assert jp2hip.tiff_orientation(oc.tag(tif, 6, count=2)) == 1       # two values
    outside = mf.add_tags(tif, [(oc.ORIENTATION, mf.SHORT, 1 << 20, None, len(tif) + 4096)])
    assert jp2hip.tiff_orientation(outside) == 1
    # a bad tag never fails the parse: the layout is the untagged file's
    lay, _ = jp2hip.tiff_layout(oc.tag(tif, 9))
    assert (lay.width, lay.height) == (30, 20)


def test_tiff_orientation_of_no_tiff():
    for data in (b"", b"II", b"PNG\r\n\x1a\n" * 4, b"II+\0" + bytes(20), b"MM\0\x2b\0\x04\0\0" + bytes(16)):
        with pytest.raises(jp2hip.Jp2hipError, match="TIFF"):
            jp2hip.tiff_orientation(data)
    # a TIFF whose IFD lies outside the file is still a TIFF: no tag to read
    assert jp2hip.tiff_orientation(b"II*\0" + struct.pack("<I", 1 << 20)) == 1


def test_oriented_size_and_source_rows_follow_the_model():
    for o in (0,) + oc.VALUES:
        for h, w in ((1, 1), (5, 9), (64, 65), (900, 77)):
            idx = np.arange(h * w).reshape(h, w)
            up = oc.upright(idx, max(o, 1))
            assert jp2hip.oriented_size(w, h, o) == (up.shape[1], up.shape[0])
            oh = up.shape[0]
            for r0, r1 in ((0, oh), (0, 1), (oh - 1, oh), (oh // 3, oh // 3 + max(1, oh // 2))):
                r1 = min(r1, oh)
                rows = up[r0:r1] // w  # the stored row of every pixel of the band
                assert jp2hip.orientation_source_rows(h, w, o, r0, r1) == (int(rows.min()), int(rows.max()) + 1)
            s0, s1 = jp2hip.orientation_source_rows(h, w, o, oh, oh)
            assert s0 == s1
    for bad in (-1, 9, 10):
        with pytest.raises(jp2hip.Jp2hipError, match=str(bad)):
            jp2hip.oriented_size(4, 4, bad)
        with pytest.raises(jp2hip.Jp2hipError, match=str(bad)):
            jp2hip.orientation_source_rows(4, 4, bad, 0, 4)


def test_setters_refuse_other_values():
    L = _lib.lib()
    from jp2hip import batch as jb
    jb._bind()
    for bad in (10, -1, 99):
        assert L.jp2hip_set_source_orientation(None, bad) < 0
        assert str(bad) in _lib.last_error() and "JP2HIP_ORIENT_TIFF" in _lib.last_error()
    for ok in (jp2hip.ORIENT_OFF, 1, 6, 8, jp2hip.ORIENT_TIFF):  # the value passes; there is no context
        assert L.jp2hip_set_source_orientation(None, ok) < 0
        assert _lib.last_error() == "null context"
    assert L.jp2hip_batch_set_source_orientation(None, 6) < 0
    assert (jp2hip.ORIENT_OFF, jp2hip.ORIENT_TIFF) == (0, 9)


def test_header_of_a_turned_source_is_the_swapped_layouts():
    """The bytes in front of the code-stream for orientation 6: ihdr has the
    upright height and width, resc the resolutions exchanged; colr and cdef
    are the stored file's."""
    px = oc.pixels("rgba8", 40, 90)
    tif = mf.tag_source(im.tiff_bytes(px, rows_per_strip=16, alpha=1), icc=mf.icc_profile(), xres=(300, 1),
                        yres=(7200, 13), unit=2)
    lay, _ = jp2hip.tiff_layout(oc.tag(tif, 6))
    stored = jp2hip.file_header(lay, jp2hip.FORMAT_JPX, 1000)
    turned = jp2hip.file_header(oc.oriented_layout(lay, 6), jp2hip.FORMAT_JPX, 1000)
    a, b = dict(mf.jp2h_boxes(stored)), dict(mf.jp2h_boxes(turned))
    assert struct.unpack(">II", a[b"ihdr"][:8]) == (40, 90) and struct.unpack(">II", b[b"ihdr"][:8]) == (90, 40)
    assert a[b"ihdr"][8:] == b[b"ihdr"][8:] and a[b"colr"] == b[b"colr"] and a[b"cdef"] == b[b"cdef"]
    v, h = mf.resc_fields(stored), mf.resc_fields(turned)
    assert (v[0], v[1], v[4]) == (h[2], h[3], h[5]) and (v[2], v[3], v[5]) == (h[0], h[1], h[4])
    assert (v[0], v[1], v[4]) != (v[2], v[3], v[5])
    # 2, 3, 4 keep the stored header
    assert jp2hip.file_header(oc.oriented_layout(lay, 3), jp2hip.FORMAT_JPX, 1000) == stored


def test_orient_map_on_cpu(tmp_path):
    csrc = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc")
    exe = str(tmp_path / "test_orient_map")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", csrc, os.path.join(ROOT, "tests", "host", "test_orient_map.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ORIENT MAP OK")
