"""Bilevel, 2- / 4-bit grey and palette-colour TIFFs on the GPU: every route
a file takes gives exactly the file the oracle encodes from the expanded
8-bit pixels (pixel_format_cases.expand, which test_pixel_formats.py pins to
Pillow).  The sources carry no metadata, so the oracle's own header is the
expected header."""
import threading

import numpy as np
import pytest

import imaging as im
import jp2hip
import oracle_lib as ol
import pixel_format_cases as pf
from jp2hip import split as js

pytestmark = pytest.mark.gpu


def oracle(img, rc):
    return ol.encode(img, ol.copy_recipe(rc))


@pytest.mark.parametrize("case", pf.ALL_CASES, ids=[c["id"] for c in pf.ALL_CASES])
def test_encode_tiff_lossless_matrix(encoder, case):
    tif, want_px, _, _ = pf.build(case)
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    got, _ = encoder.encode_tiff(tif, jp2hip.LOSSLESS, rc)
    assert got == oracle(want_px, rc)


@pytest.fixture(scope="module")
def quantised():
    """synth_rgb8(300, 530) quantised to 256 colours: indices, 16-bit map
    and the RGB pixels the palette file stands for."""
    rgb = im.synth_rgb8(300, 530, seed=3)
    idx = ((rgb[..., 0] >> 5).astype(np.uint8) << 5) | ((rgb[..., 1] >> 5) << 2) | (rgb[..., 2] >> 6)
    k = np.arange(256)
    cm = np.stack([(k >> 5) * 36 + 2, ((k >> 2) & 7) * 36 + 1, (k & 3) * 85]).astype(np.uint16) * 257
    return np.ascontiguousarray(idx), cm, pf.expand(idx, 8, pf.PALETTE, cm)


def test_lossy_palette(encoder, quantised):
    idx, cm, want_px = quantised
    assert len(np.unique(idx)) > 100 and want_px.shape == (300, 530, 3)
    tif = pf.make_tiff(idx, 8, pf.PALETTE, colormap=cm, rows_per_strip=64)
    rc = jp2hip.recipe(jp2hip.LOSSY)
    got, _ = encoder.encode_tiff(tif, jp2hip.LOSSY, rc)
    assert got == oracle(want_px, rc)


def test_one_context_equal_geometry_own_colours(encoder):
    """Palette A, palette B (the same indices, another map), then an ordinary
    RGB8 TIFF of that size, twice over: the cached plan is shared, the colour
    table is each file's own."""
    idx = pf.indices(90, 77, 4, 31)
    cm_a, cm_b = pf.random_colormap(4, 32), pf.random_colormap(4, 33)
    rgb = im.synth_rgb8(90, 77, seed=34)
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    files = [(pf.make_tiff(idx, 4, pf.PALETTE, colormap=cm_a), pf.expand(idx, 4, pf.PALETTE, cm_a)),
             (pf.make_tiff(idx, 4, pf.PALETTE, colormap=cm_b), pf.expand(idx, 4, pf.PALETTE, cm_b)),
             (im.tiff_bytes(rgb, rows_per_strip=16), rgb)]
    want = [oracle(px, rc) for _, px in files]
    assert len(set(want)) == 3
    for _ in range(2):
        assert [encoder.encode_tiff(t, jp2hip.LOSSLESS, rc)[0] for t, _ in files] == want


def test_encode_device_with_the_parsed_layout(encoder):
    from devmem import DeviceBytes
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    for case in (dict(id="", bits=1, photometric=pf.WHITE_IS_ZERO, h=75, w=261, seed=41,
                      kw=dict(fill_order=2, rows_per_strip=16)),
                 dict(id="", bits=8, photometric=pf.PALETTE, h=70, w=90, seed=42, cmap_seed=43, wide=True,
                      kw=dict(tile=(32, 48), codec="deflate"))):
        tif, want_px, _, _ = pf.build(case)
        lay, keep = jp2hip.tiff_layout(tif)
        d = DeviceBytes(tif)
        try:
            got, _ = encoder.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, rc)
        finally:
            d.free()
        assert got == oracle(want_px, rc)


def test_encode_device_validates_a_callers_layout(encoder):
    """A caller's layout is held to the parser's rules before a kernel runs."""
    from devmem import DeviceBytes
    idx = pf.indices(40, 50, 4, 44)
    tif = pf.make_tiff(idx, 4, pf.PALETTE, colormap=pf.random_colormap(4, 45))
    d = DeviceBytes(tif)
    try:
        def attempt(**changes):
            lay, keep = jp2hip.tiff_layout(tif)
            for k, v in changes.items():
                setattr(lay, k, v)
            return encoder.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS)

        with pytest.raises(jp2hip.Jp2hipError, match="colormap"):
            attempt(colormap=None)
        with pytest.raises(jp2hip.Jp2hipError, match="colormap"):
            attempt(colormap_entries=47)
        with pytest.raises(jp2hip.Jp2hipError, match="bits/sample"):
            attempt(bits=3)
        with pytest.raises(jp2hip.Jp2hipError, match="1 component"):
            attempt(components=2)
        with pytest.raises(jp2hip.Jp2hipError, match="WhiteIsZero"):
            attempt(photometric=jp2hip._lib.PHOTO_WHITE_IS_ZERO, bits=8)
        with pytest.raises(jp2hip.Jp2hipError, match="outside the source buffer"):
            lay, keep = jp2hip.tiff_layout(tif)
            encoder.encode_device(d.ptr, lay.strip_offsets[lay.nstrips - 1] + 3, lay, jp2hip.LOSSLESS)
        attempt()
    finally:
        d.free()


@pytest.fixture(scope="module")
def tall():
    """900 rows, flush_period 0: two flush stripes, so two ranks have work.
    (bits 1 uncompressed strips, WhiteIsZero) and (4-bit palette, LZW)."""
    rc = jp2hip.recipe(jp2hip.LOSSLESS, flush_period=0)
    g_idx = pf.indices(900, 261, 1, 51)
    p_idx = pf.indices(900, 77, 4, 52)
    cm = pf.random_colormap(4, 53)
    return rc, {
        "g1_raw": (pf.make_tiff(g_idx, 1, pf.WHITE_IS_ZERO, fill_order=2, rows_per_strip=48),
                   oracle(pf.expand(g_idx, 1, pf.WHITE_IS_ZERO), rc)),
        "p4_lzw": (pf.make_tiff(p_idx, 4, pf.PALETTE, colormap=cm, rows_per_strip=48, codec="lzw", big_endian=True),
                   oracle(pf.expand(p_idx, 4, pf.PALETTE, cm), rc)),
    }


@pytest.mark.parametrize("which", ["g1_raw", "p4_lzw"])
def test_encode_file_single_gpu_and_split_identical(tmp_path, tall, which):
    rc, files = tall
    tif, want = files[which]
    src = tmp_path / "m.tif"
    src.write_bytes(tif)
    single, split = jp2hip.Encoder(0), jp2hip.Encoder(0)
    try:
        split.split_peers([0])
        a, b = tmp_path / "single.jpx", tmp_path / "split.jpx"
        single.encode_file(str(src), str(a), jp2hip.LOSSLESS, rc)
        st = split.encode_file(str(src), str(b), jp2hip.LOSSLESS, rc)
        assert a.read_bytes() == want
        assert b.read_bytes() == want
        assert st.out_bytes == len(want)
    finally:
        single.close()
        split.close()


@pytest.mark.parametrize("which", ["g1_raw", "p4_lzw"])
def test_encode_device_split_on_band_strips(tall, which):
    """Two ranks (threads), each given only its band's strips."""
    from devmem import DeviceBytes
    rc, files = tall
    tif, want = files[which]
    lay, offs = jp2hip.tiff_layout(tif)
    world = 2
    g = js.ThreadGroup(world)
    parts, errs = [None] * world, []

    def work(r):
        try:
            enc = jp2hip.Encoder(0)
            try:
                r0, r1 = js.split_rows(lay.height, rc.tile_h, r, world, rc.flush_period)
                assert r1 > r0
                buf, blay, keep = js.band_strips(tif, lay, offs, r0, r1)
                assert len(buf) < len(tif)
                d = DeviceBytes(buf or b"\0")
                try:
                    parts[r] = enc.encode_device_split(d.ptr, d.nbytes, blay, jp2hip.LOSSLESS, g.member(r).split(), rc)
                finally:
                    d.free()
            finally:
                enc.close()
        except Exception as e:  # keep the other rank from waiting forever
            errs.append(e)
            g.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    if errs:
        raise errs[0]
    assert parts[0][1] == 0 and parts[1][1] == len(parts[0][0])
    assert parts[0][2] == parts[1][2] == len(want)
    assert parts[0][0] + parts[1][0] == want


def test_batch_queue(tmp_path, encoder):
    from jp2hip import batch as jb
    case = dict(id="", bits=2, photometric=pf.PALETTE, h=75, w=77, seed=61, cmap_seed=62, wide=True,
                kw=dict(codec="packbits", rows_per_strip=16))
    tif, want_px, _, _ = pf.build(case)
    src = tmp_path / "t.tif"
    src.write_bytes(tif)
    with jb.BatchQueue(contexts=1, delete_after_upload=False) as q:
        q.submit(1, "ark:/x/palette", src, tmp_path / "batch.jpx")
        res = q.drain()
    assert res[0]["status"] == jb.OK, res[0]["message"]
    assert (tmp_path / "batch.jpx").read_bytes() == oracle(want_px, jp2hip.recipe(jp2hip.LOSSLESS))


def test_expanded_copy_is_accounted_and_limited(quantised):
    """The expanded copy is one of the context's buffers: jp2hip_device_bytes
    shows it, the hard limit covers it, and the context stays usable."""
    from devmem import DeviceBytes
    idx, cm, want_px = quantised
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    pal_tif = pf.make_tiff(idx, 8, pf.PALETTE, colormap=cm, rows_per_strip=64)
    rgb_tif = im.tiff_bytes(want_px, rows_per_strip=64)
    want = oracle(want_px, rc)
    held = {}
    for name, tif in (("palette", pal_tif), ("rgb", rgb_tif)):
        enc = jp2hip.Encoder(0)
        d = DeviceBytes(tif)  # the caller's buffer: the context holds no copy of the source
        try:
            lay, keep = jp2hip.tiff_layout(tif)
            got, _ = enc.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, rc)
            assert got == want, name
            held[name] = enc.device_bytes()
        finally:
            d.free()
            enc.close()
    assert held["palette"] - held["rgb"] >= want_px.nbytes
    enc = jp2hip.Encoder(0)
    try:
        enc.set_memory_limits(hard=held["palette"] - 1)
        with pytest.raises(jp2hip.Jp2hipError, match="device memory limit"):
            enc.encode_tiff(pal_tif, jp2hip.LOSSLESS, rc)
        assert enc.device_bytes() <= held["palette"] - 1
        enc.set_memory_limits(hard=0)
        got, _ = enc.encode_tiff(pal_tif, jp2hip.LOSSLESS, rc)
        assert got == want
    finally:
        enc.close()


def test_profile_mode_times_the_expansion():
    """The stage has its own timing events: ingest_ms is their span (the
    ordinary path launches nothing between its ingest events)."""
    idx = pf.indices(300, 530, 1, 71)
    enc = jp2hip.Encoder(0, profile=True)
    try:
        _, st = enc.encode_tiff(pf.make_tiff(idx, 1, pf.WHITE_IS_ZERO, rows_per_strip=64), jp2hip.LOSSLESS)
        assert 0.001 < st.ingest_ms < 50.0
    finally:
        enc.close()


@pytest.mark.parametrize("which", ["bilevel", "palette"])
def test_lossless_files_decode_to_the_expanded_pixels(encoder, which):
    if which == "bilevel":
        idx = pf.indices(120, 261, 1, 81)
        tif, want_px = pf.make_tiff(idx, 1, pf.WHITE_IS_ZERO), pf.expand(idx, 1, pf.WHITE_IS_ZERO)
    else:
        idx, cm = pf.indices(120, 77, 8, 82), pf.random_colormap(8, 83)
        tif, want_px = pf.make_tiff(idx, 8, pf.PALETTE, colormap=cm, big_endian=True), pf.expand(idx, 8, pf.PALETTE, cm)
    got, _ = encoder.encode_tiff(tif, jp2hip.LOSSLESS)
    assert np.array_equal(im.decode_pillow(got), want_px)
