"""The TIFF's ICC profile, ExtraSamples and resolution through every route a
file takes on the GPU: encode_tiff, encode_device, encode_device_split,
encode_file (single GPU and the in-process tile-split) and the batch queue.

Only the bytes in front of the code-stream depend on the metadata, so the
expected file is always jp2hip.file_header(...) of the TIFF's layout followed
by the oracle's code-stream for the same pixels and recipe (the header writer
itself is checked box by box on the CPU, test_source_metadata.py)."""
import threading

import numpy as np
import pytest

import imaging as im
import jp2hip
import metadata_fixtures as mf
import oracle_lib as ol
from jp2hip import split as js

pytestmark = pytest.mark.gpu

RESTRICTED = mf.icc_profile()
ANY = mf.icc_profile(tags=mf.RGB_MATRIX_TAGS + (b"A2B0",))
UNUSABLE = mf.icc_profile(magic=b"ascp")


def expected(tif, img, rc):
    """file_header of the TIFF's layout + the oracle's code-stream."""
    cs = im.codestream(ol.encode(img, ol.copy_recipe(rc)))
    return jp2hip.file_header(jp2hip.tiff_layout(tif)[0], rc.format, len(cs)) + cs


@pytest.fixture(scope="module")
def rgb16():
    img = im.synth_u16(100, 70, comps=3, seed=3)
    tif = mf.tag_source(im.tiff_bytes(img, rows_per_strip=16, big_endian=True), icc=RESTRICTED,
                        xres=(300, 1), yres=(300, 1), unit=2)
    return img, tif


@pytest.mark.parametrize("conv,fmt", [(jp2hip.LOSSLESS, jp2hip.FORMAT_JPX), (jp2hip.LOSSY, jp2hip.FORMAT_JP2)],
                         ids=["lossless_jpx", "lossy_jp2"])
def test_encode_tiff_icc_and_resolution(encoder, rgb16, conv, fmt):
    img, tif = rgb16
    rc = jp2hip.recipe(conv, format=fmt)
    got, _ = encoder.encode_tiff(tif, conv, rc)
    want = expected(tif, img, rc)
    assert got == want
    # the header does carry them (and so differs from the untagged file's)
    kinds = [t for t, _ in mf.jp2h_boxes(got[:len(got) - len(im.codestream(got))])]
    assert kinds == [b"ihdr", b"colr", b"res "]
    plain, _ = encoder.encode_tiff(im.tiff_bytes(img, rows_per_strip=16, big_endian=True), conv, rc)
    assert plain == ol.encode(img, ol.copy_recipe(rc))
    assert im.codestream(plain) == im.codestream(got) and len(got) == len(plain) - 15 + 11 + len(RESTRICTED) + 26
    if conv == jp2hip.LOSSLESS:
        # (Pillow reduces 16-bit RGB to 8 bits; OpenJPEG's own tool keeps them)
        assert np.array_equal(im.decode_opj(got), img)


@pytest.mark.parametrize("nc", [4, 2], ids=["rgba8", "grey_alpha8"])
def test_encode_tiff_extra_samples(encoder, nc):
    rgb = im.synth_rgb8(90, 60, seed=8)
    img = np.ascontiguousarray(np.dstack([rgb, rgb[..., 1:2]]) if nc == 4 else rgb[..., :2])
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    files = {}
    for alpha in (0, 1, 2):
        tif = im.tiff_bytes(img, alpha=alpha)
        files[alpha], _ = encoder.encode_tiff(tif, jp2hip.LOSSLESS, rc)
        assert files[alpha] == expected(tif, img, rc), alpha
    assert files[2] == ol.encode(img, ol.copy_recipe(rc))  # unassociated alpha: the file as it always was
    assert len(files[1]) == len(files[2]) and files[1] != files[2]      # cdef Typ 2
    assert len(files[0]) == len(files[2]) - (8 + 2 + 6 * nc)            # no cdef box
    if nc == 4:
        for alpha in (0, 1, 2):
            assert np.array_equal(im.decode_pillow(files[alpha]), img), alpha


@pytest.mark.parametrize("fmt", [jp2hip.FORMAT_JPX, jp2hip.FORMAT_JP2], ids=["jpx", "jp2"])
def test_encode_tiff_any_and_unusable_profiles(encoder, fmt):
    img = im.synth_rgb8(90, 60, seed=9)
    base = im.tiff_bytes(img, rows_per_strip=32)
    rc = jp2hip.recipe(jp2hip.LOSSY, format=fmt)
    untagged, _ = encoder.encode_tiff(base, jp2hip.LOSSY, rc)
    assert untagged == ol.encode(img, ol.copy_recipe(rc))
    tif = mf.tag_source(base, icc=ANY)
    got, _ = encoder.encode_tiff(tif, jp2hip.LOSSY, rc)
    assert got == expected(tif, img, rc)
    if fmt == jp2hip.FORMAT_JPX:
        assert len(got) == len(untagged) + 11 + len(ANY)  # the METH 3 box after the enumerated one
    else:
        assert got == untagged                            # Part 1 cannot carry it
    bad, _ = encoder.encode_tiff(mf.tag_source(base, icc=UNUSABLE), jp2hip.LOSSY, rc)
    assert bad == untagged


def test_encode_device_equals_encode_tiff(encoder, rgb16):
    from devmem import DeviceBytes
    img, tif = rgb16
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    want, _ = encoder.encode_tiff(tif, jp2hip.LOSSLESS, rc)
    lay, keep = jp2hip.tiff_layout(tif)
    d = DeviceBytes(tif)
    try:
        got, _ = encoder.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, rc)
    finally:
        d.free()
    assert got == want == expected(tif, img, rc)


def test_plan_cache_does_not_keep_the_metadata(encoder):
    """Equal geometry and recipe, different metadata, one context: each file
    gets its own header (the cached plan holds none of it)."""
    img = im.synth_rgb8(90, 60, seed=10)
    base = im.tiff_bytes(img, rows_per_strip=32)
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    tifs = [mf.tag_source(base, icc=RESTRICTED, xres=(72, 1), yres=(72, 1), unit=2), base,
            mf.tag_source(base, xres=(400, 1), yres=(400, 1), unit=3), mf.tag_source(base, icc=ANY)]
    got = [encoder.encode_tiff(t, jp2hip.LOSSLESS, rc)[0] for t in tifs]
    assert got == [expected(t, img, rc) for t in tifs]
    assert len(set(got)) == 4


@pytest.fixture(scope="module")
def lzw_master():
    img = im.synth_rgb8(900, 500, seed=17)
    tif = mf.tag_source(im.tiff_bytes(img, rows_per_strip=48, strip_codec=im.lzw_encode, compression=5),
                        icc=RESTRICTED, xres=(600, 1), yres=(600, 1), unit=2)
    rc = jp2hip.recipe(jp2hip.LOSSY, flush_period=0)
    return img, tif, rc, expected(tif, img, rc)


def test_encode_file_single_gpu_and_split_identical(tmp_path, lzw_master):
    img, tif, rc, want = lzw_master
    src = tmp_path / "m.tif"
    src.write_bytes(tif)
    single, split = jp2hip.Encoder(0), jp2hip.Encoder(0)
    try:
        split.split_peers([0])
        a, b = tmp_path / "single.jpx", tmp_path / "split.jpx"
        single.encode_file(str(src), str(a), jp2hip.LOSSY, rc)
        st = split.encode_file(str(src), str(b), jp2hip.LOSSY, rc)
        assert a.read_bytes() == want
        assert b.read_bytes() == want
        assert st.out_bytes == len(want)
    finally:
        single.close()
        split.close()


def test_encode_device_split_bands_carry_the_metadata(lzw_master):
    """The collective with a caller's all-reduce: two ranks (threads), each
    given only its band's strips (jp2hip.split.band_strips keeps the file's
    metadata on the band layout)."""
    from devmem import DeviceBytes
    img, tif, rc, want = lzw_master
    lay, offs = jp2hip.tiff_layout(tif)
    world = 2
    g = js.ThreadGroup(world)
    parts, errs = [None] * world, []

    def work(r):
        try:
            enc = jp2hip.Encoder(0)
            try:
                r0, r1 = js.split_rows(lay.height, rc.tile_h, r, world, rc.flush_period)
                buf, blay, keep = js.band_strips(tif, lay, offs, r0, r1)
                d = DeviceBytes(buf or b"\0")
                try:
                    parts[r] = enc.encode_device_split(d.ptr, d.nbytes, blay, jp2hip.LOSSY, g.member(r).split(), rc)
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


def test_batch_queue_carries_the_metadata(tmp_path, encoder, rgb16):
    from jp2hip import batch as jb
    img, tif = rgb16
    src = tmp_path / "t.tif"
    src.write_bytes(tif)
    encoder.encode_file(str(src), str(tmp_path / "direct.jpx"), jp2hip.LOSSLESS)
    with jb.BatchQueue(contexts=1, delete_after_upload=False) as q:
        q.submit(1, "ark:/x/tagged", src, tmp_path / "batch.jpx")
        res = q.drain()
    assert res[0]["status"] == jb.OK, res[0]["message"]
    got = (tmp_path / "batch.jpx").read_bytes()
    assert got == (tmp_path / "direct.jpx").read_bytes()
    assert got == expected(tif, img, jp2hip.recipe(jp2hip.LOSSLESS))
