"""The decoders in front of ingest (LZW, PackBits, Predictor 2, tiles) on
crafted streams and on layouts no encoder-written fixture expresses
(ingest_stream_cases.py; test_ingest_streams.py pins its expectations to
libtiff).  The expected file is always the oracle's encode of the expected
pixels: never the GPU's own encode of an uncompressed twin, where a fault
common to both routes would cancel out."""
import threading

import numpy as np
import pytest

import imaging as im
import ingest_stream_cases as ic
import jp2hip
import oracle_lib as ol
from jp2hip import split as js

pytestmark = pytest.mark.gpu


def oracle(img, rc):
    return ol.encode(img, ol.copy_recipe(rc))


def lossless():
    return jp2hip.recipe(jp2hip.LOSSLESS)


def check(encoder, tif, want_px):
    rc = lossless()
    got, _ = encoder.encode_tiff(tif, jp2hip.LOSSLESS, rc)
    assert got == oracle(want_px, rc)


# ---- valid streams ----
@pytest.mark.parametrize("name", sorted(ic.LZW_FILES))
def test_lzw_named_streams(encoder, name):
    f = ic.lzw_file(name)
    check(encoder, f.tiff(), f.pixels())


def test_lzw_random_streams(encoder):
    """200 strips of codes no encoder wrote, beginning at every residue
    modulo 16 of the source buffer (which is aligned far beyond 16)."""
    residues = set()
    for i in range(ic.RANDOM_LZW):
        f = ic.random_lzw_file(i)
        assert 64 <= f.w <= 103 and f.h == 40 and len(f.streams) == 5
        residues |= {o % 16 for o in f.offsets()}
        rc = lossless()
        got, _ = encoder.encode_tiff(f.tiff(), jp2hip.LOSSLESS, rc)
        assert got == oracle(f.pixels(), rc), i
    assert residues == set(range(16))


@pytest.mark.parametrize("name", sorted(ic.PB_FILES))
def test_packbits_named_streams(encoder, name):
    f = ic.pb_file(name)
    check(encoder, f.tiff(), f.pixels())


# ---- error streams: the error class, then the same context on the good file ----
def refused_then_good(encoder, bad, good, match):
    rc = lossless()
    with pytest.raises(jp2hip.Jp2hipError, match=match):
        encoder.encode_tiff(bad.tiff(), jp2hip.LOSSLESS, rc)
    got, _ = encoder.encode_tiff(good.tiff(), jp2hip.LOSSLESS, rc)
    assert got == oracle(good.pixels(), rc)  # (no stale segment table, no stale error flag)


@pytest.mark.parametrize("route", ic.ROUTES)
@pytest.mark.parametrize("kind", ic.LZW_ERROR_KINDS)
def test_lzw_error_streams(encoder, kind, route):
    refused_then_good(encoder, *ic.lzw_error_pair(kind, route))


@pytest.mark.parametrize("neighbour", ic.ROUTES)
def test_lzw_old_style_stream(encoder, neighbour):
    refused_then_good(encoder, *ic.lzw_old_style_pair(neighbour))


@pytest.mark.parametrize("kind", ic.PB_ERROR_KINDS)
def test_packbits_error_streams(encoder, kind):
    refused_then_good(encoder, *ic.pb_error_pair(kind))


# ---- layouts ----
@pytest.mark.parametrize("case", ic.LAYOUT_CASES, ids=[c["id"] for c in ic.LAYOUT_CASES])
def test_layout_matrix(encoder, case):
    tif, px = ic.layout_build(case)
    check(encoder, tif, px)


@pytest.mark.parametrize("case", ic.PACKED_CASES, ids=[c["id"] for c in ic.PACKED_CASES])
def test_packed_and_palette_files_with_runs(encoder, case):
    tif, want_px, _ = ic.packed_build(case)
    check(encoder, tif, want_px)


@pytest.mark.parametrize("big_endian", [False, True])
def test_bigtiff_predictor(encoder, big_endian):
    px = ic.noise(37, 45, 3, np.uint8, 1101)
    tif = im.bigtiff_bytes(px, rows_per_strip=8, big_endian=big_endian, strip_codec=im.lzw_encode, compression=ic.LZW,
                           predictor=2)
    check(encoder, tif, px)


def _case(**want):
    (c,) = [c for c in ic.LAYOUT_CASES if all(c[k] == v for k, v in want.items())][:1]
    return c


def test_lossy_lzw_tiles(encoder):
    tif, px = ic.layout_build(dict(_case(codec="lzw", layout="tiles_chunky", sample="u8", components=3), w=77), h=90)
    rc = jp2hip.recipe(jp2hip.LOSSY)
    got, _ = encoder.encode_tiff(tif, jp2hip.LOSSY, rc)
    assert got == oracle(px, rc)


# ---- routes: four representatives, 900 rows, two flush stripes ----
@pytest.fixture(scope="module")
def tall():
    """900 rows, flush_period 0: two flush stripes, so two ranks have work."""
    rc = jp2hip.recipe(jp2hip.LOSSLESS, flush_period=0)
    files = {}
    files["lzw_tiles_rgb8"] = ic.layout_build(
        dict(_case(codec="lzw", layout="tiles_chunky", sample="u8", components=3), w=45), h=900)
    files["deflate_tiles_planar_u16be"] = ic.layout_build(
        dict(_case(codec="deflate", layout="tiles_planar", sample="u16be", components=3), w=45), h=900)
    files["bilevel_packbits_runs"] = ic.packed_build(dict(ic.PACKED_CASES[0], w=100, rps=48), h=900)[:2]
    mixed = ic.three_ways_file(("long", "parallel", "clear3", "parallel", "long", "clear3"), h=900, seed=991)
    assert {ic.lzw_route(s) for s in mixed.streams} == {"parallel", "serial"}
    files["lzw_mixed_routes"] = (mixed.tiff(), mixed.pixels())
    return rc, {k: (tif, oracle(px, rc)) for k, (tif, px) in files.items()}


TALL = ["lzw_tiles_rgb8", "deflate_tiles_planar_u16be", "bilevel_packbits_runs", "lzw_mixed_routes"]


@pytest.mark.parametrize("which", TALL)
def test_encode_device_with_the_parsed_layout(encoder, tall, which):
    from devmem import DeviceBytes
    rc, files = tall
    tif, want = files[which]
    lay, keep = jp2hip.tiff_layout(tif)
    d = DeviceBytes(tif)
    try:
        got, _ = encoder.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, rc)
    finally:
        d.free()
    assert got == want


@pytest.mark.parametrize("which", TALL)
def test_encode_file_with_a_split_peer(tmp_path, tall, which):
    rc, files = tall
    tif, want = files[which]
    src, dst = tmp_path / "m.tif", tmp_path / "split.jpx"
    src.write_bytes(tif)
    enc = jp2hip.Encoder(0)
    try:
        enc.split_peers([0])
        st = enc.encode_file(str(src), str(dst), jp2hip.LOSSLESS, rc)
        assert dst.read_bytes() == want
        assert st.out_bytes == len(want)
    finally:
        enc.close()


@pytest.mark.parametrize("which", TALL)
def test_encode_device_split_on_band_strips(tall, which):
    """Two ranks (threads), each given only its band's strips or tiles."""
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
