"""The expectations of test_gpu_ingest_streams.py, on the CPU: the LZW and
PackBits reference decoders of ingest_stream_cases.py agree with libtiff
(Pillow's) on every crafted stream libtiff accepts, the two kinds of stream
it refuses are pinned as refused, the Predictor 2 writers produce files a
second reader decodes to the source pixels, and jp2hip.tiff_layout describes
every file.  No device is needed."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import imaging as im
import ingest_stream_cases as ic
import jp2hip


def pillow(tif: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(tif)))


def pillow_refuses(tif: bytes) -> bool:
    try:
        pillow(tif)
    except OSError:
        return True
    return False


# ---- LZW ----
@pytest.mark.parametrize("clear_every,clear_when_full", [(None, True), (700, True), (1, True), (3, True), (None, False)])
def test_lzw_pack_of_greedy_codes_is_lzw_encode(clear_every, clear_when_full):
    rng = np.random.default_rng(1)
    for data in (b"", b"a", b"aaaaaaa", im.synth_rgb8(20, 31).tobytes(),
                 bytes(rng.integers(0, 256, 6000, dtype=np.uint8)),  # fills the table: every width, Clear when full
                 bytes(rng.integers(0, 4, 9000, dtype=np.uint8))):
        codes = ic.lzw_greedy(data, clear_every, clear_when_full)
        assert ic.lzw_pack(codes) == im.lzw_encode(data, clear_every, clear_when_full)
        assert ic.lzw_model(ic.lzw_pack(codes), len(data)) == (data, "ok")


def test_lzw_model_statuses():
    s = ic.lzw_pack([ic.CLEAR, 65, 258, 259, 66, ic.EOI])  # A AA AAA B
    assert ic.lzw_model(s, 7) == (b"AAAAAAB", "ok")
    assert ic.lzw_model(s, 5) == (b"AAAAA", "ok")  # cut inside AAA; the rest is not looked at
    assert ic.lzw_model(s, 8) == (b"AAAAAAB", "short")
    assert ic.lzw_model(ic.lzw_pack([ic.CLEAR, 65, 259]), 9) == (b"A", "bad")
    assert ic.lzw_model(ic.lzw_pack([ic.CLEAR, 258]), 9) == (b"", "bad")
    assert ic.lzw_model(ic.lzw_pack([ic.CLEAR, 65, 258, ic.CLEAR, 258]), 9) == (b"AAA", "bad")
    assert ic.lzw_model(b"\x00\x01\x02", 9) == (b"", "old")
    assert ic.lzw_model(b"\x00\x02\x02", 1) == (b"\x00", "ok")
    assert ic.lzw_model(b"", 1) == (b"", "short")
    assert ic.lzw_segments(s) == [4] and ic.lzw_route(s) == "parallel"


@pytest.mark.parametrize("name", sorted(ic.LZW_FILES))
def test_lzw_named_streams_against_libtiff(name):
    f = ic.lzw_file(name)
    want = f.pixels()  # (asserts that every strip models as "ok")
    if name in ic.LIBTIFF_REFUSES:
        assert pillow_refuses(f.tiff())
    else:
        assert np.array_equal(pillow(f.tiff()), want)
    assert (f.w * f.h < 100_000) == (name not in ic.LARGE)


def test_lzw_named_streams_are_what_their_names_say():
    routes = {n: [ic.lzw_route(s) for s in ic.lzw_file(n).streams] for n in ic.LZW_FILES}
    assert routes["segment_4096"] == ["parallel"] and routes["segment_4097"] == ["serial"]
    assert routes["flat_full_dictionary"] == ["parallel"] and len(ic.lzw_file("flat_full_dictionary").streams[0]) == 5409
    assert routes["three_ways_parallel"] == ["parallel"] * 6
    assert routes["three_ways_long"] == ["serial"] * 5 + ["parallel"]  # (the last strip is 25 rows: 2500 codes)
    assert routes["three_ways_clear3"] == ["serial"] * 6
    assert routes["three_ways_mixed"] == ["serial", "parallel", "serial", "parallel", "serial", "serial"]
    assert routes["never_clears_6000"] == ["serial"]
    px = [ic.lzw_file(n).pixels() for n in ("three_ways_parallel", "three_ways_long", "three_ways_clear3", "three_ways_mixed")]
    assert all(np.array_equal(px[0], p) for p in px[1:])
    assert ic.lzw_segments(ic.lzw_file("flat_full_dictionary").streams[0]) == [3838]
    assert [len(s) for s in ic.lzw_file("three_byte_strips").streams[:2]] == [3, 4]
    flat = ic.lzw_file("flat_past_10_bits").pixels()
    assert flat.min() == flat.max() == 0x5A


def test_lzw_random_streams_against_libtiff():
    """40 files of 5 strips of codes no encoder wrote: all "ok" (the
    generator's promise), all read by libtiff to the model's bytes; Clears
    fall exactly at the first width change; the strips begin at every
    residue modulo 16."""
    residues, clear254 = set(), 0
    for i in range(ic.RANDOM_LZW):
        f = ic.random_lzw_file(i)
        assert (f.w, f.h, len(f.streams)) == (64 + i, 40, 5)
        assert [st for _, st in f.model()] == ["ok"] * 5, i
        assert np.array_equal(pillow(f.tiff()), f.pixels()), i
        residues |= {o % 16 for o in f.offsets()}
        clear254 += sum(ic.lzw_segments(s)[0] == 254 for s in f.streams)
    assert residues == set(range(16))
    assert clear254 >= 30
    tif, f = ic.random_lzw_file(3).tiff(), ic.random_lzw_file(3)
    assert [tif[o:o + len(s)] for o, s in zip(f.offsets(), f.streams)] == list(f.streams)


@pytest.mark.parametrize("route", ic.ROUTES)
@pytest.mark.parametrize("kind", ic.LZW_ERROR_KINDS)
def test_lzw_error_streams(kind, route):
    bad, good, _ = ic.lzw_error_pair(kind, route)  # (asserts the model's status and the route)
    assert np.array_equal(pillow(good.tiff()), good.pixels())
    assert pillow_refuses(bad.tiff())


def test_lzw_old_style_streams():
    for neighbour in ic.ROUTES:
        bad, good, _ = ic.lzw_old_style_pair(neighbour)
        assert np.array_equal(pillow(good.tiff()), good.pixels())


# ---- PackBits ----
@pytest.mark.parametrize("name", sorted(ic.PB_FILES))
def test_packbits_named_streams_against_libtiff(name):
    f = ic.pb_file(name)
    assert np.array_equal(pillow(f.tiff()), f.pixels())


def test_packbits_runs_writes_every_kind_of_run():
    hs = [h for s in ic.pb_file("runs").streams for h in ic.packbits_headers(s)]
    assert 127 in hs and 0x81 in hs and 0x80 in hs  # 128 literals, 128 repeats, no-op
    assert 0 in hs and 0xFF in hs                   # 1 literal, 2 repeats
    assert len({h for h in hs if h < 128}) > 5 and len({h for h in hs if h > 128}) > 5  # and lengths between
    cut = ic.pb_file("cut_at_cap")
    assert cut.pixels()[3, -5:].tolist() == [0xC3] * 5
    rng = np.random.default_rng(5)
    for row_bytes in (1, 2, 127, 128, 129, 300):
        raw = bytes(rng.integers(0, 3, 4 * row_bytes, dtype=np.uint8)) + bytes(2 * row_bytes)
        s = ic.packbits_runs(raw, row_bytes, rng)
        assert ic.packbits_model(s, len(raw)) == (raw, "ok")
        assert ic.packbits_model(s, len(raw) + 1)[1] == "short"


@pytest.mark.parametrize("kind", ic.PB_ERROR_KINDS)
def test_packbits_error_streams(kind):
    bad, good, _ = ic.pb_error_pair(kind)  # (asserts the model's status)
    assert np.array_equal(pillow(good.tiff()), good.pixels())


# ---- Predictor 2 layout matrix ----
def _units(tif):
    lay, keep = jp2hip.tiff_layout(tif)
    return lay, [tif[lay.strip_offsets[i]:lay.strip_offsets[i] + lay.strip_bytes[i]] for i in range(lay.nstrips)]


def _decoded(case, stream):
    if case["codec"] == "deflate":
        return zlib.decompress(stream)
    cap = 1 << 20
    out, status = (ic.lzw_model if case["codec"] == "lzw" else ic.packbits_model)(stream, cap)
    assert status == "short"  # (all of it: the codes end before 1 MiB)
    return out


@pytest.mark.parametrize("case", ic.LAYOUT_CASES, ids=[c["id"] for c in ic.LAYOUT_CASES])
def test_layout_matrix_files(case):
    tif, px = ic.layout_build(case)
    nc, u16 = case["components"], case["sample"] != "u8"
    planar = case["layout"].endswith("planar")
    px3 = px.reshape(case["h"], case["w"], nc)
    # What Pillow reads to the source pixels: 8-bit samples with any number of
    # components, 16-bit ones with one.  Not planar grey + alpha (it takes the
    # second plane from the wrong place), and not PackBits: libtiff knows
    # Predictor for LZW and Deflate only and hands PackBits data out
    # differenced, where the product honours the tag with every codec.
    if case["codec"] != "packbits" and (nc == 1 or (not u16 and not (planar and nc == 2))):
        assert np.array_equal(pillow(tif), px)
    else:
        # The writer is checked instead: its differenced samples of component c
        # must be those of the one-component LZW or Deflate file of that
        # component (which Pillow does read), unit by unit, whatever the
        # interleaving and the codec.
        twin = dict(case, layout=case["layout"].replace("planar", "chunky"),
                    codec="lzw" if case["codec"] == "packbits" else case["codec"])
        lay, units = _units(tif)
        dt = np.dtype(np.uint16).newbyteorder(">" if case["sample"] == "u16be" else "<") if u16 else np.uint8
        per_plane = lay.nstrips // nc if planar else lay.nstrips
        for c in range(nc):
            one = ic.layout_write(twin, px3[..., c:c + 1])
            assert np.array_equal(pillow(one), px3[..., c])
            _, one_units = _units(one)
            assert len(one_units) == per_plane
            for j in range(per_plane):
                want = np.frombuffer(_decoded(twin, one_units[j]), dt)
                if planar:
                    got = np.frombuffer(_decoded(case, units[c * per_plane + j]), dt)
                else:
                    got = np.frombuffer(_decoded(case, units[j]), dt).reshape(-1, nc)[:, c]
                assert np.array_equal(got, want), (c, j)
    lay, _ = jp2hip.tiff_layout(tif)
    want = ic.layout_expect(case)
    assert (lay.width, lay.height, lay.components, lay.bits) == (case["w"], case["h"], nc, 16 if u16 else 8)
    assert (lay.compression, lay.predictor) == (want["compression"], want["predictor"])
    assert (lay.tile_width, lay.tile_height) == want["tile"] and lay.nstrips == want["units"]
    assert lay.planar == (2 if case["layout"].endswith("planar") else 1)
    assert lay.big_endian == (tif[:2] == b"MM")


def test_predictor_writers_default_to_the_files_they_always_wrote():
    img = im.synth_rgb8(40, 50)
    assert b"\x3d\x01\x03\x00" not in im.tiff_bytes(img)[:200]  # no Predictor entry
    for fn in (im.tiff_bytes, im.bigtiff_bytes):
        a = fn(img, rows_per_strip=16, strip_codec=zlib.compress, compression=8, predictor=2)
        assert np.array_equal(pillow(a), img)
    t = im.tiled_tiff_bytes(img, tile=(16, 16), codec=im.lzw_encode, compression=5, predictor=2)
    assert np.array_equal(pillow(t), img)
    assert np.array_equal(pillow(im.tiled_tiff_bytes(img, tile=(16, 16), codec=zlib.compress, compression=8)), img)


# ---- packed and palette files with real runs ----
@pytest.mark.parametrize("case", ic.PACKED_CASES, ids=[c["id"] for c in ic.PACKED_CASES])
def test_packed_cases(case):
    tif, want, headers = ic.packed_build(case)
    palette = case["photometric"] == ic.pf.PALETTE
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(tif)).convert("RGB" if palette else "L")), want)
    lzw = case.get("codec") == "lzw"
    assert lzw or (any(h > 128 for h in headers) and any(h < 128 for h in headers) and 0x80 in headers)
    lay, _ = jp2hip.tiff_layout(tif)
    assert (lay.width, lay.height, lay.bits) == (case["w"], case["h"], case["bits"])
    assert lay.compression == (ic.LZW if lzw else ic.PACKBITS)
    assert (lay.tile_width, lay.tile_height) == (case["tile"] or (0, 0))
