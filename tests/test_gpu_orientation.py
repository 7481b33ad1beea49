"""TIFF Orientation on the GPU: an encode with source orientation o gives
exactly the file the oracle encodes from the upright pixels
(orientation_cases.upright, which test_orientation.py pins to Pillow), on
every route a file takes.  For sources with metadata the expected file is
jp2hip.file_header of the upright layout followed by the oracle's
code-stream, as in test_gpu_source_metadata.py."""
import threading

import numpy as np
import pytest

import imaging as im
import jp2hip
import metadata_fixtures as mf
import oracle_lib as ol
import orientation_cases as oc
import pixel_format_cases as pf
from jp2hip import split as js

pytestmark = pytest.mark.gpu

OFF, TIFF = jp2hip.ORIENT_OFF, jp2hip.ORIENT_TIFF


def oracle(img, rc):
    return ol.encode(img, ol.copy_recipe(rc))


@pytest.fixture(scope="module")
def oenc():
    """A context of this module's own: the suite's shared one keeps its
    default orientation."""
    enc = jp2hip.Encoder(0)
    yield enc
    enc.close()


def encode(enc, o, tif, conv, rc):
    enc.set_source_orientation(o)
    try:
        return enc.encode_tiff(tif, conv, rc)
    finally:
        enc.set_source_orientation(OFF)


# ---- the matrix: element form x size x orientation, lossless ----

@pytest.mark.parametrize("form", oc.FORMS)
def test_matrix_lossless(oenc, form):
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    for h, w in oc.SIZES:
        px = oc.pixels(form, h, w)
        tif = oc.form_tiff(form, px)
        for o in oc.VALUES:
            got, _ = encode(oenc, o, tif, jp2hip.LOSSLESS, rc)
            assert got == oracle(oc.upright(px, o), rc), (form, h, w, o)
    # off is the default and ignores the tag
    got, _ = oenc.encode_tiff(oc.tag(tif, 6), jp2hip.LOSSLESS, rc)
    assert got == oracle(px, rc)


@pytest.mark.parametrize("o", [6, 7])
def test_lossy_turned(oenc, o):
    px = im.synth_rgb8(300, 530, seed=3)
    rc = jp2hip.recipe(jp2hip.LOSSY)
    got, st = encode(oenc, o, im.tiff_bytes(px), jp2hip.LOSSY, rc)
    assert got == oracle(oc.upright(px, o), rc)
    assert st.out_bytes == len(got)


def test_lossless_turned_file_decodes_to_the_upright_pixels(oenc):
    px = im.synth_rgb8(130, 67, seed=4)
    got, _ = encode(oenc, 5, im.tiff_bytes(px, rows_per_strip=16), jp2hip.LOSSLESS, jp2hip.recipe(jp2hip.LOSSLESS))
    assert np.array_equal(im.decode_pillow(got), oc.upright(px, 5))


# ---- the stages in front of it: decoders and the sample expansion ----

def _coded_sources():
    rgb = im.synth_rgb8(75, 130, seed=11)
    g16 = im.synth_u16(70, 90, comps=1, seed=12)
    idx1, idx4 = pf.indices(75, 261, 1, 13), pf.indices(70, 90, 4, 14)
    cm = pf.random_colormap(4, 15)
    return {
        "lzw_predictor2": (im.tiff_bytes(rgb, rows_per_strip=16, strip_codec=im.lzw_encode, compression=5, predictor=2),
                           rgb),
        "deflate_tiles_ragged": (im.tiled_tiff_bytes(rgb, tile=(32, 48), deflate=True), rgb),
        "packbits": (im.tiff_bytes(g16, rows_per_strip=16, strip_codec=im.packbits_encode, compression=32773), g16),
        "bilevel_white_is_zero_lsb": (pf.make_tiff(idx1, 1, pf.WHITE_IS_ZERO, fill_order=2, rows_per_strip=16),
                                      pf.expand(idx1, 1, pf.WHITE_IS_ZERO)),
        "palette4": (pf.make_tiff(idx4, 4, pf.PALETTE, colormap=cm), pf.expand(idx4, 4, pf.PALETTE, cm)),
        "bigtiff": (im.bigtiff_bytes(rgb, rows_per_strip=16, big_endian=True), rgb),
    }


CODED = _coded_sources()


@pytest.mark.parametrize("name", sorted(CODED))
def test_sources_in_front_of_it(oenc, name):
    tif, px = CODED[name]
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    for o in (3, 6):
        got, _ = encode(oenc, o, tif, jp2hip.LOSSLESS, rc)
        assert got == oracle(oc.upright(px, o), rc), (name, o)


# ---- one context, one geometry after another ----

def test_one_context_plan_cache_sees_the_upright_size():
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    sq = im.synth_rgb8(96, 96, seed=21)
    tif = im.tiff_bytes(sq, rows_per_strip=16)
    enc = jp2hip.Encoder(0)
    try:
        first = True
        for o in (OFF, 6, 1, 8, OFF):
            got, st = encode(enc, o, tif, jp2hip.LOSSLESS, rc)
            assert got == oracle(oc.upright(sq, max(o, 1)), rc), o
            # a square image keeps its geometry under every orientation
            assert bool(st.reused & jp2hip._lib.REUSED_PLAN) == (not first), o
            first = False
        tall = im.synth_rgb8(90, 77, seed=22)
        ttif = im.tiff_bytes(tall, rows_per_strip=16)
        got, st = encode(enc, 6, ttif, jp2hip.LOSSLESS, rc)       # 90 wide, 77 high
        assert got == oracle(oc.upright(tall, 6), rc) and not st.reused & jp2hip._lib.REUSED_PLAN
        got, st = encode(enc, 1, ttif, jp2hip.LOSSLESS, rc)       # 77 wide, 90 high: another plan
        assert got == oracle(tall, rc) and not st.reused & jp2hip._lib.REUSED_PLAN
    finally:
        enc.close()


# ---- routes ----

@pytest.fixture(scope="module")
def tagged():
    """RGB16 big-endian with an ICC profile, unequal resolutions and tag 274 = 6."""
    px = im.synth_u16(100, 70, comps=3, seed=3)
    tif = oc.tag(mf.tag_source(im.tiff_bytes(px, rows_per_strip=16, big_endian=True), icc=mf.icc_profile(),
                               xres=(300, 1), yres=(450, 1), unit=2), 6)
    return px, tif


def expected(tif, px, o, rc):
    """file_header of the upright layout + the oracle's code-stream of the upright pixels."""
    cs = im.codestream(oracle(oc.upright(px, o), rc))
    return jp2hip.file_header(oc.oriented_layout(jp2hip.tiff_layout(tif)[0], o), rc.format, len(cs)) + cs


def test_encode_tiff_and_file_honour_the_files_tag(tmp_path, oenc, tagged):
    px, tif = tagged
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    want = expected(tif, px, 6, rc)
    assert want != expected(tif, px, 1, rc)
    got, _ = encode(oenc, TIFF, tif, jp2hip.LOSSLESS, rc)
    assert got == want
    src, out = tmp_path / "t.tif", tmp_path / "t.jpx"
    src.write_bytes(tif)
    oenc.set_source_orientation(TIFF)
    try:
        oenc.encode_file(str(src), str(out), jp2hip.LOSSLESS, rc)
    finally:
        oenc.set_source_orientation(OFF)
    assert out.read_bytes() == want
    # a file without the tag is upright already
    plain = mf.add_tags(tif, [], drop=(oc.ORIENTATION,))
    got, _ = encode(oenc, TIFF, plain, jp2hip.LOSSLESS, rc)
    assert got == expected(plain, px, 1, rc)
    # off: the tag is ignored, as before
    got, _ = oenc.encode_tiff(tif, jp2hip.LOSSLESS, rc)
    assert got == expected(tif, px, 1, rc)


def test_encode_device_takes_a_value_and_refuses_the_tag(oenc, tagged):
    from devmem import DeviceBytes
    px, tif = tagged
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    lay, keep = jp2hip.tiff_layout(tif)
    d = DeviceBytes(tif)
    try:
        oenc.set_source_orientation(jp2hip.tiff_orientation(tif))
        got, _ = oenc.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, rc)
        assert got == expected(tif, px, 6, rc)
        oenc.set_source_orientation(TIFF)
        with pytest.raises(jp2hip.Jp2hipError, match="jp2hip_tiff_orientation") as e:
            oenc.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, rc)
        assert "jp2hip_set_source_orientation" in str(e.value)
        with pytest.raises(jp2hip.Jp2hipError, match="jp2hip_tiff_orientation"):
            oenc.encode_device_split(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, js.SingleGroup().split(), rc)
        oenc.set_source_orientation(8)  # the context stays usable
        got, _ = oenc.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, rc)
        assert got == expected(tif, px, 8, rc)
        with pytest.raises(jp2hip.Jp2hipError, match="10"):
            oenc.set_source_orientation(10)
    finally:
        oenc.set_source_orientation(OFF)
        d.free()


def test_batch_queue_honours_the_tag(tmp_path, tagged):
    from jp2hip import batch as jb
    px, tif = tagged
    src = tmp_path / "t.tif"
    src.write_bytes(tif)
    with jb.BatchQueue(contexts=1, delete_after_upload=False, orientation=TIFF) as q:
        q.submit(1, "ark:/x/turned", src, tmp_path / "batch.jpx")
        with pytest.raises(jp2hip.Jp2hipError):  # only before the first submit
            q.set_source_orientation(OFF)
        res = q.drain()
    assert res[0]["status"] == jb.OK, res[0]["message"]
    assert (tmp_path / "batch.jpx").read_bytes() == expected(tif, px, 6, jp2hip.recipe(jp2hip.LOSSLESS))


@pytest.fixture(scope="module")
def tall():
    """900 rows (and, turned, 900 columns of 500 rows: one tile row), LZW
    strips, flush_period 0: two flush stripes, so two ranks have work."""
    px = im.synth_rgb8(900, 500, seed=17)
    tif = mf.tag_source(im.tiff_bytes(px, rows_per_strip=48, strip_codec=im.lzw_encode, compression=5),
                        xres=(600, 1), yres=(300, 1), unit=2)
    wide = np.ascontiguousarray(px.swapaxes(0, 1))  # 500 rows of 900: turned, it has 900 rows
    wtif = mf.tag_source(im.tiff_bytes(wide, rows_per_strip=48), xres=(600, 1), yres=(300, 1), unit=2)
    return px, tif, wide, wtif, jp2hip.recipe(jp2hip.LOSSY, flush_period=0)


@pytest.mark.parametrize("o", [3, 6])
def test_split_peers_equal_the_single_gpu_file(tmp_path, tall, o):
    px, tif, wide, wtif, rc = tall
    px, tif = (px, tif) if o == 3 else (wide, wtif)
    want = expected(tif, px, o, rc)
    src = tmp_path / "m.tif"
    src.write_bytes(tif)
    single, split = jp2hip.Encoder(0), jp2hip.Encoder(0)
    try:
        single.set_source_orientation(o)
        split.split_peers([0])
        split.set_source_orientation(o)  # the peer gets it here
        a, b = tmp_path / "single.jpx", tmp_path / "split.jpx"
        single.encode_file(str(src), str(a), jp2hip.LOSSY, rc)
        st = split.encode_file(str(src), str(b), jp2hip.LOSSY, rc)
        assert a.read_bytes() == want
        assert b.read_bytes() == want and st.out_bytes == len(want)
        split.split_peers([0])           # a peer added later inherits it
        got, _ = split.encode_tiff(tif, jp2hip.LOSSY, rc)
        assert got == want
    finally:
        single.close()
        split.close()


@pytest.mark.parametrize("o", [3, 6])
def test_split_over_a_callers_group(tall, o):
    """Two ranks (threads) over a caller's all-reduce.  o = 3: each is given
    only the strips of its mirrored band; o = 6: each the whole source."""
    from devmem import DeviceBytes
    px, tif, wide, wtif, rc = tall
    px, tif = (px, tif) if o == 3 else (wide, wtif)
    want = expected(tif, px, o, rc)
    lay, offs = jp2hip.tiff_layout(tif)
    _, oh = jp2hip.oriented_size(lay.width, lay.height, o)
    assert oh == 900
    world = 2
    g = js.ThreadGroup(world)
    parts, errs, given = [None] * world, [], [0] * world

    def work(r):
        try:
            enc = jp2hip.Encoder(0)
            try:
                enc.set_source_orientation(o)
                r0, r1 = js.split_rows(oh, rc.tile_h, r, world, rc.flush_period)
                s0, s1 = jp2hip.orientation_source_rows(lay.height, lay.width, o, r0, r1)
                buf, blay, keep = js.band_strips(tif, lay, offs, s0, s1)
                given[r] = len(buf)
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
    strips = sum(int(offs[lay.nstrips + i]) for i in range(lay.nstrips)) if lay.compression > 1 else px.nbytes
    if o == 3:
        assert 0 < given[0] < strips and 0 < given[1] < strips  # its band's strips only
    else:
        assert given[0] == given[1] == strips                   # the whole source


# ---- organisation and layer settings ride along ----

def test_organisation_letters_order_and_layer_rates_together(oenc):
    px = im.synth_rgb8(300, 530, seed=31)
    rc = jp2hip.recipe(jp2hip.LOSSY, progression=jp2hip.ORDER_LRCP, tparts_r=0, layers=3)
    rates = [0.5, 1.0, 2.0]
    tif = im.tiff_bytes(px)
    oenc.set_organisation(tlm=True)
    oenc.set_tile_part_divisions("L")
    oenc.set_layer_rates(rates)
    try:
        got, _ = encode(oenc, 6, tif, jp2hip.LOSSY, rc)
        want, _ = oenc.encode_tiff(im.tiff_bytes(oc.upright(px, 6)), jp2hip.LOSSY, rc)
        assert got == want
    finally:
        oenc.set_layer_rates(None)
        oenc.set_tile_part_divisions(0)
        oenc.set_organisation(tlm=False)
    plain, _ = encode(oenc, 6, tif, jp2hip.LOSSY, rc)  # (the oracle writes RPCL only: the upright TIFF's encode again)
    assert plain == oenc.encode_tiff(im.tiff_bytes(oc.upright(px, 6)), jp2hip.LOSSY, rc)[0]
    assert plain != got  # (the settings did apply)


# ---- accounting ----

def test_oriented_copy_is_accounted_and_limited():
    """The upright copy is one of the context's buffers: jp2hip_device_bytes
    shows it, the hard limit covers it, and the context stays usable."""
    from devmem import DeviceBytes
    px = im.synth_rgb8(300, 530, seed=3)
    tif = im.tiff_bytes(px, rows_per_strip=64)
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    want = oracle(oc.upright(px, 6), rc)
    # (orientation 1 of the turned pixels: the same geometry, nothing launched)
    cases = {6: (tif, want), 1: (im.tiff_bytes(oc.upright(px, 6), rows_per_strip=64), want)}
    held = {}
    for o, (t, w) in cases.items():
        enc = jp2hip.Encoder(0)
        d = DeviceBytes(t)  # the caller's buffer: the context holds no copy of the source
        try:
            enc.set_source_orientation(o)
            lay, keep = jp2hip.tiff_layout(t)
            got, _ = enc.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, rc)
            assert got == w, o
            held[o] = enc.device_bytes()
        finally:
            d.free()
            enc.close()
    assert held[6] - held[1] >= px.nbytes
    enc = jp2hip.Encoder(0)
    try:
        enc.set_source_orientation(6)
        enc.set_memory_limits(hard=held[6] - 1)
        with pytest.raises(jp2hip.Jp2hipError, match="device memory limit"):
            enc.encode_tiff(tif, jp2hip.LOSSLESS, rc)
        assert enc.device_bytes() <= held[6] - 1
        enc.set_memory_limits(hard=0)
        got, _ = enc.encode_tiff(tif, jp2hip.LOSSLESS, rc)
        assert got == want
    finally:
        enc.close()


def test_profile_mode_times_the_orientation():
    px = im.synth_rgb8(300, 530, seed=3)
    tif = im.tiff_bytes(px)
    enc = jp2hip.Encoder(0, profile=True)
    try:
        _, plain = enc.encode_tiff(tif, jp2hip.LOSSY)
        enc.set_source_orientation(6)
        _, turned = enc.encode_tiff(tif, jp2hip.LOSSY)
        assert turned.ingest_ms > plain.ingest_ms >= 0.0
    finally:
        enc.close()
