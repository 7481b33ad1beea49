"""TLM marker segments (ORGgen_tlm, jp2hip_set_organisation) on the GPU: every
file is compared byte for byte with the model of tests/tlm_cases.py (the
oracle's file with the segments inserted, which tests/test_tlm.py reads back
and decodes on the CPU; a rate-driven case: the oracle's file at the target
lowered by the segments' bytes).  Default and varied recipes, rate-driven
encodes, the five progression orders, the untiled recipe, three segments,
every encode route, one context switching the organisation, the host waits,
and the refusals.  No test touches the session's shared encoder's organisation.
"""
import threading

import numpy as np
import pytest

import imaging as im
import jp2hip
import progression_cases as pc
import tlm_cases as tc
from jp2hip import split as js

pytestmark = pytest.mark.gpu

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY


def same(got, want):
    d = pc.first_difference(bytes(got), want)
    assert d is None, d


@pytest.fixture(scope="module")
def tlm_encoder():
    """A context of this module's own with tlm = 1."""
    enc = jp2hip.Encoder(0)
    enc.set_organisation(tlm=1)
    yield enc
    enc.close()


_want = {}


def want_file(key, img, rc):
    """The expected file, made once per case."""
    if key not in _want:
        _want[key] = tc.expected(img, rc)
    return _want[key]


def encode(enc, img, conv, rc):
    return enc.encode_tiff(im.tiff_bytes(img), conv, rc)


# ---- lossless, the default recipe and its organisation switches ----------------------

LOSSLESS_VARIANTS = {"default": {}, "comment0": dict(comment=0), "flush0": dict(flush_period=0),
                     "tparts0": dict(tparts_r=0)}


@pytest.mark.parametrize("name", list(LOSSLESS_VARIANTS))
def test_lossless_default_recipe(tlm_encoder, name):
    img = tc.lossless_image()
    rc = jp2hip.recipe(LL, **LOSSLESS_VARIANTS[name])
    got, st = encode(tlm_encoder, img, LL, rc)
    want = want_file(("ll", name), img, rc)
    same(got, want)
    assert st.out_bytes == len(want)
    entries = tc.parse(got)
    tiles = [t for t, _ in entries]
    if name in ("default", "comment0"):  # two flush stripes, a tile-part per resolution
        assert tiles == [0, 1, 2, 3] * 7 + [4, 5] * 7 and tiles != sorted(tiles)
    elif name == "flush0":               # a stripe per tile row
        assert tiles == [0, 1] * 7 + [2, 3] * 7 + [4, 5] * 7
    else:
        assert tiles == [0, 1, 2, 3, 4, 5]


def test_lossless_file_decodes_to_the_source(tlm_encoder):
    img = tc.lossless_image()
    got, _ = encode(tlm_encoder, img, LL, jp2hip.recipe(LL))
    assert np.array_equal(im.decode_pillow(got), img)


# ---- rate-driven ---------------------------------------------------------------------

def test_rate_driven_counts_the_tlm_against_the_target(tlm_encoder, encoder):
    """The default lossy recipe: the tile-part bytes are the oracle's at
    target - T, which differ from those at the target (test_tlm.py)."""
    img = tc.lossless_image()
    rc = jp2hip.recipe(LY, **tc.LOSSY_T_SENSITIVE)
    got, st = encode(tlm_encoder, img, LY, rc)
    want = want_file("ly", img, rc)
    same(got, want)
    assert st.out_bytes == len(want)
    assert len(im.codestream(got)) <= tc.rate_target(rc.rate_bpp, 700, 1100)
    # the same recipe without the organisation stays the oracle's file at the target
    off, _ = encode(encoder, img, LY, rc)
    assert im.codestream(off)[tc.first_sot(im.codestream(off)):] != \
        im.codestream(got)[tc.first_sot(im.codestream(got)):]


def test_rate_driven_two_iterations_without_slope_skip(tlm_encoder):
    img, rc = tc.two_iteration_case()
    assert rc.slope_skip == 0
    got, st = encode(tlm_encoder, img, LY, rc)
    same(got, want_file("ly2", img, rc))
    assert st.rate_iterations == tc.TWO_ITERATION_COUNT


def test_rate_driven_over_the_target(tlm_encoder):
    img, rc = tc.over_target_case()
    got, st = encode(tlm_encoder, img, LY, rc)
    same(got, want_file("over", img, rc))
    assert st.rate_iterations == 8


# ---- progression orders --------------------------------------------------------------

ORDERS = [(o, 0) for o in range(5)] + [(pc.RLCP, 1), (pc.RPCL, 1)]


@pytest.mark.parametrize("order,tparts_r", ORDERS, ids=[f"{pc.NAMES[o]}-tparts{t}" for o, t in ORDERS])
def test_progression_orders(tlm_encoder, order, tparts_r):
    img, rc = tc.order_case(order, tparts_r)
    got, _ = encode(tlm_encoder, img, LL, rc)
    same(got, want_file(("order", order, tparts_r), img, rc))
    assert len(tc.parse(got)) == (36 if tparts_r else 12)


# ---- the untiled recipe, three segments ----------------------------------------------

def test_untiled_recipe(tlm_encoder):
    img, rc = tc.untiled_case()
    got, _ = encode(tlm_encoder, img, LL, rc)
    same(got, want_file("untiled", img, rc))
    assert [t for t, _ in tc.parse(got)] == [0] * 7


def test_three_segments(tlm_encoder):
    img, rc = tc.multi_segment_case()
    got, st = encode(tlm_encoder, img, LL, rc)
    want = want_file("multi", img, rc)
    same(got, want)
    entries = tc.parse(got)
    assert len(entries) == 22050 and [t for t, _ in entries] == list(range(11025)) * 2
    assert st.out_bytes == len(want)


# ---- routes --------------------------------------------------------------------------

ROUTE_CASES = {"lossless": (LL, {}, ("ll", "default")), "lossy": (LY, tc.LOSSY_T_SENSITIVE, "ly")}


@pytest.fixture(scope="module", params=list(ROUTE_CASES))
def route_case(request):
    """(conversion, recipe, TIFF bytes, expected file) of the first lossless and the first lossy case."""
    conv, ov, key = ROUTE_CASES[request.param]
    img = tc.lossless_image()
    rc = jp2hip.recipe(conv, **ov)
    return conv, rc, im.tiff_bytes(img, rows_per_strip=48), want_file(key, img, rc)


def test_route_encode_tiff_and_device(tlm_encoder, route_case):
    from devmem import DeviceBytes
    conv, rc, tif, want = route_case
    got, _ = tlm_encoder.encode_tiff(tif, conv, rc)
    same(got, want)
    lay, offs = jp2hip.tiff_layout(tif)
    d = DeviceBytes(tif)
    try:
        got, st = tlm_encoder.encode_device(d.ptr, d.nbytes, lay, conv, rc)
    finally:
        d.free()
    same(got, want)
    assert st.out_bytes == len(want)


def test_route_encode_file_single_gpu_and_split(tmp_path, route_case):
    conv, rc, tif, want = route_case
    src = tmp_path / "m.tif"
    src.write_bytes(tif)
    single, split, late = jp2hip.Encoder(0), jp2hip.Encoder(0), jp2hip.Encoder(0)
    try:
        single.set_organisation(tlm=1)
        split.split_peers([0])
        split.set_organisation(tlm=1)   # reaches the peer it has
        late.set_organisation(tlm=1)
        late.split_peers([0])           # a peer added later inherits it
        for name, enc in (("single", single), ("split", split), ("late", late)):
            out = tmp_path / f"{name}.jpx"
            st = enc.encode_file(str(src), str(out), conv, rc)
            same(out.read_bytes(), want)
            assert st.out_bytes == len(want), name
    finally:
        single.close()
        split.close()
        late.close()


@pytest.mark.parametrize("world", [2, 3])
def test_route_encode_device_split_over_thread_ranks(route_case, world):
    """Every rank holds only its band's strips; with three ranks over the two
    flush stripes rank 0's band is empty -- and rank 0 writes the main header
    with the TLM.  Parts, offsets and file_len against the expected file."""
    from devmem import DeviceBytes
    conv, rc, tif, want = route_case
    lay, offs = jp2hip.tiff_layout(tif)
    g = js.ThreadGroup(world)
    parts, errs, bands = [None] * world, [], [None] * world

    def work(r):
        try:
            enc = jp2hip.Encoder(0)
            try:
                enc.set_organisation(tlm=1)
                r0, r1 = js.split_rows(lay.height, rc.tile_h, r, world, rc.flush_period)
                bands[r] = (r0, r1)
                buf, blay, keep = js.band_strips(tif, lay, offs, r0, r1)
                d = DeviceBytes(buf or b"\0")
                try:
                    parts[r] = enc.encode_device_split(d.ptr, d.nbytes, blay, conv, g.member(r).split(), rc)
                finally:
                    d.free()
            finally:
                enc.close()
        except Exception as e:  # keep the other ranks from waiting forever
            errs.append(e)
            g.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    if errs:
        raise errs[0]
    assert sum(1 for r0, r1 in bands if r1 == r0) == (1 if world == 3 else 0)
    off = 0
    for part, file_offset, file_len, st in parts:
        assert file_offset == off and file_len == len(want)
        assert st.out_bytes == len(want)
        off += len(part)
    same(b"".join(p[0] for p in parts), want)


def test_route_batch_queue(tmp_path, route_case):
    from jp2hip import batch as jb
    conv, rc, tif, want = route_case
    src = tmp_path / "t.tif"
    src.write_bytes(tif)
    with jb.BatchQueue(contexts=1, delete_after_upload=False, tlm=True) as q:
        q.submit(1, "ark:/x/tlm", src, tmp_path / "batch.jpx", conv, rc)
        with pytest.raises(jp2hip.Jp2hipError):  # only before the first submit
            q.set_organisation(tlm=0)
        res = q.drain()
    assert res[0]["status"] == jb.OK, res[0]["message"]
    assert res[0]["out_bytes"] == len(want)
    same((tmp_path / "batch.jpx").read_bytes(), want)


def test_route_gpu_converter_keyword(tmp_path, monkeypatch):
    """GpuConverter(tlm=True): Converter.convert with the default recipe."""
    from jp2hip.converters import Conversion, GpuConverter
    monkeypatch.setattr("tempfile.tempdir", str(tmp_path))
    img = tc.lossless_image()
    src = tmp_path / "c.tif"
    src.write_bytes(im.tiff_bytes(img))
    conv = GpuConverter(devices=[0], per_gpu=1, tlm=True)
    try:
        jpx = conv.convert("ark:/x/conv", src, Conversion.LOSSLESS)
        same(jpx.read_bytes(), want_file(("ll", "default"), img, jp2hip.recipe(LL)))
    finally:
        conv.close()


# ---- one context: switching, host waits, refusals ------------------------------------

def test_switching_the_organisation_on_one_context():
    """Off, on, off on one geometry: the plan cache is keyed by the recipe
    alone and serves all three, each file the right one."""
    import oracle_lib as ol
    img = tc.lossless_image()
    tif = im.tiff_bytes(img)
    enc = jp2hip.Encoder(0)
    try:
        for conv, key in ((LL, ("ll", "default")), (LY, "ly")):
            rc = jp2hip.recipe(conv)
            off = ol.encode(img, ol.copy_recipe(rc))
            on = want_file(key, img, rc)
            for i, tlm in enumerate((0, 1, 0)):
                enc.set_organisation(tlm=tlm)
                got, st = enc.encode_tiff(tif, conv, rc)
                same(got, on if tlm else off)
                assert bool(st.reused & jp2hip._lib.REUSED_PLAN) == (i > 0), (conv, i, st.reused)
    finally:
        enc.close()


def test_host_waits_are_equal_with_and_without_tlm():
    img = tc.lossless_image()
    tif = im.tiff_bytes(img)
    enc = jp2hip.Encoder(0)
    try:
        for conv in (LL, LY):
            rc = jp2hip.recipe(conv)
            enc.encode_tiff(tif, conv, rc)  # warm: buffers, plan, pool
            waits = {}
            for tlm in (0, 1, 0, 1):
                enc.set_organisation(tlm=tlm)
                _, st = enc.encode_tiff(tif, conv, rc)
                waits.setdefault(tlm, []).append(st.host_waits)
            assert waits[0] == waits[1], (conv, waits)
    finally:
        enc.close()


@pytest.mark.parametrize("kw,field", [(dict(tlm=2), "tlm"), (dict(tlm=-1), "tlm"),
                                      (dict(tlm=1, reserved=(0, 1, 0)), "reserved")])
def test_refusals_name_the_field_and_change_nothing(kw, field):
    img, rc = tc.untiled_case()
    enc = jp2hip.Encoder(0)
    try:
        enc.set_organisation(tlm=1)
        with pytest.raises(jp2hip.Jp2hipError, match=field):
            enc.set_organisation(**kw)
        got, _ = encode(enc, img, LL, rc)  # still the organisation set before
        same(got, want_file("untiled", img, rc))
    finally:
        enc.close()
