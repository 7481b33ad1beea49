"""Fixed-slope quality layers (jp2hip_set_layer_slopes) and the per-layer
report on the GPU.  Every expectation comes from the oracle alone
(tests/slope_cases.py): at slopes = Kc of the oracle's own final selection the
library must write the oracle's file byte for byte, COM included; anywhere in
[Kc, K] the same file outside the COM's slope column.  With a TLM, with
tile-part divisions and in LRCP the expected file is made by the helpers of
tlm_cases, tparts_cases and progression_cases from the same oracle file --
at the full rate: with slopes there is no target for T or E to lower.  Then
every encode route, a short decision-stream pool, slopes set and cleared on
one context, the refusal of a wrong count, and the report: bytes against the
file, distortion against the sums derived from the oracle's export (1e-9
relative: about 1e5 terms of 2^-53 each), equal bits on a repeat, NaN when
not enabled, and on the levels = 0 case the decoder's squared error.
"""
import math
import threading

import numpy as np
import pytest

import imaging as im
import jp2hip
import oracle_lib as ol
import progression_cases as pc
import slope_cases as sc
import tlm_cases as tc
import tparts_cases as tp
from jp2hip import split as js

pytestmark = pytest.mark.gpu

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY


def same(got, want):
    d = pc.first_difference(bytes(got), want)
    assert d is None, d


@pytest.fixture(scope="module")
def enc():
    """A context of this module's own (no test touches the session's shared one)."""
    e = jp2hip.Encoder(0)
    yield e
    e.close()


def tiff_of(name):
    return im.tiff_bytes(sc.image(name), rows_per_strip=16)


def bits_of(name):
    return sc.image(name).dtype.itemsize * 8


def encode(e, name, slopes, rc=None):
    conv, rc0 = sc.recipe(name)
    e.set_layer_slopes(slopes)
    try:
        return e.encode_tiff(tiff_of(name), conv, rc if rc is not None else rc0)
    finally:
        e.set_layer_slopes(None)


# ---- byte identity at slopes = Kc ------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in sc.CASES if n != "lossless_lrcp"])
def test_identical_to_the_oracle_at_kc(enc, name):
    x = sc.expectation(name)
    got, st = encode(enc, name, x["slopes"])
    same(got, x["file"])
    assert st.rate_iterations == 0 and st.out_bytes == len(x["file"])


def test_slope_skip_is_ignored(enc):
    """The recipe asks for slope prediction; the expected file is the oracle's
    with every plane coded, and every plane was coded."""
    conv, rc = sc.recipe("slope_skip_1")
    assert rc.slope_skip == 1
    x = sc.expectation("slope_skip_1")
    got, st = encode(enc, "slope_skip_1", x["slopes"])
    same(got, x["file"])
    _, st0 = encode(enc, "rgb_2.0bpp_6ly", x["slopes"])
    assert st.coded_passes == st0.coded_passes and st.t1_bytes == st0.t1_bytes


# ---- anywhere in [Kc, K] ----------------------------------------------------------------

@pytest.mark.parametrize("where", ["top", "halfway"])
@pytest.mark.parametrize("name", ["rgb_2.0bpp_12ly", "grey16_2bpp", "p128_1bpp", "lossless_one_group"])
def test_the_interval_selects_the_same_passes(enc, name, where):
    conv, rc = sc.recipe(name)
    x = sc.expectation(name)
    given = x["top"] if where == "top" else [sc.halfway(a, b) for a, b in zip(x["slopes"], x["top"])]
    assert given != x["slopes"]
    got, _ = encode(enc, name, given)
    same(got, sc.with_slope_column(x["file"], rc.layers, given, bits_of(name)))
    assert [b for _, b in sc.com_lines(bytes(got), rc.layers)] == [b for _, b in sc.com_lines(x["file"], rc.layers)]


# ---- with a TLM, with tile-part divisions, in LRCP ---------------------------------------

@pytest.mark.parametrize("name", ["lossless_one_group", "rgb_2.0bpp_6ly"])
def test_with_tlm(name):
    conv, rc = sc.recipe(name)
    x = sc.expectation(name)
    e = jp2hip.Encoder(0)
    try:
        e.set_organisation(tlm=1)
        got, st = encode(e, name, x["slopes"])
    finally:
        e.close()
    want = tc.with_tlm(x["file"], tc.layout_of(sc.image(name)), rc.format)
    same(got, want)
    assert st.out_bytes == len(want) and tc.parse(bytes(got))


@pytest.mark.parametrize("name", ["lossless_one_group", "rgb_2.0bpp_6ly"])
def test_with_tile_parts_per_layer(name):
    conv, rc = sc.recipe(name)
    x = sc.expectation(name)
    e = jp2hip.Encoder(0)
    try:
        e.set_tile_part_divisions("L")
        got, _ = encode(e, name, x["slopes"])
    finally:
        e.close()
    want = tp.divide(x["file"], tp.L, rc, tc.layout_of(sc.image(name)))
    assert want != x["file"]
    same(got, want)


def test_in_lrcp(enc):
    name = "lossless_lrcp"
    conv, rc = sc.recipe(name)
    assert rc.progression == pc.LRCP
    x = sc.expectation(name)
    got, _ = encode(enc, name, x["slopes"])
    same(got, pc.resequence(x["file"], pc.LRCP))


# ---- routes ----------------------------------------------------------------------------

ROUTE_CASES = ["lossless_four_groups", "p128_1bpp"]


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_route_encode_device_and_file(tmp_path, enc, name):
    from devmem import DeviceBytes
    conv, rc = sc.recipe(name)
    x = sc.expectation(name)
    tif = tiff_of(name)
    lay, offs = jp2hip.tiff_layout(tif)
    src = tmp_path / "s.tif"
    src.write_bytes(tif)
    enc.set_layer_slopes(x["slopes"])
    try:
        d = DeviceBytes(tif)
        try:
            got, st = enc.encode_device(d.ptr, d.nbytes, lay, conv, rc)
        finally:
            d.free()
        same(got, x["file"])
        st = enc.encode_file(str(src), str(tmp_path / "o.jpx"), conv, rc)
        same((tmp_path / "o.jpx").read_bytes(), x["file"])
        assert st.rate_iterations == 0
    finally:
        enc.set_layer_slopes(None)


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_route_split_peers(tmp_path, name):
    """Two ranks inside the library; peers get the slopes when they are set
    and inherit them when added later."""
    conv, rc = sc.recipe(name)
    x = sc.expectation(name)
    src = tmp_path / "s.tif"
    src.write_bytes(tiff_of(name))
    early, late = jp2hip.Encoder(0), jp2hip.Encoder(0)
    try:
        early.split_peers([0])
        early.set_layer_slopes(x["slopes"])
        early.set_layer_report(1)
        late.set_layer_slopes(x["slopes"])
        late.set_layer_report(1)
        late.split_peers([0])
        for tag, e in (("early", early), ("late", late)):
            out = tmp_path / f"{tag}.jpx"
            st = e.encode_file(str(src), str(out), conv, rc)
            same(out.read_bytes(), x["file"])
            assert st.rate_iterations == 0, tag
            check_report(e.layer_report(), name, x)
    finally:
        early.close()
        late.close()


def split_over_threads(name, world, slopes, report=True):
    """The callback split over `world` thread ranks: (file, rank 0's report)."""
    from devmem import DeviceBytes
    conv, rc = sc.recipe(name)
    tif = tiff_of(name)
    lay, offs = jp2hip.tiff_layout(tif)
    g = js.ThreadGroup(world)
    parts, errs, reports = [None] * world, [], [None] * world

    def work(r):
        try:
            e = jp2hip.Encoder(0)
            try:
                e.set_layer_slopes(slopes)
                e.set_layer_report(1 if report else 0)
                r0, r1 = js.split_rows(lay.height, rc.tile_h, r, world, rc.flush_period)
                buf, blay, keep = js.band_strips(tif, lay, offs, r0, r1)
                d = DeviceBytes(buf or b"\0")
                try:
                    parts[r] = e.encode_device_split(d.ptr, d.nbytes, blay, conv, g.member(r).split(), rc)
                finally:
                    d.free()
                if r == 0:
                    reports[0] = e.layer_report()
            finally:
                e.close()
        except Exception as ex:  # keep the other ranks from waiting forever
            errs.append(ex)
            g.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    if errs:
        raise errs[0]
    off = 0
    for part, file_offset, file_len, st in parts:
        assert file_offset == off and st.rate_iterations == 0
        off += len(part)
    return b"".join(p[0] for p in parts), reports[0]


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("name", ROUTE_CASES)
def test_route_callback_split(name, world):
    x = sc.expectation(name)
    got, rep = split_over_threads(name, world, x["slopes"])
    same(got, x["file"])
    check_report(rep, name, x)


def test_route_batch_queue(tmp_path):
    from jp2hip import batch as jb
    name = "lossless_four_groups"
    conv, rc = sc.recipe(name)
    x = sc.expectation(name)
    src = tmp_path / "t.tif"
    src.write_bytes(tiff_of(name))
    with jb.BatchQueue(contexts=1, delete_after_upload=False, layer_slopes=x["slopes"]) as q:
        q.submit(1, "ark:/x/slopes", src, tmp_path / "batch.jpx", conv, rc)
        with pytest.raises(jp2hip.Jp2hipError):  # only before the first submit
            q.set_layer_slopes(None)
        res = q.drain()
    assert res[0]["status"] == jb.OK, res[0]["message"]
    same((tmp_path / "batch.jpx").read_bytes(), x["file"])


def test_route_gpu_converter_keyword(tmp_path, monkeypatch):
    """GpuConverter(layer_slopes=...): Converter.convert with the default recipe."""
    from jp2hip.converters import Conversion, GpuConverter
    monkeypatch.setattr("tempfile.tempdir", str(tmp_path))
    name = "default_recipe"
    x = sc.expectation(name)
    src = tmp_path / "c.tif"
    src.write_bytes(tiff_of(name))
    conv = GpuConverter(devices=[0], per_gpu=1, layer_slopes=x["slopes"])
    try:
        same(conv.convert("ark:/x/conv", src, Conversion.LOSSLESS).read_bytes(), x["file"])
    finally:
        conv.close()


# ---- a short pool, history, a wrong count -------------------------------------------------

@pytest.mark.parametrize("name", ["rgb_8.0bpp_6ly", "lossless_one_group"])
def test_short_decision_stream_pool(monkeypatch, name):
    monkeypatch.setenv("JP2HIP_TEST_POOL_FRAC", "0.02")
    e = jp2hip.Encoder(0)
    monkeypatch.delenv("JP2HIP_TEST_POOL_FRAC")
    try:
        x = sc.expectation(name)
        got, st = encode(e, name, x["slopes"])
        same(got, x["file"])
        assert st.pool_grows >= 1 and st.rate_iterations == 0
    finally:
        e.close()


@pytest.mark.parametrize("name", ["rgb_2.0bpp_6ly", "lossless_four_groups"])
def test_slopes_set_then_cleared(name):
    """Slopes on, then off: the next encode is the plain oracle file of the
    recipe, on the plan the slope-driven encode built."""
    conv, rc = sc.recipe(name)
    x = sc.expectation(name)
    plain = ol.encode(sc.image(name), ol.copy_recipe(rc))
    e = jp2hip.Encoder(0)
    try:
        tif = tiff_of(name)
        e.set_layer_slopes(x["top"] if x["groups"] == 1 else x["slopes"])
        got, st = e.encode_tiff(tif, conv, rc)
        assert not st.reused & jp2hip._lib.REUSED_PLAN
        e.set_layer_slopes(None)
        got, st = e.encode_tiff(tif, conv, rc)
        same(got, plain)
        assert st.reused & jp2hip._lib.REUSED_PLAN
        assert st.rate_iterations >= 1
        e.set_layer_slopes(x["slopes"])
        got, st = e.encode_tiff(tif, conv, rc)
        same(got, x["file"])
        assert st.reused & jp2hip._lib.REUSED_PLAN and st.rate_iterations == 0
    finally:
        e.close()


def test_a_wrong_count_is_refused_and_the_context_stays_usable():
    name = "rgb_2.0bpp_6ly"
    conv, rc = sc.recipe(name)
    x = sc.expectation(name)
    e = jp2hip.Encoder(0)
    try:
        e.set_layer_slopes(x["slopes"][:3])
        with pytest.raises(jp2hip.Jp2hipError, match=r"n = 3.*layers = 6"):
            e.encode_tiff(tiff_of(name), conv, rc)
        with pytest.raises(jp2hip.Jp2hipError, match=r"slopes\[1\] increases"):
            e.set_layer_slopes([1.0, 2.0])
        with pytest.raises(jp2hip.Jp2hipError, match="last, must be 0"):  # lossless recipe, last threshold not 0
            e.encode_tiff(tiff_of(name), LL, jp2hip.recipe(LL, layers=3, tile_w=256, tile_h=256, levels=3))
        e.set_layer_slopes(x["slopes"])
        got, st = e.encode_tiff(tiff_of(name), conv, rc)
        same(got, x["file"])
        assert not st.reused & jp2hip._lib.AFTER_FAILURE
    finally:
        e.close()


# ---- the report ----------------------------------------------------------------------------

def check_report(rep, name, x, distortion=True):
    conv, rc = sc.recipe(name)
    L = rc.layers
    assert rep.layers == L
    assert list(rep.threshold[:L]) == x["slopes"]
    layers, ends = tc.layer_ends(im.codestream(x["file"]), 0)
    assert layers == L and list(rep.bytes[:L]) == ends
    assert ["%8.1e" % float(b) for b in rep.bytes[:L]] == [b for _, b in sc.com_lines(x["file"], L)]
    if not distortion:
        assert rep.distortion_valid == 0 and all(math.isnan(d) for d in rep.distortion[:L])
        return
    assert rep.distortion_valid == 1
    for l in range(L):
        want = x["distortion"][l]
        print(f"{name} layer {l}: report {rep.distortion[l]!r}, export {want!r}")
        assert abs(rep.distortion[l] - want) <= 1e-9 * want, (name, l, rep.distortion[l], want)


REPORT_CASES = ["rgb_2.0bpp_12ly", "rgb_8.0bpp_6ly", "grey16_2bpp", "p128_1bpp", "lossless_one_group",
                "lossless_four_groups", "levels0", "levels3"]


@pytest.mark.parametrize("name", REPORT_CASES)
def test_report_bytes_thresholds_and_distortion(name):
    x = sc.expectation(name)
    e = jp2hip.Encoder(0)
    try:
        with pytest.raises(jp2hip.Jp2hipError, match="no encode"):
            e.layer_report()
        got, _ = encode(e, name, x["slopes"])
        same(got, x["file"])
        check_report(e.layer_report(), name, x, distortion=False)  # not enabled: NaN
        e.set_layer_report(1)
        got, _ = encode(e, name, x["slopes"])
        same(got, x["file"])
        first = e.layer_report()
        check_report(first, name, x)
        encode(e, name, x["slopes"])
        again = e.layer_report()
        assert bytes(first) == bytes(again), "a repeat gave other bits"
        e.set_layer_report(0)
        encode(e, name, x["slopes"])
        check_report(e.layer_report(), name, x, distortion=False)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["rgb_2.0bpp_6ly", "lossless_four_groups"])
def test_report_of_an_encode_without_slopes(name):
    """The report describes any encode: a rate-driven or lossless one reports
    the thresholds it chose (Kc), the same bytes and the same distortion."""
    conv, rc = sc.recipe(name)
    x = sc.expectation(name)
    e = jp2hip.Encoder(0)
    try:
        e.set_layer_report(1)
        got, st = e.encode_tiff(tiff_of(name), conv, rc)
        same(got, x["file"])
        assert st.rate_iterations >= 1
        check_report(e.layer_report(), name, x)
    finally:
        e.close()


def test_report_psnr_helper(enc):
    name = "levels0"
    x = sc.expectation(name)
    enc.set_layer_report(1)
    try:
        encode(enc, name, x["slopes"])
        rep = enc.layer_report()
    finally:
        enc.set_layer_report(0)
    h, w = sc.image(name).shape
    for l in range(5):
        assert abs(rep.psnr(l, w, h, 1, 8) - 10 * math.log10(255.0 ** 2 * w * h / rep.distortion[l])) < 1e-9
    assert rep.psnr(5, w, h, 1, 8) == math.inf


@pytest.mark.skipif(im.opj("opj_decompress") is None, reason="opj_decompress not installed")
def test_report_levels0_is_the_decoded_squared_error(enc):
    """levels = 0: the device's sums against the image a decoder makes of the
    first l + 1 layers, within 0.2 % at every layer."""
    name = "levels0"
    x = sc.expectation(name)
    enc.set_layer_report(1)
    try:
        got, _ = encode(enc, name, x["slopes"])
        rep = enc.layer_report()
    finally:
        enc.set_layer_report(0)
    img = sc.image(name).astype(np.int64)
    for l in range(rep.layers):
        dec = im.decode_opj(bytes(got), layers=l + 1).astype(np.int64).reshape(img.shape)
        sse = float(((dec - img) ** 2).sum())
        print(f"layer {l}: report {rep.distortion[l]:.6g}, decoded SSE {sse:.6g}")
        assert abs(rep.distortion[l] - sse) <= 2e-3 * sse, (l, rep.distortion[l], sse)
