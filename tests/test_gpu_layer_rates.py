"""Explicit per-layer rates (jp2hip_set_layer_rates) on the GPU.

1. One layer is the oracle's: set_layer_rates([r]) writes the oracle's file for
   rate_bpp = r, with its iteration count, on every rate-driven one-layer case
   of the PCRD corpus (the CPU suite shows they reach 1, 2 and 8 iterations).
2. Many layers are the slope path's: the file equals the slope-driven encode
   (merged, pinned to the oracle) at the thresholds the report names.
3. The loop is the model's: run_model of tests/layer_rate_cases.py, selecting
   by jp2hip.split.thresholds over the oracle's hull segments and sizing each
   iteration by a slope-driven encode's report, ends on the same thresholds,
   iteration count and per-layer bytes.
4. It fits: where the loop halts before its eighth iteration every targeted
   layer is within floor(rate * W * H / 8), TLM and tile-part divisions counted.
5. Extremes, 6. every route, 7. rates turned on and off on one context.
"""
import io
import math
import threading

import numpy as np
import pytest

import imaging as im
import jp2hip
import layer_rate_cases as lr
import oracle_lib as ol
import pcrd_cases as pc
import progression_cases as prc
from jp2hip import split as js

pytestmark = pytest.mark.gpu

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY
REUSED_PLAN = jp2hip._lib.REUSED_PLAN


def same(got, want):
    d = prc.first_difference(bytes(got), bytes(want))
    assert d is None, d


@pytest.fixture(scope="module")
def enc():
    """A context of this module's own (no test touches the session's shared one)."""
    e = jp2hip.Encoder(0)
    yield e
    e.close()


def by_rates(e, name, rates=None, **more):
    """(file, stats, report) of case `name` encoded by its rates on context e."""
    conv, rc = lr.recipe(name, **more)
    e.set_layer_rates(lr.rates(name) if rates is None else rates)
    try:
        got, st = e.encode_tiff(lr.tiff_of(name), conv, rc)
        return got, st, e.layer_report()
    finally:
        e.set_layer_rates(None)


def by_slopes(name, slopes, **more):
    """(file, report) of a slope-driven encode on a fresh context."""
    conv, rc = lr.recipe(name, **more)
    e = jp2hip.Encoder(0)
    try:
        e.set_layer_slopes(slopes)
        got, st = e.encode_tiff(lr.tiff_of(name), conv, rc)
        assert st.rate_iterations == 0
        return got, e.layer_report()
    finally:
        e.close()


_BASE = {}


def base(enc, name):
    """The rates encode of a case, once."""
    if name not in _BASE:
        _BASE[name] = by_rates(enc, name)
    return _BASE[name]


# ---- 1. one layer is the oracle's --------------------------------------------------------

ONE = lr.one_layer_cases()


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("case", ONE, ids=[c["name"] for c in ONE])
def test_one_layer_is_the_oracles(enc, case, skip):
    rcp = dict(case["recipe"], slope_skip=skip)
    want = ol.encode(pc.image(case), ol.copy_recipe(jp2hip.recipe(LY, **rcp)))
    iters = ol.lib().oracle_pcrd_export_iterations()
    # rate_bpp is no target with rates set: any positive value says "not lossless"
    rc = jp2hip.recipe(LY, **dict(rcp, rate_bpp=7.0))
    enc.set_layer_rates([rcp["rate_bpp"]])
    try:
        got, st = enc.encode_tiff(im.tiff_bytes(pc.image(case), rows_per_strip=16), LY, rc)
    finally:
        enc.set_layer_rates(None)
    if bytes(got) != want:
        raise AssertionError(pc.describe_mismatch(case, bytes(got), want))
    assert st.rate_iterations == iters, (case["name"], st.rate_iterations, iters)


# ---- 2. many layers are the slope path's ---------------------------------------------------

@pytest.mark.parametrize("name", lr.SLOPE_CASES)
def test_many_layers_are_the_slope_paths(enc, name):
    got, st, rep = base(enc, name)
    L = rep.layers
    assert 1 <= st.rate_iterations <= 8
    want, rep2 = by_slopes(name, list(rep.threshold[:L]))
    same(got, want)
    assert list(rep2.bytes[:L]) == list(rep.bytes[:L])


# ---- 3. the loop is the model's ------------------------------------------------------------

_MODEL = {}


def model(name):
    """run_model for a case without TLM or divisions (T = E = 0), once."""
    if name not in _MODEL:
        conv, rc = lr.recipe(name)
        t, b, info = lr.plan_numbers(name)
        assert info["T"] == info["E"] == 0
        e = jp2hip.Encoder(0)
        try:
            def size(K):
                e.set_layer_slopes(lr.slopes_of(K, conv == LL))
                e.encode_tiff(lr.tiff_of(name), conv, rc)
                rep = e.layer_report()
                return [int(x) + 2 for x in rep.bytes[:rc.layers]]
            _MODEL[name] = dict(lr.run_model(t, b, lr.select_on_segments(name), size), t=t)
        finally:
            e.close()
    return _MODEL[name]


# (and a case the loop leaves by its last door: eight iterations, layer 0 over at budget 0)
@pytest.mark.parametrize("name", lr.SLOPE_CASES + ("below_estimate",))
def test_the_loop_is_the_models(enc, name):
    conv, rc = lr.recipe(name)
    got, st, rep = base(enc, name)
    m = model(name)
    assert (m["iterations"] == 8 and not m["fits"]) if name == "below_estimate" else m["iterations"] < 8
    L = rc.layers
    for i, x in enumerate(m["trace"]):
        print(f"{name} it {i}: budgets {x['budgets']} S {x['S']} over {x['over']} (targets {m['t']})")
    assert st.rate_iterations == m["iterations"]
    assert list(rep.threshold[:L]) == lr.slopes_of(m["thresholds"], conv == LL)
    assert [int(x) + 2 for x in rep.bytes[:L]] == m["S"]
    if m["iterations"] < 8:   # 4. it fits
        assert m["fits"]
        W, H, _, _ = lr.geometry(name)
        for l, r in enumerate(lr.rates(name)):
            if m["t"][l] != lr.NO_TARGET:
                assert rep.bytes[l] + 2 <= math.floor(r * W * H / 8), (name, l)


def test_a_lower_layer_alone_takes_the_second_iteration():
    m = model(lr.LOWER_ONLY)
    L = len(m["t"])
    assert m["iterations"] >= 2
    assert all(x["over"] and max(x["over"]) < L - 1 for x in m["trace"][:-1]), m["trace"]


def test_equal_rates_trigger_the_clamp(enc):
    """Layers 1 and 2 have one rate: the clamp gives them one budget (layer
    1's own first budget is the larger: its header estimate is smaller), one
    threshold, and layer 2 adds no packet bytes."""
    name = lr.CLAMPED
    t, b, info = lr.plan_numbers(name)
    unclamped = lr.first_budgets_of(t, info["ntileparts"], info["npackets"])
    assert t[1] == t[2] and unclamped[1] > unclamped[2] and b[1] == b[2]
    m = model(name)
    assert all(x["budgets"][1] == x["budgets"][2] for x in m["trace"])
    got, st, rep = base(enc, name)
    assert rep.threshold[1] == rep.threshold[2]
    lb = im.packet_bytes_by_layer(im.codestream(bytes(got)), 3)
    # layer 2's packets are empty: SOP, one header byte, EPH
    assert lb[1] > 0 and rep.bytes[2] - rep.bytes[1] == lb[2] == 9 * (info["npackets"] // 3)


# ---- 4. it fits, with a TLM and with tile-part divisions -------------------------------------

def check_fits(name, st, rep, rates=None):
    W, H, _, _ = lr.geometry(name)
    conv, rc = lr.recipe(name)
    rates = lr.rates(name) if rates is None else rates
    for l, r in enumerate(rates):
        print(f"{name} layer {l}: {rep.bytes[l] + 2} of {math.floor(r * W * H / 8)} bytes, "
              f"{st.rate_iterations} iterations")
    if st.rate_iterations < 8:
        for l, r in enumerate(rates):
            if not (conv == LL and l == len(rates) - 1):
                assert rep.bytes[l] + 2 <= math.floor(r * W * H / 8), (name, l)


@pytest.mark.parametrize("org", ["tlm", "LC", "tlm+LC"])
@pytest.mark.parametrize("name", ["grey_ly3", "grey_ll4_org", "grey_ly3_low"])
def test_it_fits_with_tlm_and_divisions(name, org):
    e = jp2hip.Encoder(0)
    try:
        if "tlm" in org:
            e.set_organisation(tlm=1)
        if "LC" in org:
            e.set_tile_part_divisions("LC")
        got, st, rep = by_rates(e, name)
    finally:
        e.close()
    assert st.rate_iterations < 8   # (the case's rates leave room for T and E)
    check_fits(name, st, rep)
    assert rep.bytes[rep.layers - 1] + 2 == len(im.codestream(bytes(got)))
    check_decodes(name, bytes(got))


# ---- 5. extremes ---------------------------------------------------------------------------

def decode_layers(data: bytes, k: int) -> np.ndarray:
    from PIL import Image
    x = Image.open(io.BytesIO(data))
    x.layers = k
    x.load()
    return np.array(x)


def check_decodes(name, data: bytes):
    """Pillow / OpenJPEG decodes every prefix of layers; PSNR never decreases
    with the layer; a lossless top layer gives the source exactly."""
    conv, rc = lr.recipe(name)
    src = lr.image(name)
    bits = src.dtype.itemsize * 8
    last = -1.0
    for k in range(1, rc.layers + 1):
        dec = decode_layers(data, k).reshape(src.shape)
        p = im.psnr(dec, src, bits)
        assert p >= last, (name, k, p, last)
        last = p
    full = im.decode_pillow(data).reshape(src.shape)
    if conv == LL:
        assert np.array_equal(full, src), name


@pytest.mark.parametrize("name", list(lr.EXTREMES))
def test_extremes(enc, name):
    got, st, rep = by_rates(enc, name)
    got = bytes(got)
    conv, rc = lr.recipe(name)
    L = rc.layers
    check_fits(name, st, rep)
    assert rep.bytes[L - 1] + 2 == len(im.codestream(got)) and st.out_bytes == len(got)
    assert all(rep.bytes[l] <= rep.bytes[l + 1] for l in range(L - 1))
    check_decodes(name, got)
    lb = im.packet_bytes_by_layer(im.codestream(got), L)
    if name == "below_estimate":
        t, b, info = lr.plan_numbers(name)
        # the target is below the header estimate: budget 0, nothing selected --
        # every packet of layer 0 is SOP, one header byte and EPH
        assert b[0] == 0 and rc.sop == 1 and rc.eph == 1
        assert lb[0] == 9 * (info["npackets"] // L) and lb[1] > lb[0]
        assert rep.threshold[0] > rep.threshold[1]
    if name == "all_equal":
        assert len(set(rep.threshold[:L])) == 1 and rep.bytes[L - 1] - rep.bytes[0] == sum(lb[1:])
    again = bytes(by_rates(enc, name)[0])
    assert again == got, "two runs of one encode gave other bytes"


@pytest.mark.parametrize("name", lr.SLOPE_CASES)
def test_every_case_decodes(enc, name):
    check_decodes(name, bytes(base(enc, name)[0]))


# ---- 6. routes -----------------------------------------------------------------------------

def split_over_threads(name, world, more):
    from devmem import DeviceBytes
    conv, rc = lr.recipe(name, **more)
    tif = lr.tiff_of(name)
    lay, offs = jp2hip.tiff_layout(tif)
    g = js.ThreadGroup(world)
    parts, errs = [None] * world, []

    def work(r):
        try:
            e = jp2hip.Encoder(0)
            try:
                e.set_layer_rates(lr.rates(name))
                r0, r1 = js.split_rows(lay.height, rc.tile_h, r, world, rc.flush_period)
                assert r1 > r0
                buf, blay, keep = js.band_strips(tif, lay, offs, r0, r1)
                d = DeviceBytes(buf or b"\0")
                try:
                    parts[r] = e.encode_device_split(d.ptr, d.nbytes, blay, conv, g.member(r).split(), rc)
                finally:
                    d.free()
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
        assert file_offset == off
        off += len(part)
    return b"".join(p[0] for p in parts), [p[3].rate_iterations for p in parts]


@pytest.mark.parametrize("name,skip", [(lr.ROUTES[0], 0), (lr.ROUTES[0], 1), (lr.ROUTES[1], 0)])
def test_every_route_writes_the_encode_device_file(tmp_path, name, skip):
    from devmem import DeviceBytes
    from jp2hip import batch as jb
    more = dict(slope_skip=skip)
    conv, rc = lr.recipe(name, **more)
    tif = lr.tiff_of(name)
    lay, offs = jp2hip.tiff_layout(tif)
    src = tmp_path / "s.tif"
    src.write_bytes(tif)
    e = jp2hip.Encoder(0)
    try:
        e.set_layer_rates(lr.rates(name))
        d = DeviceBytes(tif)
        try:
            want, st0 = e.encode_device(d.ptr, d.nbytes, lay, conv, rc)
        finally:
            d.free()
        want = bytes(want)
        rep = e.layer_report()
        if skip:   # planes skipped: no slope equivalence, the properties hold
            check_fits(name, st0, rep)
            check_decodes(name, want)
        else:
            same(want, base_of(name))
        got, st = e.encode_tiff(tif, conv, rc)
        same(got, want)
        assert st.rate_iterations == st0.rate_iterations
        e.encode_file(str(src), str(tmp_path / "o.j2k"), conv, rc)
        same((tmp_path / "o.j2k").read_bytes(), want)
        # the library's own split: the context's ordinal repeated; peers get the rates set before them
        e.split_peers([0, 0])
        st = e.encode_file(str(src), str(tmp_path / "p.j2k"), conv, rc)
        same((tmp_path / "p.j2k").read_bytes(), want)
        assert st.rate_iterations == st0.rate_iterations
    finally:
        e.close()
    late = jp2hip.Encoder(0)
    try:   # ... and those set after them
        late.split_peers([0])
        late.set_layer_rates(lr.rates(name))
        late.encode_file(str(src), str(tmp_path / "q.j2k"), conv, rc)
        same((tmp_path / "q.j2k").read_bytes(), want)
    finally:
        late.close()
    for world in (2, 3):
        got, iters = split_over_threads(name, world, more)
        same(got, want)
        assert iters == [st0.rate_iterations] * world
    with jb.BatchQueue(contexts=1, delete_after_upload=False, layer_rates=lr.rates(name)) as q:
        q.submit(1, "ark:/x/rates", src, tmp_path / "batch.j2k", conv, rc)
        with pytest.raises(jp2hip.Jp2hipError):  # only before the first submit
            q.set_layer_rates(None)
        res = q.drain()
    assert res[0]["status"] == jb.OK, res[0]["message"]
    same((tmp_path / "batch.j2k").read_bytes(), want)


def base_of(name):
    e = jp2hip.Encoder(0)
    try:
        return bytes(by_rates(e, name)[0])
    finally:
        e.close()


def test_gpu_converter_keyword(tmp_path, monkeypatch):
    """GpuConverter(layer_rates=...): Converter.convert with the default
    lossless recipe, Bucketeer's "-rate -" with named lower layers."""
    from jp2hip.converters import Conversion, GpuConverter
    monkeypatch.setattr("tempfile.tempdir", str(tmp_path))
    img = lr.image("rgb_ll2")
    tif = im.tiff_bytes(img, rows_per_strip=16)
    src = tmp_path / "c.tif"
    src.write_bytes(tif)
    rates = [0.25, 0.5, 1.0, 2.0, 4.0, 0.0]
    conv = GpuConverter(devices=[0], per_gpu=1, layer_rates=rates)
    try:
        got = conv.convert("ark:/x/conv", src, Conversion.LOSSLESS).read_bytes()
    finally:
        conv.close()
    e = jp2hip.Encoder(0)
    try:
        e.set_layer_rates(rates)
        want, st = e.encode_tiff(tif, LL, jp2hip.recipe(LL))
    finally:
        e.close()
    same(got, want)
    assert np.array_equal(im.decode_pillow(got), img)


# ---- refusals at the encode; rates and slopes exclude each other ---------------------------------

def test_refusals_leave_the_context_usable():
    name = "grey_ly3"
    conv, rc = lr.recipe(name)
    e = jp2hip.Encoder(0)
    try:
        want = bytes(by_rates(e, name)[0])
        e.set_layer_rates([0.5, 1.0])
        with pytest.raises(jp2hip.Jp2hipError, match=r"n = 2.*layers = 3"):
            e.encode_tiff(lr.tiff_of(name), conv, rc)
        e.set_layer_rates([0.5, 1.0, 0.0])
        with pytest.raises(jp2hip.Jp2hipError, match=r"rates\[2\] is 0 with rate_bpp > 0"):
            e.encode_tiff(lr.tiff_of(name), conv, rc)
        e.set_layer_rates([0.5, 1.0, 2.0])
        with pytest.raises(jp2hip.Jp2hipError, match="last, must be 0"):
            e.encode_tiff(lr.tiff_of(name), LL, jp2hip.recipe(LL, **dict(lr.C16, layers=3)))
        with pytest.raises(jp2hip.Jp2hipError, match=r"rates\[1\] decreases"):
            e.set_layer_rates([1.0, 0.5, 2.0])
        with pytest.raises(jp2hip.Jp2hipError, match="jp2hip_set_layer_rates"):
            e.set_layer_slopes([4.0, 2.0, 1.0])     # rates, then slopes
        e.set_layer_rates(None)
        e.set_layer_slopes([4.0, 2.0, 1.0])
        with pytest.raises(jp2hip.Jp2hipError, match="jp2hip_set_layer_slopes"):
            e.set_layer_rates(lr.rates(name))       # slopes, then rates
        e.set_layer_slopes(None)
        got, st, _ = by_rates(e, name)
        same(got, want)
        assert not st.reused & jp2hip._lib.AFTER_FAILURE
    finally:
        e.close()


# ---- 7. history ------------------------------------------------------------------------------

def test_rates_on_and_off_on_one_context():
    """Lossless without rates, with, without; then lossy the same: each file
    is a fresh context's, and the plan is rebuilt exactly where the rate-control
    groups change (a lossless recipe: four flush stripes <-> one group)."""
    name_ll, name_ly = "grey_ll6_stripes", "grey_ly3"
    fresh = {}
    for key, name, on in (("ll", name_ll, False), ("ll+r", name_ll, True), ("ly", name_ly, False),
                          ("ly+r", name_ly, True)):
        e = jp2hip.Encoder(0)
        try:
            conv, rc = lr.recipe(name, **({} if conv_is_ll(name) else dict(rate_bpp=1.0)))
            e.set_layer_rates(lr.rates(name) if on else None)
            fresh[key] = bytes(e.encode_tiff(lr.tiff_of(name), conv, rc)[0])
        finally:
            e.close()
    assert fresh["ll"] != fresh["ll+r"] and fresh["ly"] != fresh["ly+r"]
    e = jp2hip.Encoder(0)
    try:
        #         key     rates  plan reused
        steps = (("ll", False, False), ("ll", False, True), ("ll+r", True, False), ("ll+r", True, True),
                 ("ll", False, False), ("ly", False, False), ("ly+r", True, True), ("ly+r", True, True),
                 ("ly", False, True))
        for i, (key, on, reused) in enumerate(steps):
            name = name_ll if key.startswith("ll") else name_ly
            conv, rc = lr.recipe(name, **({} if conv_is_ll(name) else dict(rate_bpp=1.0)))
            e.set_layer_rates(lr.rates(name) if on else None)
            got, st = e.encode_tiff(lr.tiff_of(name), conv, rc)
            same(got, fresh[key])
            assert bool(st.reused & REUSED_PLAN) == reused, (i, key, st.reused)
    finally:
        e.close()


def conv_is_ll(name):
    return lr.ALL[name][1] == LL
