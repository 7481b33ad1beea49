"""Quality layers by target PSNR (jp2hip_set_layer_psnr) on the GPU.

Thresholds: for every case of tests/psnr_cases.py the report's thresholds
after the PSNR-driven encode are the model's K, bit for bit, and the file is
the one jp2hip_set_layer_slopes gives at those thresholds on a fresh context.
Oracle anchor: targets that land on the thresholds of the oracle's own
rate-driven selection give the oracle's file (its COM's slope column rendered
from the keys, as tests/test_gpu_slopes.py does for thresholds inside [Kc, K]).
Routes: encode_tiff, encode_device, encode_file, the batch queue, the
in-process split over 2 and 3 ranks and the callback split over 2.
Truth: at levels = 0 a Pillow decode of the first l + 1 layers reaches the
target, and the selection one tie group smaller does not -- both within the
0.2 % the layer report's exactness test (tests/test_gpu_slopes.py) allows
between the estimate and a decoder's squared error.
Recipes, and a context's history.
"""
import io
import math
import threading

import numpy as np
import pytest

import imaging as im
import jp2hip
import oracle_lib as ol
import pcrd_cases as pc
import pixel_format_cases as pf
import psnr_cases as pq
import slope_cases as sc
from jp2hip import split as js

pytestmark = pytest.mark.gpu

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY
ESTIMATE_TOL = 2e-3   # tests/test_gpu_slopes.py::test_report_levels0_is_the_decoded_squared_error


def same(got, want):
    import progression_cases as prc
    d = prc.first_difference(bytes(got), bytes(want))
    assert d is None, d


def recipe_of(c):
    conv = LL if c["lossless"] else LY
    return conv, jp2hip.recipe(conv, **c["recipe"])


def tiff_of(c):
    return im.tiff_bytes(pq.image(c), rows_per_strip=16)


_PSNR = {}


def psnr_for(c):
    """(psnr targets in dB, the model's K) of a corpus case: each integer
    target searched as a PSNR whose jp2hip_layer_psnr_targets integer it is."""
    if c["name"] not in _PSNR:
        targets, K, _ = pq.wanted(c)
        fn = lambda p: jp2hip.layer_psnr_targets(pc.SIDE, pc.SIDE, 1, c["bits"], [p])[0]
        ps = []
        for t in targets:
            if t < 0:
                ps.append(0.0)
            else:
                t = min(t, fn(1e-3))   # (a target above the image's at 0.001 dB: that one takes nothing too)
                ps.append(pq.find_psnr(fn, t))
        assert all(b >= a for a, b in zip(ps, ps[1:]) if b != 0.0), (c["name"], ps)
        assert jp2hip.layer_psnr_targets(pc.SIDE, pc.SIDE, 1, c["bits"], ps) == [
            t if t < 0 else min(t, fn(1e-3)) for t in targets]
        _PSNR[c["name"]] = (ps, K)
    return _PSNR[c["name"]]


def keys_of(rep, L):
    return [pq.key_of(t) for t in rep.threshold[:L]]


def by_slopes(tif, conv, rc, slopes, setup=None):
    e = jp2hip.Encoder(0)
    try:
        if setup:
            setup(e)
        e.set_layer_slopes(slopes)
        return e.encode_tiff(tif, conv, rc)
    finally:
        e.close()


@pytest.fixture(scope="module")
def enc():
    e = jp2hip.Encoder(0)
    yield e
    e.close()


# ---- thresholds and file identity ---------------------------------------------------------

@pytest.mark.parametrize("name", [c["name"] for c in pq.cases()])
def test_thresholds_are_the_models_and_the_file_is_the_slope_driven_one(enc, name):
    c = pq.by_name(name)
    conv, rc = recipe_of(c)
    ps, K = psnr_for(c)
    enc.set_layer_psnr(ps)
    try:
        got, st = enc.encode_tiff(tiff_of(c), conv, rc)
        rep = enc.layer_report()
    finally:
        enc.set_layer_psnr(None)
    print(name, ps, [hex(k) for k in keys_of(rep, rc.layers)], [hex(k) for k in K])
    assert keys_of(rep, rc.layers) == K
    assert st.rate_iterations == 0
    want, _ = by_slopes(tiff_of(c), conv, rc, list(rep.threshold[:rc.layers]))
    same(got, want)


# ---- the oracle's own selection ------------------------------------------------------------

@pytest.mark.parametrize("name", ["extremes_noise_b6000_p128", "ties_tie65_exact_p128", "nearties_b9000_p1",
                                  "ties_tie190_exact_ly3_p1"])
def test_oracle_anchor(enc, name):
    c = pc.by_name(name)
    m = pc.measure(c)
    L = c["recipe"]["layers"]
    layers = sorted(m["export"]["layers"], key=lambda x: x["layer"])
    segs = pq.segments(m["export"], c["bits"])
    groups = pq.groups_of(segs)
    total = groups[-1]["upper"]
    by_key = {g["key"]: g for g in groups}
    # a layer in which the oracle took nothing (K = all ones): its Kc, one
    # above the largest key, is what a target everything meets gives
    NONE = (1 << 64) - 1
    assert all(l["Kc"] == groups[0]["key"] + 1 for l in layers if l["K"] == NONE)
    K = [l["Kc"] if l["K"] == NONE else l["K"] for l in layers]
    targets = [total if l["K"] == NONE else total - by_key[l["K"]]["upper"] for l in layers]
    assert pq.thresholds(segs, targets) == K
    fn = lambda p: jp2hip.layer_psnr_targets(pc.SIDE, pc.SIDE, 1, c["bits"], [p])[0]
    ps = [pq.find_psnr(fn, t) for t in targets]
    conv = LY
    rc = jp2hip.recipe(conv, **c["recipe"])
    enc.set_layer_psnr(ps)
    try:
        got, st = enc.encode_tiff(im.tiff_bytes(pc.image(c), rows_per_strip=16), conv, rc)
        rep = enc.layer_report()
    finally:
        enc.set_layer_psnr(None)
    assert keys_of(rep, L) == K
    same(got, sc.with_slope_column(m["file"], L, [pq.slope_of(k) for k in K], c["bits"]))


# ---- routes ----------------------------------------------------------------------------------

ROUTE_CASES = ["tie190_p128", "tie100mix_p128", "lossless_top_p128"]


@pytest.mark.parametrize("name", ROUTE_CASES[:2])
def test_route_cases_straddle_both_flush_stripes(name):
    """What the split tests rest on, from the export (no GPU work): the tie
    group the five layers are aimed at has segments in blocks of both flush
    stripes -- block rows 0..7 (the first 128 blocks) and 8..15 -- so both
    ranks of a two-rank split own part of it."""
    c = pq.by_name(name)
    _, K, _ = pq.wanted(c)
    blocks = {b for k, _, b in pq.measure(c)["segs"] if k == K[2]}
    assert c["recipe"]["flush_period"] == 128 and pc.SIDE == 256
    assert any(b < pc.NB // 2 for b in blocks) and any(b >= pc.NB // 2 for b in blocks), sorted(blocks)[:8]


def single(c):
    conv, rc = recipe_of(c)
    ps, K = psnr_for(c)
    e = jp2hip.Encoder(0)
    try:
        e.set_layer_psnr(ps)
        got, _ = e.encode_tiff(tiff_of(c), conv, rc)
        assert keys_of(e.layer_report(), rc.layers) == K
        return bytes(got)
    finally:
        e.close()


@pytest.mark.parametrize("name", ROUTE_CASES[:2])
def test_route_encode_device_file_and_batch(tmp_path, name):
    from devmem import DeviceBytes
    from jp2hip import batch as jb
    c = pq.by_name(name)
    conv, rc = recipe_of(c)
    ps, K = psnr_for(c)
    want = single(c)
    tif = tiff_of(c)
    lay, offs = jp2hip.tiff_layout(tif)
    src = tmp_path / "s.tif"
    src.write_bytes(tif)
    e = jp2hip.Encoder(0)
    try:
        e.set_layer_psnr(ps)
        d = DeviceBytes(tif)
        try:
            got, st = e.encode_device(d.ptr, d.nbytes, lay, conv, rc)
        finally:
            d.free()
        same(got, want)
        st = e.encode_file(str(src), str(tmp_path / "o.jpx"), conv, rc)
        same((tmp_path / "o.jpx").read_bytes(), want)
        assert st.rate_iterations == 0
    finally:
        e.close()
    with jb.BatchQueue(contexts=1, delete_after_upload=False, layer_psnr=ps) as q:
        q.submit(1, "ark:/x/psnr", src, tmp_path / "batch.jpx", conv, rc)
        with pytest.raises(jp2hip.Jp2hipError):  # only before the first submit
            q.set_layer_psnr(None)
        res = q.drain()
    assert res[0]["status"] == jb.OK, res[0]["message"]
    same((tmp_path / "batch.jpx").read_bytes(), want)


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("name", ROUTE_CASES)
def test_route_split_peers(tmp_path, name, ranks):
    """Two flush stripes (flush_period 128 of 256 rows), the tie group's
    blocks in both (test_route_cases_straddle_both_flush_stripes): with two
    ranks each owns segments of it; with three, one rank has no stripe and
    joins the exchange with no segments.  Peers get the targets when they are
    set and inherit them when added later."""
    c = pq.by_name(name)
    conv, rc = recipe_of(c)
    ps, K = psnr_for(c)
    want = single(c)
    src = tmp_path / "s.tif"
    src.write_bytes(tiff_of(c))
    early, late = jp2hip.Encoder(0), jp2hip.Encoder(0)
    try:
        early.split_peers([0] * (ranks - 1))
        early.set_layer_psnr(ps)
        late.set_layer_psnr(ps)
        late.split_peers([0] * (ranks - 1))
        for tag, e in (("early", early), ("late", late)):
            out = tmp_path / f"{tag}.jpx"
            st = e.encode_file(str(src), str(out), conv, rc)
            same(out.read_bytes(), want)
            assert st.rate_iterations == 0, tag
            assert keys_of(e.layer_report(), rc.layers) == K
    finally:
        early.close()
        late.close()


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_route_callback_split(name):
    from devmem import DeviceBytes
    world = 2
    c = pq.by_name(name)
    conv, rc = recipe_of(c)
    ps, K = psnr_for(c)
    want = single(c)
    tif = tiff_of(c)
    lay, offs = jp2hip.tiff_layout(tif)
    g = js.ThreadGroup(world)
    parts, errs = [None] * world, []

    def work(r):
        try:
            e = jp2hip.Encoder(0)
            try:
                e.set_layer_psnr(ps)
                r0, r1 = js.split_rows(lay.height, rc.tile_h, r, world, rc.flush_period)
                assert r1 > r0
                buf, blay, keep = js.band_strips(tif, lay, offs, r0, r1)
                d = DeviceBytes(buf or b"\0")
                try:
                    parts[r] = e.encode_device_split(d.ptr, d.nbytes, blay, conv, g.member(r).split(), rc)
                finally:
                    d.free()
                if r == 0:
                    assert keys_of(e.layer_report(), rc.layers) == K
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
    assert all(p[3].rate_iterations == 0 for p in parts)
    same(b"".join(p[0] for p in parts), want)


# ---- truth: a decoder's PSNR ---------------------------------------------------------------

def _truth_image(bits):
    r = np.random.default_rng(20261021 + bits)
    yy, xx = np.mgrid[0:64, 0:64]
    amp = (1 << (bits - 1)) - 1
    a = 0.6 * amp * np.sin(xx * 0.21 + yy * 0.13) + r.normal(0, amp * 0.08, (64, 64))
    a = np.rint(a).clip(-amp, amp) + (1 << (bits - 1))
    return a.astype(np.uint16 if bits == 16 else np.uint8)


def _decode(data, layers):
    from PIL import Image
    img = Image.open(io.BytesIO(bytes(data)))
    # (Pillow's load() passes `layers` on only together with a reduce: the
    # decoder's arguments -- codec, reduce, layers, fd, length -- set here)
    t = img.tile[0]
    img.tile = [type(t)(t[0], t[1], t[2], (t[3][0], 0, layers, t[3][3], t[3][4]))]
    img.load()
    return np.array(img).astype(np.int64)


@pytest.mark.parametrize("bits,targets", [(8, [24.0, 31.0, 38.0, 45.0]), (16, [30.0, 45.0, 60.0, 75.0])])
def test_truth_a_decoder_measures_the_target(enc, bits, targets):
    """On the reversible path, where the tolerance was established (the
    layer report's exact case is the lossless recipe at levels = 0) and D is
    all there is: the irreversible path's quantisation error is by definition
    no part of D (jp2hip.h), and at the higher targets it is far more than
    0.2 % of what the target allows (step 1 at 8 bits: 1/4 a sample against an
    allowed 2 a sample at 45 dB).  The top layer is the lossless one."""
    img = _truth_image(bits)
    rc = jp2hip.recipe(LL, levels=0, mct=0, tile_w=64, tile_h=64, cblk_w_log2=4, cblk_h_log2=4,
                       layers=len(targets) + 1, format=0, nprecincts=0)
    tif = im.tiff_bytes(img, rows_per_strip=16)
    enc.set_layer_psnr(targets + [0.0])
    try:
        got, _ = enc.encode_tiff(tif, LL, rc)
        rep = enc.layer_report()
    finally:
        enc.set_layer_psnr(None)
    assert np.array_equal(_decode(got, len(targets) + 1), img)
    peak2n = float((1 << bits) - 1) ** 2 * img.size
    src = img.astype(np.int64)
    fewer = [math.nextafter(t, math.inf) for t in rep.threshold[:len(targets)]] + [0.0]   # one tie group smaller
    less, _ = by_slopes(tif, LL, rc, fewer)
    for l, t in enumerate(targets):
        allowed = peak2n / 10.0 ** (t / 10.0)
        sse = float(((_decode(got, l + 1) - src) ** 2).sum())
        sse_less = float(((_decode(less, l + 1) - src) ** 2).sum())
        print(f"{bits}-bit layer {l}: target {t} dB = SSE {allowed:.6g}; measured {sse:.6g} "
              f"({10 * math.log10(peak2n / max(sse, 1e-300)):.3f} dB), one group smaller {sse_less:.6g}")
        assert sse <= allowed * (1 + ESTIMATE_TOL), (l, sse, allowed)
        assert sse_less > allowed * (1 - ESTIMATE_TOL), (l, sse_less, allowed)


# ---- recipes -----------------------------------------------------------------------------------

def _palette_tiff():
    case = next(c for c in pf.palette_matrix() if c["id"].startswith("p8_le"))
    return pf.build(case)[0]


RECIPES = {
    "default_lossy": (LY, {}, None, None, [30.0, 34.0, 38.0, 42.0, 46.0, 50.0]),
    "default_lossless": (LL, {}, None, None, [30.0, 34.0, 38.0, 42.0, 46.0, 0.0]),
    "tlm": (LY, {}, lambda e: e.set_organisation(tlm=1), None, [30.0, 34.0, 38.0, 42.0, 46.0, 50.0]),
    "tparts_LC": (LL, {}, lambda e: e.set_tile_part_divisions("LC"), None, [28.0, 33.0, 38.0, 43.0, 48.0, 0.0]),
    "orientation_6": (LY, {}, lambda e: e.set_source_orientation(6), None, [30.0, 34.0, 38.0, 42.0, 46.0, 50.0]),
    "palette": (LL, {}, None, _palette_tiff, [25.0, 30.0, 35.0, 40.0, 45.0, 0.0]),
}


@pytest.mark.parametrize("name", list(RECIPES))
def test_recipes(name):
    conv, ov, setup, source, targets = RECIPES[name]
    rc = jp2hip.recipe(conv, **ov)
    tif = source() if source else im.tiff_bytes(im.synth_rgb8(300, 530, seed=3))
    e = jp2hip.Encoder(0)
    try:
        if setup:
            setup(e)
        e.set_layer_psnr(targets)
        got, st = e.encode_tiff(tif, conv, rc)
        rep = e.layer_report()
    finally:
        e.close()
    L = rc.layers
    thr = list(rep.threshold[:L])
    print(name, thr, list(rep.bytes[:L]))
    assert st.rate_iterations == 0
    assert all(b <= a for a, b in zip(thr, thr[1:])) and (conv == LY or thr[-1] == 0.0)
    want, _ = by_slopes(tif, conv, rc, thr, setup)
    same(got, want)
    lay, _ = jp2hip.tiff_layout(tif)
    nc, bits = jp2hip.encoded_format(lay)
    assert [s for s, _ in sc.com_lines(bytes(got), L)] == [sc.slope_text(s, bits) for s in thr]


# ---- exclusivity, refusals at the encode, history ------------------------------------------------

def test_exclusive_with_slopes_and_rates_in_every_order(enc):
    setters = dict(psnr=(enc.set_layer_psnr, [30.0, 40.0], "jp2hip_set_layer_psnr"),
                   slopes=(enc.set_layer_slopes, [2.0, 1.0], "jp2hip_set_layer_slopes"),
                   rates=(enc.set_layer_rates, [1.0, 2.0], "jp2hip_set_layer_rates"))
    try:
        for first in setters:
            for second in setters:
                if first == second:
                    continue
                setters[first][0](setters[first][1])
                with pytest.raises(jp2hip.Jp2hipError, match=f"layer {second}: .*{setters[first][2]}"):
                    setters[second][0](setters[second][1])
                setters[second][0](None)          # clearing what is not set is no conflict
                setters[first][0](None)
                setters[second][0](setters[second][1])   # ... and after a clear the other may be set
                setters[second][0](None)
    finally:
        for f, _, _ in setters.values():
            f(None)


@pytest.mark.parametrize("targets,msg", [
    ([float("nan")], r"psnr_db\[0\] is NaN"), ([30.0, float("inf")], r"psnr_db\[1\] is infinite"),
    ([30.0, -2.0], r"psnr_db\[1\] = -2.* is negative"), ([30.0, 40.0, 35.0], r"psnr_db\[2\] decreases"),
    ([30.0] * 33, r"n = 33 is outside")])
def test_the_setter_refuses_and_keeps_what_was_set(enc, targets, msg):
    """The setter's own refusals (not the check's), on a context: the targets
    set before stay set -- the next encode is still driven by them."""
    c = pq.by_name("layers1_texture_p1")
    conv, rc = recipe_of(c)
    ps, K = psnr_for(c)
    enc.set_layer_psnr(ps)
    try:
        with pytest.raises(jp2hip.Jp2hipError, match=msg):
            enc.set_layer_psnr(targets)
        _, st = enc.encode_tiff(tiff_of(c), conv, rc)
        assert keys_of(enc.layer_report(), rc.layers) == K and st.rate_iterations == 0
    finally:
        enc.set_layer_psnr(None)


def test_refused_at_the_encode_and_the_context_stays_usable():
    c = pq.by_name("tie60_p128")
    conv, rc = recipe_of(c)
    ps, K = psnr_for(c)
    e = jp2hip.Encoder(0)
    try:
        e.set_layer_psnr(ps[:3])
        with pytest.raises(jp2hip.Jp2hipError, match=r"n = 3 targets .*layers = 5"):
            e.encode_tiff(tiff_of(c), conv, rc)
        e.set_layer_psnr(ps[:4] + [0.0])
        with pytest.raises(jp2hip.Jp2hipError, match=r"psnr_db\[4\] is 0 with rate_bpp > 0"):
            e.encode_tiff(tiff_of(c), conv, rc)
        e.set_layer_psnr(ps)
        with pytest.raises(jp2hip.Jp2hipError, match="last, must be 0"):
            e.encode_tiff(tiff_of(c), LL, jp2hip.recipe(LL, **dict(c["recipe"], rate_bpp=0.0)))
        got, st = e.encode_tiff(tiff_of(c), conv, rc)
        assert keys_of(e.layer_report(), rc.layers) == K
        assert not st.reused & jp2hip._lib.AFTER_FAILURE
    finally:
        e.close()


def test_history_psnr_then_plain_then_rates():
    """One context: PSNR targets, then none, then per-layer rates -- each file
    is a fresh context's, and a lossless recipe's plan is rebuilt exactly when
    the one-group bit of its key changes (rates and targets share it)."""
    c = pq.by_name("lossless_top_p128")
    conv, rc = recipe_of(c)
    ps, K = psnr_for(c)
    tif = tiff_of(c)
    rates = [0.5, 1.5, 0.0]

    def fresh(setup):
        e = jp2hip.Encoder(0)
        try:
            setup(e)
            return bytes(e.encode_tiff(tif, conv, rc)[0])
        finally:
            e.close()

    want = [fresh(lambda e: e.set_layer_psnr(ps)), fresh(lambda e: None), fresh(lambda e: e.set_layer_rates(rates))]
    PLAN = jp2hip._lib.REUSED_PLAN
    e = jp2hip.Encoder(0)
    try:
        e.set_layer_psnr(ps)
        got, st = e.encode_tiff(tif, conv, rc)
        same(got, want[0])
        assert not st.reused & PLAN
        got, st = e.encode_tiff(tif, conv, rc)
        same(got, want[0])
        assert st.reused & PLAN and st.rate_iterations == 0
        e.set_layer_psnr(None)
        got, st = e.encode_tiff(tif, conv, rc)
        same(got, want[1])
        assert not st.reused & PLAN          # the flush stripes are groups again
        e.set_layer_rates(rates)
        got, st = e.encode_tiff(tif, conv, rc)
        same(got, want[2])
        assert not st.reused & PLAN          # one group
        e.set_layer_rates(None)
        e.set_layer_psnr(ps)
        got, st = e.encode_tiff(tif, conv, rc)
        same(got, want[0])
        assert st.reused & PLAN              # one group still: the bit rates and targets share
        assert keys_of(e.layer_report(), rc.layers) == K
    finally:
        e.close()
