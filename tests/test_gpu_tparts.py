"""Tile-part divisions L and C (ORGtparts, jp2hip_set_tile_part_divisions) on
the GPU: every file is compared byte for byte with the model of
tests/tparts_cases.py (the oracle's file with its tile-parts cut anew, which
tests/test_tparts.py reads back and decodes on the CPU; a rate-driven case:
the oracle's file at the target lowered by the added headers' bytes), never
with another GPU encode.  The order x letters matrix, TLM, R and L combined
over two flush stripes, rate-driven encodes, PLTs of several segments, the
untiled recipe, one context cycling the letters, and every encode route.
No test touches the session's shared encoder's divisions.
"""
import threading

import numpy as np
import pytest

import imaging as im
import jp2hip
import progression_cases as pc
import recipe_axes_cases as rac
import tlm_cases as tc
import tparts_cases as tp
from jp2hip import split as js

pytestmark = pytest.mark.gpu

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY
REUSED_PLAN, REUSED_T2 = jp2hip._lib.REUSED_PLAN, jp2hip._lib.REUSED_T2_TABLES


def same(got, want):
    d = pc.first_difference(bytes(got), want)
    assert d is None, d


@pytest.fixture(scope="module")
def enc():
    """A context of this module's own; every test sets the letters it needs."""
    e = jp2hip.Encoder(0)
    yield e
    e.close()


_want = {}


def want_file(key, img, rc, letters, tlm=0):
    """The expected file, made once per case."""
    if key not in _want:
        _want[key] = tp.expected(img, rc, letters, tlm)
    return _want[key]


def encode(e, img, conv, rc, letters, tlm=0):
    e.set_tile_part_divisions(letters)
    e.set_organisation(tlm=tlm)
    return e.encode_tiff(im.tiff_bytes(img), conv, rc)


def lrcp(rc):
    rc.progression, rc.tparts_r = pc.LRCP, 0
    return rc


# ---- the order x letters matrix, lossless, J2K with COMs -----------------------------

ORDERS = [(o, 0) for o in range(5)] + [(pc.RLCP, 1), (pc.RPCL, 1)]


@pytest.mark.parametrize("order,tparts_r", ORDERS, ids=[f"{pc.NAMES[o]}-tparts{r}" for o, r in ORDERS])
@pytest.mark.parametrize("name", list(pc.GEOMETRIES))
def test_order_by_letters(enc, name, order, tparts_r):
    """L, C and LC by name and by bits; a combination that gives a tile more
    than 255 tile-parts is refused by the encode as jp2hip.tile_parts refuses it."""
    img = pc.image(name)
    h, w, nc, _ = pc.GEOMETRIES[name]
    rc = jp2hip.recipe(LL, **pc.overrides(name, order, tparts_r=tparts_r))
    for word, letters in tp.LETTERS.items():
        counts = tp.part_counts(w, h, nc, rc, letters)
        if max(counts) > tp.MAX_PARTS:
            t = next(i for i, n in enumerate(counts) if n > tp.MAX_PARTS)
            with pytest.raises(jp2hip.Jp2hipError, match=f"tile {t}: {counts[t]} tile-parts"):
                encode(enc, img, LL, rc, word)
            continue
        got, st = encode(enc, img, LL, rc, word if order % 2 else letters)
        want = want_file((name, order, tparts_r, letters), img, rc, letters)
        same(got, want)
        assert st.out_bytes == len(want)
        assert len(tp.walk(got)) == sum(counts)


def test_without_plt(enc):
    img = pc.image("rgb_t128")
    rc = jp2hip.recipe(LL, **pc.overrides("rgb_t128", pc.LRCP, plt=0))
    got, _ = encode(enc, img, LL, rc, "LC")
    same(got, want_file("noplt", img, rc, tp.L | tp.C))
    assert all(p[3] == 0 for p in im.tile_part_walk(got, 1))


def test_jpx_with_tlm_lists_the_divided_tile_parts(enc):
    img = pc.image("rgb_t128")
    rc = jp2hip.recipe(LL, **pc.overrides("rgb_t128", pc.LRCP, format=2))
    got, st = encode(enc, img, LL, rc, "L", tlm=1)
    want = want_file("jpx_tlm", img, rc, tp.L, 1)
    same(got, want)
    entries = tc.parse(got)
    assert len(entries) == 18 and [t for t, _ in entries] == [t for t, _, _ in tp.walk(got)]
    assert st.out_bytes == len(want)


def test_r_and_l_combined_across_two_stripes(enc):
    """RLCP + tparts_r + L on 700 x 1100: 7 x 6 tile-parts a tile, the four
    tiles of the first stripe interleaved part by part, then the last two."""
    img = tc.lossless_image()
    rc = jp2hip.recipe(LL, progression=pc.RLCP, tparts_r=1)
    got, _ = encode(enc, img, LL, rc, "L")
    same(got, want_file("ll_rl", img, rc, tp.L))
    parts = [(t, k) for t, k, _ in tp.walk(got)]
    assert parts == [(t, k) for k in range(42) for t in range(4)] + [(t, k) for k in range(42) for t in (4, 5)]


def test_lrcp_l_default_recipe_is_quality_progressive_across_tiles(enc):
    img = tc.lossless_image()
    rc = lrcp(jp2hip.recipe(LL))
    got, _ = encode(enc, img, LL, rc, "L")
    same(got, want_file("ll_lrcp", img, rc, tp.L))
    assert np.array_equal(im.decode_pillow(got), img)


# ---- rate-driven ---------------------------------------------------------------------

def test_rate_driven_default_lossy_recipe(enc):
    img = im.synth_rgb8(420, 300, seed=20261021)
    rc = lrcp(jp2hip.recipe(LY))
    got, st = encode(enc, img, LY, rc, "L")
    want = want_file("ly_small", img, rc, tp.L)
    same(got, want)
    assert st.out_bytes == len(want) and len(tp.walk(got)) == 6


@pytest.mark.parametrize("tlm", [0, 1])
def test_rate_driven_counts_e_against_the_target(enc, tlm):
    """700 x 1100: the packets are the oracle's at target - E (- T), which
    differ from those at the target (test_tparts.py)."""
    img = tc.lossless_image()
    rc = lrcp(jp2hip.recipe(LY))
    got, st = encode(enc, img, LY, rc, "L", tlm=tlm)
    want = want_file(("ly", tlm), img, rc, tp.L, tlm)
    same(got, want)
    assert st.out_bytes == len(want)
    assert len(im.codestream(got)) <= tc.rate_target(rc.rate_bpp, 700, 1100)


def test_rate_driven_two_iterations(enc):
    img, rc = tc.two_iteration_case()
    lrcp(rc)
    got, st = encode(enc, img, LY, rc, "L")
    same(got, want_file("ly2", img, rc, tp.L))
    assert st.rate_iterations == tc.TWO_ITERATION_COUNT
    _, off = encode(enc, img, LY, rc, 0)
    assert off.rate_iterations == st.rate_iterations


def test_rate_driven_over_the_target_floors_at_zero(enc):
    img, rc = tc.over_target_case()
    lrcp(rc)
    got, st = encode(enc, img, LY, rc, "L")
    same(got, want_file("over", img, rc, tp.L))
    assert st.rate_iterations == 8
    rc.rate_bpp = 0.001  # a target below E
    got, _ = encode(enc, img, LY, rc, "L")
    same(got, want_file("floor", img, rc, tp.L))


# ---- PLTs of several segments, the untiled recipe ------------------------------------

@pytest.mark.parametrize("order,tparts_r", [(pc.RLCP, 1), (pc.LRCP, 0)])
def test_multi_segment_plt_geometry(enc, order, tparts_r):
    """recipe_axes_cases' two-segment geometry (73 728 packets in one tile, 32
    layers): L cuts its long tile-part into parts of one PLT segment each."""
    case = next(c for c in rac.cases() if c["axis"] == "plt" and c["name"] == "2seg")
    img = rac.image(case)
    rc = jp2hip.recipe(LL, **dict(case["recipe"], progression=order, tparts_r=tparts_r))
    got, _ = encode(enc, img, LL, rc, "L")
    same(got, want_file(("2seg", order), img, rc, tp.L))
    walk = im.tile_part_walk(got, 1)
    assert len(walk) == (7 * 32 if tparts_r else 32) and all(p[3] == 1 for p in walk)
    # the undivided file's long tile-part did take two segments
    enc.set_tile_part_divisions(0)
    off, _ = enc.encode_tiff(im.tiff_bytes(img), LL, rc)
    assert max(p[3] for p in im.tile_part_walk(off, 1)) == 2


def test_untiled_recipe(enc):
    img, rc = tc.untiled_case()
    lrcp(rc)
    got, _ = encode(enc, img, LL, rc, "L")
    same(got, want_file("untiled", img, rc, tp.L))
    assert [(t, k) for t, k, _ in tp.walk(got)] == [(0, k) for k in range(6)]


# ---- one context cycling the letters -------------------------------------------------

def test_one_context_cycling_letters():
    """L, LC, 0, C on one geometry: each file the expected one, the 0 file the
    plain oracle file; the plan is kept, the tier-2 tables are rebuilt at every
    change and kept when nothing changes; the host waits do not move."""
    name = "rgb_t128"
    img = pc.image(name)
    tif = im.tiff_bytes(img)
    rc = jp2hip.recipe(LL, **pc.overrides(name, pc.LRCP))
    plain = pc.expected(img, rc)
    e = jp2hip.Encoder(0)
    try:
        e.encode_tiff(tif, LL, rc)  # warm: buffers, plan
        waits = []
        for i, word in enumerate(("L", "LC", 0, "C", "C")):
            e.set_tile_part_divisions(word)
            got, st = e.encode_tiff(tif, LL, rc)
            letters = jp2hip._lib.tparts_letters(word)
            same(got, want_file((name, pc.LRCP, 0, letters), img, rc, letters) if letters else plain)
            assert st.reused & REUSED_PLAN, (word, st.reused)
            assert bool(st.reused & REUSED_T2) == (i == 4), (word, st.reused)
            waits.append(st.host_waits)
        assert len(set(waits)) == 1, waits
    finally:
        e.close()


def test_host_waits_are_equal_with_and_without_letters_rate_driven():
    img = tc.lossless_image()
    tif = im.tiff_bytes(img)
    rc = lrcp(jp2hip.recipe(LY))
    e = jp2hip.Encoder(0)
    try:
        e.encode_tiff(tif, LY, rc)  # warm: buffers, plan, pool
        waits = {}
        for word in (0, "L", 0, "L"):
            e.set_tile_part_divisions(word)
            _, st = e.encode_tiff(tif, LY, rc)
            waits.setdefault(word, []).append(st.host_waits)
        assert waits[0] == waits["L"], waits
    finally:
        e.close()


def test_refused_letters_change_nothing():
    img = pc.image("rgb_t128")
    rc = jp2hip.recipe(LL, **pc.overrides("rgb_t128", pc.LRCP))
    e = jp2hip.Encoder(0)
    try:
        e.set_tile_part_divisions("L")
        with pytest.raises(jp2hip.Jp2hipError, match="tparts_r"):
            e.set_tile_part_divisions(3)
        with pytest.raises(jp2hip.Jp2hipError, match="neither"):
            e.set_tile_part_divisions(8)
        got, _ = e.encode_tiff(im.tiff_bytes(img), LL, rc)  # still the letters set before
        same(got, want_file(("rgb_t128", pc.LRCP, 0, tp.L), img, rc, tp.L))
        # an encode whose letters give a tile more than 255 tile-parts is refused (RPCL + L with
        # 16 x 16 precincts: a part per packet), and the context encodes on
        big = jp2hip.recipe(LL, **pc.overrides("rgb_t128", pc.RPCL, nprecincts=1, prec_w_log2=[4], prec_h_log2=[4]))
        n = tp.part_counts(200, 300, 3, big, tp.L)[0]
        assert n > 255
        with pytest.raises(jp2hip.Jp2hipError, match=f"tile 0: {n} tile-parts with ORGtparts=L"):
            e.encode_tiff(im.tiff_bytes(img), LL, big)
        got, _ = e.encode_tiff(im.tiff_bytes(img), LL, rc)
        same(got, want_file(("rgb_t128", pc.LRCP, 0, tp.L), img, rc, tp.L))
    finally:
        e.close()


# ---- routes --------------------------------------------------------------------------

ROUTE_CASES = {"lossless": (LL, 0), "lossless_tlm": (LL, 1), "lossy": (LY, 0), "lossy_tlm": (LY, 1)}


@pytest.fixture(scope="module", params=list(ROUTE_CASES))
def route_case(request):
    """(conversion, recipe, tlm, TIFF bytes, expected file): LRCP + L on the
    700 x 1100 image (two flush stripes), lossless and rate-driven, with and
    without TLM."""
    conv, tlm = ROUTE_CASES[request.param]
    img = tc.lossless_image()
    rc = lrcp(jp2hip.recipe(conv))
    key = "ll_lrcp" if (conv, tlm) == (LL, 0) else (("ly", tlm) if conv == LY else "ll_lrcp_tlm")
    return conv, rc, tlm, im.tiff_bytes(img, rows_per_strip=48), want_file(key, img, rc, tp.L, tlm)


def test_route_encode_tiff_and_device(enc, route_case):
    from devmem import DeviceBytes
    conv, rc, tlm, tif, want = route_case
    enc.set_tile_part_divisions("L")
    enc.set_organisation(tlm=tlm)
    got, _ = enc.encode_tiff(tif, conv, rc)
    same(got, want)
    lay, offs = jp2hip.tiff_layout(tif)
    d = DeviceBytes(tif)
    try:
        got, st = enc.encode_device(d.ptr, d.nbytes, lay, conv, rc)
    finally:
        d.free()
    same(got, want)
    assert st.out_bytes == len(want)


def test_route_encode_file_single_gpu_and_split_peers(tmp_path, route_case):
    conv, rc, tlm, tif, want = route_case
    src = tmp_path / "m.tif"
    src.write_bytes(tif)
    single, split, late = jp2hip.Encoder(0), jp2hip.Encoder(0), jp2hip.Encoder(0)
    try:
        split.split_peers([0])
        for e in (single, split, late):   # (split: reaches the peer it has)
            e.set_tile_part_divisions("L")
            e.set_organisation(tlm=tlm)
        late.split_peers([0])             # a peer added later inherits them
        for name, e in (("single", single), ("split", split), ("late", late)):
            out = tmp_path / f"{name}.jpx"
            st = e.encode_file(str(src), str(out), conv, rc)
            same(out.read_bytes(), want)
            assert st.out_bytes == len(want), name
    finally:
        single.close()
        split.close()
        late.close()


@pytest.mark.parametrize("world", [2, 3])
def test_route_encode_device_split_over_thread_ranks(route_case, world):
    """Every rank holds only its band's strips; with three ranks over the two
    flush stripes rank 0's band is empty.  Parts, offsets and file_len against
    the expected file."""
    from devmem import DeviceBytes
    conv, rc, tlm, tif, want = route_case
    lay, offs = jp2hip.tiff_layout(tif)
    g = js.ThreadGroup(world)
    parts, errs = [None] * world, []

    def work(r):
        try:
            e = jp2hip.Encoder(0)
            try:
                e.set_tile_part_divisions("L")
                e.set_organisation(tlm=tlm)
                r0, r1 = js.split_rows(lay.height, rc.tile_h, r, world, rc.flush_period)
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
        assert file_offset == off and file_len == len(want)
        assert st.out_bytes == len(want)
        off += len(part)
    same(b"".join(p[0] for p in parts), want)


def test_route_batch_queue(tmp_path, route_case):
    from jp2hip import batch as jb
    conv, rc, tlm, tif, want = route_case
    src = tmp_path / "t.tif"
    src.write_bytes(tif)
    with jb.BatchQueue(contexts=1, delete_after_upload=False, tlm=bool(tlm)) as q:
        with pytest.raises(jp2hip.Jp2hipError, match="tparts_r"):  # refused letters, before a submit too
            q.set_tile_part_divisions(1)
        q.set_tile_part_divisions("L")
        q.submit(1, "ark:/x/tparts", src, tmp_path / "batch.jpx", conv, rc)
        with pytest.raises(jp2hip.Jp2hipError):  # only before the first submit
            q.set_tile_part_divisions(0)
        res = q.drain()
    assert res[0]["status"] == jb.OK, res[0]["message"]
    assert res[0]["out_bytes"] == len(want)
    same((tmp_path / "batch.jpx").read_bytes(), want)
