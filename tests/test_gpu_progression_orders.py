"""GPU parity in every progression order: libjp2hip's file against the
oracle's RPCL file re-sequenced (tests/progression_cases.py, which
tests/test_progression_orders.py checks against OpenJPEG on the CPU).  Every
assertion is bytes against bytes.  The matrix of orders and geometries, the
marker switches, both tier-2 coders, rate-driven encodes (whose rate loop must
not notice the order), a PLT of more than one segment, every encode route,
one context changing order, and the recipes refused.
"""
import threading

import numpy as np
import pytest

import imaging as im
import jp2hip
import progression_cases as pc
import recipe_axes_cases as rac
import sweep_cases as sc
from jp2hip import split as js

pytestmark = pytest.mark.gpu

LL = jp2hip.LOSSLESS


def same(got, want):
    d = pc.first_difference(bytes(got), want)
    assert d is None, d


_rpcl = {}


def want_file(key, img, conv, ov):
    """The expected file for overrides `ov` of image `img` (`key` names the
    pixels); the oracle's RPCL file is made once per recipe and shared by
    the orders."""
    k = (key, conv, repr(sorted((a, b) for a, b in ov.items() if a != "progression")))
    if k not in _rpcl:
        _rpcl[k] = pc.oracle_rpcl(img, jp2hip.recipe(conv, **ov))
    return pc.resequence(_rpcl[k], ov["progression"])


def encode(encoder, img, conv, ov):
    return encoder.encode_tiff(im.tiff_bytes(img), conv, jp2hip.recipe(conv, **ov))


# ---- the matrix -----------------------------------------------------------------

MATRIX = [(n, o, {}) for n in pc.GEOMETRIES for o in pc.NEW_ORDERS] + \
         [(n, pc.RLCP, dict(tparts_r=1, flush_period=fp)) for n in pc.GEOMETRIES for fp in (0, 128)]


def _mid(n, o, more):
    return f"{n}-{pc.NAMES[o]}" + "".join(f"-{k}{v}" for k, v in more.items())


@pytest.mark.parametrize("name,order,more", MATRIX, ids=[_mid(*m) for m in MATRIX])
def test_lossless_matrix(encoder, name, order, more):
    img = pc.image(name)
    ov = pc.overrides(name, order, **more)
    got, _ = encode(encoder, img, LL, ov)
    same(got, want_file(name, img, LL, ov))
    im.tile_part_walk(got, 1)


# ---- marker switches ------------------------------------------------------------

SWITCH_GEOMETRY = {pc.LRCP: "rgb_t128", pc.RLCP: "gray_rect", pc.PCRL: "rgba_ragged", pc.CPRL: "rgb_300"}


@pytest.mark.parametrize("order", pc.NEW_ORDERS, ids=[pc.NAMES[o] for o in pc.NEW_ORDERS])
@pytest.mark.parametrize("off", ["sop", "eph"])
def test_without_sop_or_eph(encoder, order, off):
    name = SWITCH_GEOMETRY[order]
    img = pc.image(name)
    ov = pc.overrides(name, order, **{off: 0})
    got, _ = encode(encoder, img, LL, ov)
    same(got, want_file(name, img, LL, ov))
    im.tile_part_walk(got, ov.get("sop", 1))


@pytest.mark.parametrize("order", pc.NEW_ORDERS, ids=[pc.NAMES[o] for o in pc.NEW_ORDERS])
def test_without_plt(encoder, order):
    """No PLT, no packet boundaries for the helper: the file is the plt = 1
    file of the same order less its PLT segments.  (No COM markers:
    Kdu-Layer-Info counts the PLT bytes into the layers' sizes.)"""
    name = SWITCH_GEOMETRY[order]
    img = pc.image(name)
    ov = pc.overrides(name, order, comment=0)
    got, _ = encode(encoder, img, LL, dict(ov, plt=0))
    same(got, pc.without_plt(want_file(name, img, LL, ov)))
    assert np.array_equal(im.decode_opj(got, ".j2k").reshape(img.shape), img)


# ---- both tier-2 coders ---------------------------------------------------------

@pytest.mark.parametrize("order", [pc.LRCP, pc.PCRL], ids=["LRCP", "PCRL"])
def test_serial_coder_precincts_of_192_blocks(encoder, order):
    """16 x 16 blocks under 256 x 256 precincts: more than 64 blocks a
    precinct, so k_t2_code + k_apply write the packets and their SOPs."""
    img = sc._content("synth", 300, 420, 1, 8, 7)
    ov = dict(pc.J2K, progression=order, tparts_r=0, tile_w=256, tile_h=256, cblk_w_log2=4, cblk_h_log2=4)
    got, _ = encode(encoder, img, LL, ov)
    same(got, want_file("gray_cb16", img, LL, ov))
    im.tile_part_walk(got, 1)


# ---- rate-driven ----------------------------------------------------------------

@pytest.fixture(scope="module")
def lossy_image():
    return im.synth_rgb8(300, 530, seed=3)


@pytest.mark.parametrize("rate", [3.0, 0.5])
def test_lossy_file_and_rate_loop_do_not_depend_on_the_order(encoder, lossy_image, rate):
    base = dict(pc.J2K, tparts_r=0, rate_bpp=rate, slope_skip=1)
    _, st2 = encode(encoder, lossy_image, jp2hip.LOSSY, dict(base, progression=pc.RPCL))
    for order in pc.NEW_ORDERS:
        ov = dict(base, progression=order)
        got, st = encode(encoder, lossy_image, jp2hip.LOSSY, ov)
        same(got, want_file("lossy", lossy_image, jp2hip.LOSSY, ov))
        assert st.rate_iterations == st2.rate_iterations, pc.NAMES[order]


# ---- a PLT of two segments ------------------------------------------------------

def test_two_plt_segments_in_lrcp(encoder):
    case = next(c for c in rac.cases() if c["axis"] == "plt" and c["name"] == "2seg")
    img = rac.image(case)
    ov = dict(case["recipe"], progression=pc.LRCP, tparts_r=0)
    got, _ = encode(encoder, img, LL, ov)
    same(got, want_file("2seg", img, LL, ov))
    walk = im.tile_part_walk(got, 1)
    assert [tp[3] for tp in walk] == [2]


# ---- routes ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def tall():
    """900 rows, flush_period 0: two flush stripes, so two ranks have work."""
    img = im.synth_rgb8(900, 180, seed=11)
    return img, im.tiff_bytes(img, rows_per_strip=48)


def _tall_recipe(order):
    return dict(pc.J2K, progression=order, tparts_r=0, flush_period=0)


@pytest.mark.parametrize("order", [pc.LRCP, pc.PCRL], ids=["LRCP", "PCRL"])
def test_encode_file_single_gpu_and_split(tmp_path, tall, order):
    img, tif = tall
    ov = _tall_recipe(order)
    rc = jp2hip.recipe(LL, **ov)
    want = want_file("tall", img, LL, ov)
    src = tmp_path / "m.tif"
    src.write_bytes(tif)
    single, split = jp2hip.Encoder(0), jp2hip.Encoder(0)
    try:
        split.split_peers([0])
        a, b = tmp_path / "single.j2k", tmp_path / "split.j2k"
        single.encode_file(str(src), str(a), LL, rc)
        split.encode_file(str(src), str(b), LL, rc)
        same(a.read_bytes(), want)
        same(b.read_bytes(), want)
    finally:
        single.close()
        split.close()


@pytest.mark.parametrize("order", [pc.LRCP, pc.PCRL], ids=["LRCP", "PCRL"])
def test_encode_device_split_world_2(tall, order):
    from devmem import DeviceBytes
    img, tif = tall
    ov = _tall_recipe(order)
    rc = jp2hip.recipe(LL, **ov)
    want = want_file("tall", img, LL, ov)
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
                d = DeviceBytes(buf or b"\0")
                try:
                    parts[r] = enc.encode_device_split(d.ptr, d.nbytes, blay, LL, g.member(r).split(), rc)
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
    same(parts[0][0] + parts[1][0], want)


def test_batch_queue_with_a_recipe_in_cprl(tmp_path):
    from jp2hip import batch as jb
    name = "rgb_t128"
    img = pc.image(name)
    ov = pc.overrides(name, pc.CPRL)
    src = tmp_path / "t.tif"
    src.write_bytes(im.tiff_bytes(img))
    with jb.BatchQueue(contexts=1, delete_after_upload=False) as q:
        q.submit(1, "ark:/x/cprl", src, tmp_path / "batch.j2k", LL, jp2hip.recipe(LL, **ov))
        res = q.drain()
    assert res[0]["status"] == jb.OK, res[0]["message"]
    same((tmp_path / "batch.j2k").read_bytes(), want_file(name, img, LL, ov))


# ---- one context, changing order ------------------------------------------------

def test_one_context_changing_only_the_order():
    """The cached plan and tier-2 tables follow a change of `progression`
    alone (PlanCache compares the whole recipe)."""
    name = "rgb_t128"
    img = pc.image(name)
    enc = jp2hip.Encoder(0)
    try:
        for order in (pc.RPCL, pc.LRCP, pc.RPCL, pc.CPRL):
            ov = pc.overrides(name, order)
            got, _ = encode(enc, img, LL, ov)
            same(got, want_file(name, img, LL, ov))
    finally:
        enc.close()


# ---- refusals -------------------------------------------------------------------

@pytest.mark.parametrize("field,ov", [("progression", dict(progression=7, tparts_r=0)),
                                      ("tparts_r.*LRCP", dict(progression=pc.LRCP, tparts_r=1))],
                         ids=["order7", "LRCP_tparts_r"])
def test_refused_and_the_context_survives(encoder, field, ov):
    name = "gray_rect"
    img = pc.image(name)
    tif = im.tiff_bytes(img)
    with pytest.raises(jp2hip.Jp2hipError, match=field):
        encoder.encode_tiff(tif, LL, jp2hip.recipe(LL, **dict(pc.overrides(name, pc.RPCL), **ov)))
    good = pc.overrides(name, pc.RLCP)
    got, _ = encode(encoder, img, LL, good)
    same(got, want_file(name, img, LL, good))
