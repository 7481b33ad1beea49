"""Tile-part divisions L and C (ORGtparts, jp2hip_set_tile_part_divisions)
without a GPU: jp2hip_tile_parts against the Python model's runs
(tests/tparts_cases.py), the model's files read back by an independent reader
and decoded by Pillow, the refusals, and the premises the rate-driven GPU
cases of tests/test_gpu_tparts.py rest on, checked against the oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import imaging as im
import jp2hip
import oracle_lib as ol
import progression_cases as pc
import tlm_cases as tc
import tparts_cases as tp
from jp2hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every order with tparts_r where the order allows it
ORDERS = [(o, 0) for o in range(5)] + [(pc.RLCP, 1), (pc.RPCL, 1)]
ORDER_IDS = [f"{pc.NAMES[o]}-tparts{r}" for o, r in ORDERS]


def geometry_recipe(name, order, tparts_r):
    return jp2hip.recipe(jp2hip.LOSSLESS, **pc.overrides(name, order, tparts_r=tparts_r))


# ---- jp2hip_tile_parts against the model ---------------------------------------------

@pytest.mark.parametrize("order,tparts_r", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name", list(pc.GEOMETRIES))
def test_tile_parts_agree_with_the_model(name, order, tparts_r):
    h, w, nc, _ = pc.GEOMETRIES[name]
    rc = geometry_recipe(name, order, tparts_r)
    g = pc.geometry_of_recipe(w, h, nc, rc)
    for letters in (0, tp.L, tp.C, tp.L | tp.C):
        for t in range(pc.ntiles(g)):
            want = tp.runs(g, t, order, letters, tparts_r)
            if len(want) > tp.MAX_PARTS:
                with pytest.raises(jp2hip.Jp2hipError):
                    jp2hip.tile_parts(w, h, nc, 8, rc, letters, t)
                break
            assert jp2hip.tile_parts(w, h, nc, 8, rc, letters, t) == want, (letters, t)


@pytest.mark.parametrize("order,tparts_r", ORDERS, ids=ORDER_IDS)
def test_tile_parts_of_two_flush_stripes(order, tparts_r):
    """tlm_cases.lossless_image's geometry: 2 x 3 tiles of 512 on 700 x 1100,
    whose ragged tiles have fewer precincts (and, cut by C or L inside a
    resolution, other starts) than the full ones."""
    rc = jp2hip.recipe(jp2hip.LOSSLESS, progression=order, tparts_r=tparts_r)
    g = pc.geometry_of_recipe(700, 1100, 3, rc)
    counts = {}
    for letters in (tp.L, tp.C, tp.L | tp.C):
        for t in range(6):
            want = tp.runs(g, t, order, letters, tparts_r)
            counts[letters, t] = len(want)
            if len(want) <= tp.MAX_PARTS:
                assert jp2hip.tile_parts(700, 1100, 3, 8, rc, letters, t) == want, (letters, t)
    if order == pc.RPCL:  # a part per precinct and component: the ragged tiles have fewer
        assert len({counts[tp.C, t] for t in range(6)}) > 1


def test_letter_strings_and_ints_are_the_same_setting():
    rc = geometry_recipe("rgb_t128", pc.LRCP, 0)
    for s, bits in (("L", 2), ("C", 4), ("LC", 6), ("cl", 6), ("", 0)):
        assert _lib.tparts_letters(s) == bits
        assert jp2hip.tile_parts(200, 300, 3, 8, rc, s, 0) == jp2hip.tile_parts(200, 300, 3, 8, rc, bits, 0)
    with pytest.raises(ValueError):
        _lib.tparts_letters("LX")


def test_count_without_a_buffer_and_with_a_short_one():
    rc = geometry_recipe("rgb_t128", pc.LRCP, 0)
    want = jp2hip.tile_parts(200, 300, 3, 8, rc, tp.L, 0)
    assert len(want) == 3 and want[0] == 0
    Lb = _lib.lib()
    assert Lb.jp2hip_tile_parts(200, 300, 3, 8, ctypes.byref(rc), tp.L, 0, None, 0) == 3
    buf = (ctypes.c_uint32 * 3)(7, 7, 7)
    assert Lb.jp2hip_tile_parts(200, 300, 3, 8, ctypes.byref(rc), tp.L, 0, buf, 2) == 3
    assert list(buf) == want[:2] + [7]


def test_tables_and_counts_under_sanitizers(tmp_path):
    """The host side in a stand-alone program built with AddressSanitizer /
    UBSan (tests/host/test_tparts_tables.cpp): every tile-part of the tier-2
    tables is a run of its tile's sequence, the runs tile each tile's packets
    in order, and the counts and the file order agree with the tables, whole
    images and split bands.  (Most of the test's time is the compile.)"""
    csrc = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc")
    exe = tmp_path / "test_tparts_tables"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-Wall",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "test_tparts_tables.cpp"),
                    os.path.join(csrc, "t2.cpp"), os.path.join(csrc, "plan.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert r.stdout.startswith("TPARTS TABLES OK")


# ---- the model's files ---------------------------------------------------------------

MODEL_CASES = [("rgb_t128", pc.LRCP, 0, tp.L), ("rgb_t128", pc.CPRL, 0, tp.C), ("rgba_ragged", pc.RLCP, 1, tp.L | tp.C),
               ("gray_rect", pc.RLCP, 1, tp.L), ("rgb_300", pc.LRCP, 0, tp.L | tp.C), ("rgba_ragged", pc.PCRL, 0, tp.C)]


@pytest.mark.parametrize("name,order,tparts_r,letters", MODEL_CASES,
                         ids=[f"{n}-{pc.NAMES[o]}-r{r}-{l}" for n, o, r, l in MODEL_CASES])
def test_modelled_file_reads_and_decodes_like_the_undivided(name, order, tparts_r, letters):
    """The independent reader: Psot from the first SOT reaches EOC with
    consistent TPsot / TNsot, every tile-part's PLT covers its packets with
    Nsop counting on through the tile's parts (imaging.tile_part_walk), and
    Pillow decodes the pixels of the undivided file."""
    img = pc.image(name)
    rc = geometry_recipe(name, order, tparts_r)
    base = pc.expected(img, rc)
    want = tp.expected(img, rc, letters)
    parts = tp.walk(want)
    h, w, nc, _ = pc.GEOMETRIES[name]
    counts = tp.part_counts(w, h, nc, rc, letters)
    assert len(parts) == sum(counts) > len(tp.walk(base))
    assert [sum(1 for t, _, _ in parts if t == u) for u in range(len(counts))] == counts
    im.tile_part_walk(want, 1)
    assert len(want) - len(base) == tp.division_bytes(w, h, nc, rc, letters)
    a, b = im.decode_pillow(want), im.decode_pillow(base)
    assert np.array_equal(a, b) and np.array_equal(a.reshape(img.shape), img)


def test_modelled_file_order_interleaves_the_tiles_of_a_stripe():
    """LRCP + L on 700 x 1100 with the default recipe: per flush stripe layer 0
    of every tile, then layer 1, ... -- any prefix holds whole layers of the stripe."""
    img = tc.lossless_image()
    rc = jp2hip.recipe(jp2hip.LOSSLESS, progression=pc.LRCP, tparts_r=0)
    want = tp.expected(img, rc, tp.L)
    tiles = [(t, k) for t, k, _ in tp.walk(want)]
    assert tiles == [(t, k) for k in range(6) for t in range(4)] + [(t, k) for k in range(6) for t in (4, 5)]
    assert np.array_equal(im.decode_pillow(want), img)


def test_modelled_tlm_lists_the_divided_tile_parts():
    img = pc.image("rgb_t128")
    rc = jp2hip.recipe(jp2hip.LOSSLESS, **pc.overrides("rgb_t128", pc.LRCP, format=2))
    want = tp.expected(img, rc, tp.L, tlm=1)
    entries = tc.parse(want)
    assert [t for t, _ in entries] == [t for t, _, _ in tp.walk(want)] and len(entries) == 6 * 3
    assert np.array_equal(im.decode_pillow(want), img)


@pytest.mark.parametrize("letters,over", [(tp.L, dict(layers=1)), (tp.C, dict())])
def test_letters_that_cut_nowhere_give_the_input_file(letters, over):
    """L with one layer; C with one component."""
    name = "gray_rect"
    img = pc.image(name)
    for order, tparts_r in ((pc.LRCP, 0), (pc.RLCP, 1), (pc.CPRL, 0)):
        rc = jp2hip.recipe(jp2hip.LOSSLESS, **pc.overrides(name, order, tparts_r=tparts_r, **over))
        assert tp.expected(img, rc, letters) == pc.expected(img, rc)
        h, w, nc, _ = pc.GEOMETRIES[name]
        assert tp.division_bytes(w, h, nc, rc, letters) == 0
        for t in range(6):
            assert jp2hip.tile_parts(w, h, nc, 8, rc, letters, t) == jp2hip.tile_parts(w, h, nc, 8, rc, 0, t)


# ---- refusals ------------------------------------------------------------------------

def test_more_than_255_tile_parts_are_refused_naming_tile_and_count():
    """RPCL + L: layers are innermost, so every packet starts a tile-part --
    with 64 x 64 precincts a 512 x 512 tile of the default recipe has far
    more than 255 packets."""
    rc = jp2hip.recipe(jp2hip.LOSSLESS, progression=pc.RPCL, nprecincts=1, prec_w_log2=[6], prec_h_log2=[6])
    g = pc.geometry_of_recipe(700, 1100, 3, rc)
    n = len(tp.runs(g, 0, pc.RPCL, tp.L, 1))
    assert n > 255
    with pytest.raises(jp2hip.Jp2hipError) as e:
        jp2hip.tile_parts(700, 1100, 3, 8, rc, tp.L, 5)  # (asked for tile 5: tile 0 is the first that does not fit)
    assert "tile 0" in str(e.value) and str(n) in str(e.value) and "RL" in str(e.value) and "255" in str(e.value)
    # exactly 255 fits, 256 does not (RPCL + L: a tile-part per packet; one precinct a resolution)
    rc = jp2hip.recipe(jp2hip.LOSSLESS, progression=pc.RPCL, tparts_r=0, levels=4, layers=17, tile_w=64, tile_h=64,
                       nprecincts=1, prec_w_log2=[15], prec_h_log2=[15])
    assert len(jp2hip.tile_parts(64, 64, 3, 8, rc, tp.L, 0)) == 255 == 5 * 3 * 17
    with pytest.raises(jp2hip.Jp2hipError, match="256 tile-parts"):
        jp2hip.tile_parts(64, 64, 4, 8, jp2hip.recipe(jp2hip.LOSSLESS, progression=pc.RPCL, tparts_r=0, levels=3,
                                                      layers=16, tile_w=64, tile_h=64, nprecincts=1,
                                                      prec_w_log2=[15], prec_h_log2=[15]), tp.L, 0)


def test_the_r_bit_is_refused_pointing_at_the_recipe():
    rc = geometry_recipe("rgb_t128", pc.RLCP, 0)
    for call in (lambda: jp2hip.tile_parts(200, 300, 3, 8, rc, 1 | tp.L, 0),
                 lambda: jp2hip.tile_parts(200, 300, 3, 8, rc, "RL", 0)):
        with pytest.raises(jp2hip.Jp2hipError, match="tparts_r"):
            call()
    # the setter checks the letters before it looks at the context: the refusal shows without a GPU
    assert _lib.lib().jp2hip_set_tile_part_divisions(None, 3) < 0
    assert "tparts_r" in _lib.last_error() and "context" not in _lib.last_error()


@pytest.mark.parametrize("letters", [8, 6 | 16, -2, 1 << 30])
def test_an_unknown_bit_is_refused(letters):
    rc = geometry_recipe("rgb_t128", pc.LRCP, 0)
    with pytest.raises(jp2hip.Jp2hipError, match="neither"):
        jp2hip.tile_parts(200, 300, 3, 8, rc, letters, 0)
    assert _lib.lib().jp2hip_set_tile_part_divisions(None, letters) < 0
    assert str(letters) in _lib.last_error() and "context" not in _lib.last_error()


def test_setters_refuse_a_null_context_and_a_null_queue():
    """(The queue's setter after a submit needs a queue, so a GPU:
    test_gpu_tparts.py test_route_batch_queue.)"""
    from jp2hip import batch as jb
    for letters in (0, tp.L, tp.L | tp.C):
        assert _lib.lib().jp2hip_set_tile_part_divisions(None, letters) < 0
        assert "context" in _lib.last_error()
    assert jb._bind().jp2hip_batch_set_tile_part_divisions(None, tp.L) < 0


def test_what_the_encodes_refuse_is_refused_here():
    with pytest.raises(jp2hip.Jp2hipError, match="tparts_r"):  # R with LRCP: as ever
        jp2hip.tile_parts(200, 300, 3, 8, geometry_recipe("rgb_t128", pc.LRCP, 1), tp.L, 0)
    with pytest.raises(jp2hip.Jp2hipError, match="tile index"):
        jp2hip.tile_parts(200, 300, 3, 8, geometry_recipe("rgb_t128", pc.LRCP, 0), tp.L, 6)


def test_python_mirror_lists_the_new_symbols():
    from jp2hip import batch as jb
    for sym in ("jp2hip_set_tile_part_divisions", "jp2hip_batch_set_tile_part_divisions", "jp2hip_tile_parts"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)
    assert "jp2hip_batch_set_tile_part_divisions" in jb.BATCH_EXPORTS
    assert (_lib.TPARTS_L, _lib.TPARTS_C) == (2, 4)
    txt = open(os.path.join(ROOT, "include", "jp2hip.h")).read()
    assert "#define JP2HIP_TPARTS_L 2" in txt and "#define JP2HIP_TPARTS_C 4" in txt
    assert "13 106" in txt  # the bound of the rate rule's exactness is stated


# ---- E, and the premises of the rate-driven GPU cases --------------------------------

def lrcp(rc):
    rc.progression, rc.tparts_r = pc.LRCP, 0
    return rc


def test_e_is_as_defined():
    # LRCP + L, six layers: five more tile-parts a tile, each SOT + SOD + a PLT header
    rc = lrcp(jp2hip.recipe(jp2hip.LOSSY))
    assert tp.part_counts(300, 420, 3, rc, tp.L) == [6] and tp.part_counts(300, 420, 3, rc, 0) == [1]
    assert tp.division_bytes(300, 420, 3, rc, tp.L) == 19 * 5
    rc.plt = 0
    assert tp.division_bytes(300, 420, 3, rc, tp.L) == 14 * 5
    # on top of R: RLCP + R + L on 700 x 1100 (6 tiles, 7 resolutions, 6 layers)
    rc = jp2hip.recipe(jp2hip.LOSSY, progression=pc.RLCP)
    assert tp.division_bytes(700, 1100, 3, rc, tp.L) == 19 * (6 * 7 * 6 - 6 * 7)
    # and it is what the model's lossless file grows by
    img = pc.image("rgb_t128")
    rc = geometry_recipe("rgb_t128", pc.LRCP, 0)
    assert len(tp.expected(img, rc, tp.L)) - len(pc.expected(img, rc)) == tp.division_bytes(200, 300, 3, rc, tp.L) == 19 * 2 * 6


def oracle_iterations(img, orc):
    ol.pcrd_export_enable(True)
    try:
        data = ol.encode(img, orc)
        return data, ol.pcrd_export()["iterations"]
    finally:
        ol.pcrd_export_enable(False)


def test_premise_two_iterations_at_target_less_e():
    """tlm_cases.two_iteration_case with LRCP + L: the oracle at target - E
    (E = 95) iterates as often as the case documents."""
    img, rc = tc.two_iteration_case()
    lrcp(rc)
    E = tp.division_bytes(300, 420, 3, rc, tp.L)
    assert E == 95
    orc = ol.copy_recipe(rc)
    orc.progression = pc.RPCL
    orc.rate_bpp = tc.lower_rate(rc.rate_bpp, 300, 420, E)
    assert tc.rate_target(orc.rate_bpp, 300, 420) == tc.rate_target(0.5, 300, 420) - 95
    _, iters = oracle_iterations(img, orc)
    assert iters == tc.TWO_ITERATION_COUNT >= 2
    # and the file with its letters keeps the target it is bounded by
    want = tp.expected(img, rc, tp.L)
    assert len(im.codestream(want)) <= tc.rate_target(0.5, 300, 420)
    assert len(tp.walk(want)) == 6


def test_premise_a_rate_case_where_the_oracle_notices_e():
    """The default lossy recipe with LRCP + L on the 700 x 1100 image (E = 570):
    the oracle at target - E writes other packets than at the target, so an
    encode that did not count E against its target cannot match the model.
    (The 300 x 420 image of the GPU suite codes below its target at 3 bpp: its
    file with letters is the file without them plus E.)"""
    img = tc.lossless_image()
    rc = lrcp(jp2hip.recipe(jp2hip.LOSSY))
    assert tp.division_bytes(700, 1100, 3, rc, tp.L) == 570
    at_target = pc.expected(img, rc)
    want = tp.expected(img, rc, tp.L)
    assert len(want) - len(at_target) != 570
    assert len(im.codestream(want)) <= tc.rate_target(3.0, 700, 1100)
    small = im.synth_rgb8(420, 300, seed=20261021)
    assert len(tp.expected(small, rc, tp.L)) - len(pc.expected(small, rc)) == 95


def test_premise_the_over_target_door_floors_at_zero():
    """tlm_cases.over_target_case with LRCP + L: 35 tiles x 5 added parts; all
    8 iterations at the lowered target, the file stays over the target.  And a
    target below E floors at 0 and stays rate-driven."""
    img, rc = tc.over_target_case()
    lrcp(rc)
    E = tp.division_bytes(300, 420, 3, rc, tp.L)
    assert E == 19 * 5 * 35
    orc = ol.copy_recipe(rc)
    orc.progression = pc.RPCL
    orc.rate_bpp = tc.lower_rate(rc.rate_bpp, 300, 420, E)
    base, iters = oracle_iterations(img, orc)
    assert iters == 8 and len(im.codestream(base)) > tc.rate_target(0.5, 300, 420)
    assert tc.rate_target(tc.lower_rate(0.001, 300, 420, E), 300, 420) == 0 < tc.rate_target(0.001, 300, 420)
