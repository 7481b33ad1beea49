"""The context-history corpus (tests/history_cases.py) on the CPU: its
expected files are real files, no two steps a stale result could be mistaken
for each other, and the walks tests/test_gpu_history.py runs cover what they
are said to cover."""
import itertools

import numpy as np
import pytest

import history_cases as hc
import imaging as im
import jp2hip
import oracle_lib as ol
import pcrd_cases as pc


def _decoder():
    if im.opj("opj_decompress"):
        return "opj"
    try:
        import PIL  # noqa: F401
        return "pillow"
    except ImportError:
        return None


@pytest.mark.parametrize("i", range(hc.N), ids=hc.NAMES)
def test_expected_file_decodes(i):
    """Every expected file decodes; the lossless ones to the step's pixels."""
    dec = _decoder()
    if dec is None:
        pytest.skip("no JPEG 2000 decoder (OpenJPEG or Pillow) available")
    step = hc.STEPS[i]
    want = hc.expected(i)
    px = hc.source(i)[1]
    fmt = hc.recipe(step).format
    if dec == "opj":
        got = im.decode_opj(want, ext=".j2k" if fmt == jp2hip.FORMAT_J2K else ".jpx")
    else:
        got = im.decode_pillow(want)
    assert got.shape == px.shape
    if step.lossless:
        assert np.array_equal(got, px)
    else:
        # a rate-driven file: what matters here is that it is a file (the
        # oracle's rate control has its own tests)
        assert got.dtype == px.dtype


def test_steps_of_one_geometry_expect_different_files():
    """A stale output -- the file of an earlier step of the same (w, h, nc,
    bits) -- can never equal what a step expects."""
    for a, b in itertools.combinations(range(hc.N), 2):
        if hc.geometry(a) == hc.geometry(b):
            assert hc.expected(a) != hc.expected(b), (hc.NAMES[a], hc.NAMES[b])


def test_pair_walks_cover_every_ordered_pair():
    seen = set()
    for a in range(hc.N):
        walk = hc.pair_walk(a)
        assert len(walk) == 2 * hc.N and walk[0] == a
        seen |= hc.pairs_of(walk)
    assert seen == set(itertools.product(range(hc.N), repeat=2))


def test_corpus_has_what_each_piece_of_state_needs():
    """The neighbours the corpus promises: hits on one key over the tiff and
    the device route, both splits on that key, every route, and at least 16
    encode steps on images of at most 256 x 256."""
    assert hc.N >= 16
    base = hc.index("base")
    same = [i for i in range(hc.N) if hc.key(i) == hc.key(base)]
    routes = {hc.STEPS[i].route for i in same}
    assert routes == {"tiff", "device", "split1", "split2"}
    hits = hc.cache_hit_pairs()
    assert any(a != b and hc.STEPS[b].route == "tiff" for a, b in hits)
    assert any(a != b and hc.STEPS[b].route == "device" for a, b in hits)
    # one recipe field away from the base: same geometry, another key
    for name in ("order_cprl", "order_lrcp", "prec64", "layers1", "layers32", "no_sop_eph", "no_plt", "mct0",
                 "tparts_r1", "levels0", "levels5", "lossy_skip1"):
        i = hc.index(name)
        assert hc.geometry(i) == hc.geometry(base) and hc.key(i) != hc.key(base), name
    assert hc.key(hc.index("cblk64x16")) != hc.key(hc.index("cblk16x64"))
    assert hc.key(hc.index("lossy_skip1")) != hc.key(hc.index("lossy_skip0"))
    for i in range(hc.N):
        w, h, _, _ = hc.geometry(i)
        assert w <= 256 and h <= 256
    for names in (hc.AFTER_FAILURE, hc.TRIM_ROWS, hc.BEFORE_FAILURE.values(), [f.of for f in hc.FAILURES if f.of]):
        for name in names:
            assert name in hc.NAMES


def test_rate_driven_steps_take_the_doors_they_are_named_for():
    """The oracle's PCRD census of the two pcrd_cases steps: the prediction's
    safety-net rerun, and a rate loop of at least three iterations."""
    for name, cell in (("pcrd_safety_p1", "rate_safety_net"), ("pcrd_iter3_p128", "rate_iterations_3")):
        step = hc.STEPS[hc.index(name)]
        ol.pcrd_census_reset()
        ol.encode(hc.source(hc.index(name))[1], ol.copy_recipe(hc.recipe(step)))
        assert ol.pcrd_census_read()[cell] > 0, name
    # the serial tier-2 route: one precinct of 256 blocks of 16 x 16
    r = hc.STEPS[hc.index("serial256")].recipe
    assert (r["tile_w"] // pc.B) * (r["tile_h"] // pc.B) == 256 and r["nprecincts"] == 0 and r["levels"] == 0


def test_split_rank_1_has_rows():
    """The two-rank step gives rank 1 tile rows of its own (tile0, block0 != 0)."""
    from jp2hip import split as js
    step = hc.STEPS[hc.index("split_rank1")]
    rc = hc.recipe(step)
    r0, r1 = js.split_rows(hc.H, rc.tile_h, 1, 2, rc.flush_period)
    assert 0 < r0 < r1 == hc.H


def test_failure_sources_parse():
    """The failing sources are TIFFs the parser accepts: they fail in the
    encode, after it has begun, not before it."""
    for f in hc.FAILURES:
        if f.tiff is not None:
            lay, _ = jp2hip.tiff_layout(f.tiff())
            assert lay.width > 0


def test_random_walks_are_fixed_and_mixed():
    for seed in hc.WALK_SEEDS:
        walk = hc.random_walk(seed)
        assert walk == hc.random_walk(seed) and len(walk) == hc.WALK_LENGTH
        kinds = {t[0] for t in walk}
        assert kinds == {"encode", "fail", "trim"}
