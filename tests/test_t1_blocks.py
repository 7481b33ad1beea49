"""The crafted tier-1 corpus (tests/t1_block_cases.py) on the CPU: that its
construction holds (a tile is the block it names), that between them the cases
reach every coding state the oracle's census counts except those the standard
makes unreachable, that the extreme blocks are as extreme as a block can be,
and that an independent decoder reads the oracle's files for them.

Two figures differ from what one might expect of a 64x64 block, and both are
properties of the scan, not of this corpus (proved below, asserted as
equalities):
  * the most decisions a bit-plane can carry is 8*64*16 + 2 = 8194, not ten
    per stripe column: a column codes ten only in run mode, and run mode
    needs the column before it to have stayed insignificant (at most four
    decisions), so only a stripe's first column can add two to eight a column;
  * the longest significance-propagation chain is 220 samples, not thousands:
    a link needs the earlier sample coded before the later one is visited, so
    a chain climbs at most one row per column and cannot turn back within a
    stripe.  t1_block_cases.longest_forward_chain() computes the bound over
    every chain of the grid and chain_stair_fwd attains it.
"""
import numpy as np
import pytest

import imaging as im
import oracle_lib as ol
import t1_block_cases as tc

CASES = tc.cases()
IDS = [c["name"] for c in CASES]
N = tc.N

_FILES = {}


def oracle_file(c):
    """(file, census of the encode), computed once per case."""
    if c["name"] not in _FILES:
        ol.census_reset()
        data = ol.encode(tc.image(c), ol.recipe(c["lossless"], **c["recipe"]))
        _FILES[c["name"]] = (data, ol.census_read())
    return _FILES[c["name"]]


def block_census(block, band=0):
    ol.census_reset()
    out = ol.t1_encode(tc.to_sm(block), band, True)
    return out, ol.census_read()


# ---- preconditions of the construction ------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_image_is_what_the_case_says(case):
    img = tc.image(case)
    r = case["recipe"]
    assert img.ndim == 2 and img.dtype == (np.uint16 if case["bits"] == 16 else np.uint8)
    assert max(img.shape) <= 512
    assert r["format"] == 0 and r["flush_period"] == 0 and r["nprecincts"] == 0 and r["mct"] == 0
    ntx, nty = -(-img.shape[1] // r["tile_w"]), -(-img.shape[0] // r["tile_h"])
    assert len(case["tiles"]) <= ntx * nty < len(case["tiles"]) + ntx   # only padding in the last row
    if r["levels"] == 0:
        assert r["tile_w"] <= N and r["tile_h"] <= N
        for t, (_, w, h) in enumerate(case["tiles"]):
            ty, tx = divmod(t, ntx)
            tile = img[ty * r["tile_h"]:(ty + 1) * r["tile_h"], tx * r["tile_w"]:(tx + 1) * r["tile_w"]]
            assert tile.shape == (h, w), (t, tile.shape)


def test_block_names_are_tile_indices():
    for blocks, bits in ((tc.blocks16(), 16), (tc.blocks8(), 8)):
        img = tc.assemble(blocks, bits).astype(np.int64) - (1 << (bits - 1))
        for t, (name, a) in enumerate(blocks):
            ty, tx = divmod(t, 8)
            assert np.array_equal(img[ty * N:(ty + 1) * N, tx * N:(tx + 1) * N], a), name
            assert np.abs(a.astype(np.int64)).max() <= 1 << (bits - 1)


LEVEL0_A = [c for c in CASES if c["kind"] == "a" and c["recipe"]["levels"] == 0 and c["group"] != "straddle"]


@pytest.mark.parametrize("case", LEVEL0_A, ids=[c["name"] for c in LEVEL0_A])
def test_each_tile_is_one_block_of_the_level_shifted_samples(case):
    """Recipe (a): the body of tile t's only packet is, byte for byte, tier-1
    of the level-shifted tile as an LL block."""
    data, _ = oracle_file(case)
    img = tc.image(case).astype(np.int64) - (1 << (case["bits"] - 1))
    r = case["recipe"]
    ntx = -(-img.shape[1] // r["tile_w"])
    parts = tc.tile_part_packets(data)
    assert [p[0] for p in parts] == list(range(len(parts)))
    total = 0
    for t, _, packets in parts:
        ty, tx = divmod(t, ntx)
        tile = img[ty * r["tile_h"]:(ty + 1) * r["tile_h"], tx * r["tile_w"]:(tx + 1) * r["tile_w"]]
        body, _, _, _ = ol.t1_encode(tc.to_sm(tile), 0, True)
        assert len(packets) == 1
        assert packets[0][1] == body, (t, case["tiles"][t] if t < len(case["tiles"]) else "padding")
        total += len(body)
    assert total == sum(len(b) for _, _, pk in parts for _, b in pk)


def test_band_tiles_transform_to_the_crafted_bands():
    img = tc.bands_image().astype(np.int64) - 32768
    for i, (name, t) in enumerate(tc.band_tiles()):
        y, x = divmod(i, 4)
        f = ol.fdwt(img[y * 2 * N:(y + 1) * 2 * N, x * 2 * N:(x + 1) * 2 * N], 1, True)
        for b, (ys, xs) in enumerate(((0, 0), (0, N), (N, 0), (N, N))):
            assert np.array_equal(f[ys:ys + N, xs:xs + N], t[b]), (name, tc.BAND_NAMES[b])


@pytest.mark.parametrize("group", sorted(tc.RATES))
def test_rate_is_about_half_the_lossless_file(group):
    a = next(c for c in CASES if c["group"] == group and c["kind"] == "a")
    bpp = 8 * len(oracle_file(a)[0]) / tc.image(a).size
    assert 0.4 <= tc.RATES[group] / bpp <= 0.6, (tc.RATES[group], bpp)
    c = next(x for x in CASES if x["group"] == group and x["kind"] == "c")
    assert len(oracle_file(c)[0]) <= tc.RATES[group] * tc.image(a).size / 8 + 1


def _decisions_and_flushes(case, **override):
    ol.census_reset()
    ol.encode(tc.image(case), ol.recipe(case["lossless"], **dict(case["recipe"], **override)))
    c = ol.census_read()
    return int(c["mq"][:, :ol.MQ_SWITCH].sum()), int(c["flush"][:2].sum())


def test_slope_prediction_skips_planes_and_its_safety_net_runs():
    """Recipe (d) reaches both ends of slope prediction: on the noise blocks
    of the geometry cases the skipped planes stay skipped (pmin > 0: fewer
    decisions than without prediction), on the crafted groups the prediction
    undershoots the target and every block is coded again in full (twice the
    flushes)."""
    for case in (c for c in CASES if c["kind"] == "d"):
        with_skip, without = _decisions_and_flushes(case), _decisions_and_flushes(case, slope_skip=0)
        if case["group"] in ("geometry", "straddle"):
            assert with_skip[1] == without[1] and with_skip[0] < without[0], case["name"]
        else:
            assert with_skip[1] == 2 * without[1] and with_skip[0] > without[0], case["name"]


def test_committed_seeds_are_what_the_searches_find():
    assert tc.search_byteout_seeds() == tc.BYTEOUT_SEEDS
    assert tc.search_hvd_seeds() == tc.HVD_SEEDS


# ---- census completeness --------------------------------------------------
# Table C.2's Qe column and the rows with SWITCH = 1, restated from the
# standard (the reachability argument below needs them)
QE = (0x5601, 0x3401, 0x1801, 0x0AC1, 0x0521, 0x0221, 0x5601, 0x5401, 0x4801, 0x3801, 0x3001, 0x2401, 0x1C01, 0x1601,
      0x5601, 0x5401, 0x5101, 0x4801, 0x3801, 0x3401, 0x3001, 0x2801, 0x2401, 0x2201, 0x1C01, 0x1801, 0x1601, 0x1401,
      0x1201, 0x1101, 0x0AC1, 0x09C1, 0x08A1, 0x0521, 0x0441, 0x02A1, 0x0221, 0x0141, 0x0111, 0x0085, 0x0049, 0x0025,
      0x0015, 0x0009, 0x0005, 0x0001, 0x5601)
SWITCH_ROWS = (0, 6, 14)


def unreachable_cells():
    """{(counter, index): reason}: the cells no input can reach, each by an
    argument from Annex C / D -- never by what a run left empty."""
    out = {}
    for cls in range(3):
        for bit in (0, 1):
            out[("zc", (cls, 0, 0, 0, 0, bit))] = \
                "D.3.1: the significance pass codes only samples with a significant neighbour"
    for i, qe in enumerate(QE):
        if qe <= 0x4000:
            # C.2.2 / C.2.3: the exchange needs A - Qe < Qe with A >= 0x8000 before the subtraction
            out[("mq", (i, ol.MQ_MPS_RENORM_XCHG))] = out[("mq", (i, ol.MQ_LPS_XCHG))] = \
                "conditional exchange needs Qe > 0x4000 (A >= 0x8000 on entry)"
        if i not in SWITCH_ROWS:
            out[("mq", (i, ol.MQ_SWITCH))] = "Table C.2: SWITCH is 0 in this row"
    return out


def test_corpus_reaches_every_reachable_census_cell():
    """Every table state 0..46 is reachable (all nineteen contexts start at
    0, 3, 4 or 46 and NMPS/NLPS connect the table), every (h, v, d) fits
    inside a 64x64 block, and every other cell is a branch some input takes:
    so the only empty cells are unreachable_cells()."""
    total = None
    for c in CASES:
        total = ol.census_add(total, oracle_file(c)[1])
    skip = unreachable_cells()
    assert len(skip) == 6 + 2 * sum(q <= 0x4000 for q in QE) + 44
    empty, wrongly_listed = [], []
    for name, shape in ol.CENSUS_LAYOUT:
        for idx in np.ndindex(*shape):
            key = (name, idx)
            n = int(total[name][idx])
            if key in skip:
                if n:
                    wrongly_listed.append((key, n))
            elif n == 0:
                empty.append(key)
    assert not wrongly_listed, wrongly_listed
    assert not empty, empty


def test_byteout_family_takes_every_branch_eight_times():
    total = None
    for _, a in tc.byteout_blocks():
        total = ol.census_add(total, block_census(a)[1])
    assert total["byteout"].min() >= 8, total["byteout"]
    assert total["flush"].min() >= 8, total["flush"]


def test_short_stripes_never_enter_run_mode():
    for h in (1, 2, 3):
        a = np.zeros((h, 33), np.int32)
        a[h - 1, 17] = 5
        _, c = block_census(a)
        assert c["rl"][:ol.RL_DENIED_NEIGHBOUR + 1].sum() == 0 and c["rl"][ol.RL_DENIED_SHORT] == 3 * 33


# ---- per-block maxima -----------------------------------------------------
def test_full_block_carries_the_most_decisions_a_plane_can():
    """8 per stripe column (four samples, each a zero-coding and a sign
    decision) plus the run-mode prefix of the block's first column, whose
    four neighbours-to-be are still insignificant: 8*64*16 + 2.  (Ten per
    column -- 10240 -- would need run mode in every column; see the module
    docstring.)  Every later plane refines all 4096 samples."""
    for name, a in tc.full_blocks()[:4]:
        (_, _, _, planes), c = block_census(a)
        assert planes == 15
        assert c["max"][ol.MAX_PLANE_DECISIONS] == 8 * N * (N // 4) + 2 == 8194, name
        assert c["max"][ol.MAX_BLOCK_DECISIONS] == 8194 + 14 * N * N, name
        assert c["mr"].sum() == 14 * N * N


def test_plane_stream_cap_holds_the_largest_plane():
    # the device's slot for one plane's decisions: 11*w*h/4 + 128 bytes, one per decision
    assert 8194 <= 11 * N * N // 4 + 128


CHAINS = tc.chain_blocks()


@pytest.mark.parametrize("name,block,p", CHAINS, ids=[n for n, _, _ in CHAINS])
def test_chain_depth_is_what_the_scan_order_gives(name, block, p):
    _, c = block_census(block)
    assert c["max"][ol.MAX_SPP_DEPTH] == tc.spp_depth_model(block, p), name


def test_forward_chains_are_the_longest_possible_and_reversed_ones_do_not_propagate():
    depth = {n: int(block_census(a)[1]["max"][ol.MAX_SPP_DEPTH]) for n, a, _ in CHAINS}
    assert tc.longest_forward_chain(N, N) == 220
    assert depth["chain_stair_fwd"] == 220
    assert depth["chain_stair_rev"] <= 1 and depth["chain_up"] <= 1
    # a boustrophedon runs with the scan on every other row whichever end is
    # seeded: one row's worth joins, the next row waits for cleanup
    # (test_chain_depth_is_what_the_scan_order_gives has the exact figures)
    assert N <= depth["chain_serp_fwd"] < 2 * N and N - 1 <= depth["chain_serp_rev"] < 2 * N
    assert depth["chain_down"] == N - 1
    assert len(tc.serpentine()) >= 1000


def test_chain_blocks_split_between_propagation_and_cleanup():
    """The steps the modeller's two exceptions are about: in chain_ur_steps
    the sample at each stripe top joins the pass and the one below it does
    not; in chain_dl_inside the whole diagonal joins; in chain_dl_bottom the
    sample at the stripe bottom does not."""
    d = {n: (a, p) for n, a, p in CHAINS}
    for name, joined_per_group, left_per_group in (("chain_ur_steps", 2, 1), ("chain_dl_inside", 3, 0),
                                                   ("chain_dl_bottom", 1, 1)):
        a, p = d[name]
        groups = int((a == 1 << (p + 1)).sum())
        _, c = block_census(a)
        spp_ones = int(c["zc"][0, :, :, :, 0, 1].sum())
        cup_ones = int(c["zc"][0, :, :, :, 1, 1].sum()) + int(c["rl"][ol.RL_R0:ol.RL_R3 + 1].sum())
        assert spp_ones == joined_per_group * groups, name
        assert cup_ones == (1 + left_per_group) * groups, name   # the seeds, a plane earlier, and the rest


# ---- an independent decoder ------------------------------------------------
LOSSLESS = [c for c in CASES if c["kind"] in "ab"]


@pytest.mark.skipif(im.opj("opj_decompress") is None, reason="opj_decompress not installed")
@pytest.mark.parametrize("case", LOSSLESS, ids=[c["name"] for c in LOSSLESS])
def test_openjpeg_decodes_the_lossless_files_exactly(case):
    data, _ = oracle_file(case)
    img = tc.image(case)
    assert np.array_equal(im.decode_opj(data, ".j2k").reshape(img.shape), img)
