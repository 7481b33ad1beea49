"""Tiles wider than 4096 and the untiled recipe (tile_w = tile_h = 0), as far
as the host decides them: the plan is built (jp2hip_packet_sequence builds
the plan an encode builds, refusals included), 0 / 0 resolves to one tile of
the smallest multiples of 2^levels, half-stated and negative sizes are
refused by name, an untiled image's tile-split band is rank 0's, the chunk
constants the GPU cases are laid around are the header's, and the DWT routes
those cases name are the ones csrc/dwt_route.h gives them.  No GPU."""
import os
import re
from ctypes import byref

import pytest

import jp2hip
import large_tile_cases as lt
from jp2hip import split as js
from test_dwt_route_host import route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seq(w, h, comps, bits, **ov):
    return jp2hip.packet_sequence(w, h, comps, bits, jp2hip.recipe(jp2hip.LOSSLESS, **ov), 0)


def test_plan_of_a_tile_wider_than_4096():
    c = lt.C2
    seq = _seq(c["w"], c["h"], c["comps"], c["bits"], **c["ov"])
    assert len(seq) > 0 and sorted(seq) == list(range(len(seq)))


def test_untiled_is_one_tile_of_the_resolved_size():
    c = lt.C2
    tw, th = lt.resolved(c["w"], c["h"], c["ov"]["levels"])
    assert (tw, th) == (8320, 64)
    untiled = _seq(c["w"], c["h"], c["comps"], c["bits"], **dict(c["ov"], tile_w=0, tile_h=0))
    assert untiled == _seq(c["w"], c["h"], c["comps"], c["bits"], **dict(c["ov"], tile_w=tw, tile_h=th))
    # one tile: there is no tile 1
    with pytest.raises(jp2hip.Jp2hipError, match="tile index"):
        jp2hip.packet_sequence(c["w"], c["h"], c["comps"], c["bits"],
                               jp2hip.recipe(jp2hip.LOSSLESS, **dict(c["ov"], tile_w=0, tile_h=0)), 1)


@pytest.mark.parametrize("tw,th", [(0, 64), (64, 0), (-64, 64), (64, -64), (-64, -64), (0, -64)])
def test_half_stated_and_negative_tile_sizes_are_refused(tw, th):
    with pytest.raises(jp2hip.Jp2hipError, match="tile size"):
        _seq(300, 40, 1, 8, levels=6, tile_w=tw, tile_h=th)


def test_tile_sizes_stay_multiples_of_2_to_the_levels():
    with pytest.raises(jp2hip.Jp2hipError, match="tile size"):
        _seq(8300, 40, 1, 8, levels=6, tile_w=8300, tile_h=64)


def test_the_remaining_limit_is_named():
    """32768 on a side (include/jp2hip.h, tile_w / tile_h), stated or resolved."""
    with pytest.raises(jp2hip.Jp2hipError, match="32768"):
        _seq(100, 40, 1, 8, levels=6, tile_w=32768 + 64, tile_h=64)
    with pytest.raises(jp2hip.Jp2hipError, match="32768"):
        _seq(40000, 40, 1, 8, levels=6, tile_w=0, tile_h=0)
    assert len(_seq(100, 40, 1, 8, levels=6, tile_w=32768, tile_h=64)) > 0


def test_nsop_case_has_more_packets_than_nsop_counts():
    c = lt.C9
    assert len(_seq(c["w"], c["h"], c["comps"], c["bits"], **c["ov"])) == lt.C9_PACKETS > 65536


def test_zplt_limit_is_refused_by_name():
    """2 x 2 precincts of a 512 x 256 tile of 4 components under 32 layers:
    4.2 M packets in the top resolution's tile-part, whose lengths -- up to 5
    bytes each -- may not fit the 256 PLT segments Zplt can number.  Without
    the PLT the recipe stands."""
    ov = dict(levels=1, layers=32, tile_w=512, tile_h=256, nprecincts=1, prec_w_log2=[1], prec_h_log2=[1],
              cblk_w_log2=2, cblk_h_log2=2)

    def count(**more):  # cap = 0: the count alone
        rc = jp2hip.recipe(jp2hip.LOSSLESS, **dict(ov, **more))
        return jp2hip._lib.lib().jp2hip_packet_sequence(512, 256, 4, 8, byref(rc), 0, None, 0)

    assert count() < 0
    assert "Zplt" in jp2hip._lib.last_error()
    assert count(plt=0) == (128 * 64 + 256 * 128) * 4 * 32


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_untiled_split_gives_rank_0_the_image(world):
    h = 4000
    bands = [js.split_rows(h, 0, r, world, 1024) for r in range(world)]
    assert bands[0] == (0, h)
    assert all(r0 == r1 for r0, r1 in bands[1:])
    # contiguous, in rank order, like every other split
    assert all(bands[r][1] == bands[r + 1][0] for r in range(world - 1))


def test_case_constants_are_the_headers():
    with open(os.path.join(ROOT, "jp2-bucketeer_amd", "csrc", "dwt_chunk.h")) as f:
        src = f.read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+);", src)}
    assert consts["kL1ChunkW"] == lt.L1_CHUNK_W
    assert consts["kBandChunkW"] == lt.BAND_CHUNK_W
    assert consts["kDwtChunkHalo"] == lt.CHUNK_HALO


@pytest.mark.parametrize("nc", [1, 3])
def test_chunked_from_level_is_the_routes(nc):
    """The tile widths the chunk-edge cases use to send a level to the chunked
    kernels (large_tile_cases.CHUNKED_FROM_LEVEL), and the widest whole-row
    level they are laid around, as csrc/dwt_route.h routes them today."""
    for lv, tw in lt.CHUNKED_FROM_LEVEL.items():
        r = route(tw, 64, nc, 6)
        assert [x["level"] for x in r[:lv + 1]] == list(range(1, lv + 2))
        assert [x["form"] for x in r[:lv]] == ["L1Chunk"] + ["BandChunk"] * (lv - 1), (tw, r)
        assert r[lv]["form"] == "Band" and r[lv]["gz"] == 1, (tw, r)
    # a level the band kernel lifts -- level 2 of a one-component tile, and
    # level 1 of a three-component one (k_dwt_band with ingest) -- on either
    # side of the limit
    W = lt.WHOLE_ROW_MAX_W
    assert [x["form"] for x in route(2 * W, 64, 1, 6)[:2]] == ["L1Chunk", "Band"]
    assert [x["form"] for x in route(2 * W + 1, 64, 1, 6)[:2]] == ["L1Chunk", "BandChunk"]
    assert route(2 * W, 64, 1, 6)[1]["W"] == W and route(2 * W + 1, 64, 1, 6)[1]["W"] == W + 1
    assert route(W, 64, 3, 6)[0]["form"] == "BandIngest"
    assert route(W + 1, 64, 3, 6)[0]["form"] == "L1Chunk"


def _corpus_tiles():
    """(tile_w, tile_h, components, levels) of every encode of the GPU cases
    that are laid around a DWT route: the case lists, not their fixtures."""
    import test_gpu_dwt_fetch as tf
    import test_gpu_parity as tp

    def tile(w, h, comps, **ov):
        rc = jp2hip.recipe(jp2hip.LOSSLESS, **ov)
        tw, th = (rc.tile_w, rc.tile_h) if rc.tile_w else lt.resolved(w, h, rc.levels)
        return tw, th, comps, rc.levels

    out = [tile(w, h, nc, levels=levels, tile_w=t, tile_h=t) for h, w, nc, _, _, levels, t in tp.CASES]
    out += [tile(c["w"], c["h"], c["comps"], **c["ov"]) for c in lt.NUMBERED]
    out += [tile(c["w"], c["h"], c["comps"], **dict(c["ov"], tile_w=0, tile_h=0)) for c in lt.UNTILED]
    out += [tile(e["w"], h, comps, **e["ov"]) for e in lt.chunk_edge_cases() for h, comps, _ in lt.CHUNK_EDGE_VARIANTS]
    out += [tile(c["w"], c["h"], c["comps"], **c["ov"])
            for c in (lt.gap_case(tw, comps) for tw in lt.GAP_TILE_WIDTHS for comps in lt.GAP_COMPS)]
    out += [tile(w, h, 3, **ov) for w, h, _, ov in tf.SHAPES]
    out += [tile(w, h, 4 if kind == "rgba8" else 1 if kind.startswith("gray") else 3)
            for kind, _ in tf.LAYOUTS for w, h in tf.LAYOUT_SIZES]
    out += [tile(*tf.PLACEMENT_SIZE, 3), tile(tf.LEVELS_2_UP[0], tf.LEVELS_2_UP[1], 3, **tf.LEVELS_2_UP[2]),
            tile(tf.BAND_EDGES[0], tf.BAND_EDGES[1], 3, **tf.BAND_EDGES[2])]
    return sorted(set(out))


def test_gpu_corpus_reaches_every_dwt_form():
    """The byte-identity cases of test_gpu_parity, test_gpu_large_tiles and
    test_gpu_dwt_fetch between them launch every kernel form of dwt.hip:
    a retuned limit in csrc/dwt_route.h that takes one away fails here."""
    seen = set()
    for tw, th, nc, levels in _corpus_tiles():
        for x in route(tw, th, nc, levels):
            seen.add((x["form"], x["cpt"] if x["form"] == "L1Stream" else x["threads"] if x["form"] == "Band" else 0))
    want = {("L1Stream", 1), ("L1Stream", 2), ("L1Stream", 4), ("L1Window", 0), ("L1Chunk", 0), ("BandIngest", 0),
            ("Band", 128), ("Band", 256), ("BandChunk", 0), ("Tail", 0)}
    assert want - seen == set(), sorted(seen)
    assert seen - want == set(), sorted(seen)
