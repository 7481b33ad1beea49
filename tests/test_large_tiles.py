"""Tiles wider than 4096 and the untiled recipe (tile_w = tile_h = 0), as far
as the host decides them: the plan is built (jp2hip_packet_sequence builds
the plan an encode builds, refusals included), 0 / 0 resolves to one tile of
the smallest multiples of 2^levels, half-stated and negative sizes are
refused by name, an untiled image's tile-split band is rank 0's, and the
chunk constants the GPU cases are laid around are the header's.  No GPU."""
import os
import re
from ctypes import byref

import pytest

import jp2hip
import large_tile_cases as lt
from jp2hip import split as js

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
