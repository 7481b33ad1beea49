"""Tiles wider and taller than 4096, up to one tile per image, on the GPU:
every file is the oracle's encode of the same pixels with the same recipe,
byte for byte, and the lossless ones decode (OpenJPEG) to the source pixels.
The shapes (tests/large_tile_cases.py) send level 1, levels 2 and 3, or all
of them through the column-chunked DWT kernels (csrc/dwt_chunk.h), lay row
ends around every chunk boundary, cover the tile widths 2560 .. 4096 whose
rows never fitted in LDS, a tile whose Nsop wraps, the untiled recipe
(tile_w = tile_h = 0) and the ingest routes in front of the DWT."""
import numpy as np
import pytest

import imaging as im
import jp2hip
import large_tile_cases as lt
import oracle_lib as ol

pytestmark = pytest.mark.gpu

LL, LY = lt.LL, lt.LY
CONV_ID = {LL: "ll", LY: "ly"}


def check(encoder, img, tif, conv, ov, want_ov=None, decode=True):
    """libjp2hip's file for overrides `ov` is the oracle's for `want_ov`
    (default: the same); a lossless file decodes to the source pixels."""
    got, _ = encoder.encode_tiff(tif, conv, jp2hip.recipe(conv, **ov))
    want = ol.encode(img, ol.copy_recipe(jp2hip.recipe(conv, **(want_ov or ov))))
    assert len(got) == len(want) and got == want
    if conv == LL and decode:
        assert np.array_equal(im.decode_opj(got).reshape(img.shape), img)
    return got


def _numbered():
    return [(c, conv) for c in lt.NUMBERED for conv in c["convs"]]


@pytest.mark.parametrize("c,conv", _numbered(), ids=[f"{c['name']}-{CONV_ID[v]}" for c, v in _numbered()])
def test_numbered_shapes(encoder, c, conv):
    img = lt.image(c["h"], c["w"], c["comps"], c["bits"])
    got = check(encoder, img, im.tiff_bytes(img), conv, c["ov"])
    if c is lt.C9:  # every packet has its SOP; their Nsop runs 0 .. 65535 and starts again
        assert im.expected_packets(got) == lt.C9_PACKETS
        im.tile_part_walk(got, 1)


def _untiled():
    return [(c, conv) for c in lt.UNTILED for conv in c["convs"]]


@pytest.mark.parametrize("c,conv", _untiled(), ids=[f"{c['name']}-{CONV_ID[v]}" for c, v in _untiled()])
def test_untiled_is_the_oracle_at_the_resolved_size(encoder, c, conv):
    """tile_w = tile_h = 0: one tile, the smallest multiples of 2^levels not
    below the image, written to SIZ as they are."""
    img = lt.image(c["h"], c["w"], c["comps"], c["bits"])
    tw, th = lt.resolved(c["w"], c["h"], c["ov"]["levels"])
    got = check(encoder, img, im.tiff_bytes(img), conv, dict(c["ov"], tile_w=0, tile_h=0),
                dict(c["ov"], tile_w=tw, tile_h=th))
    siz = im.main_header_segments(got)["ff51"]
    assert (int.from_bytes(siz[22:26], "big"), int.from_bytes(siz[26:30], "big")) == (tw, th)


EDGES = lt.chunk_edge_cases()


@pytest.mark.parametrize("e", EDGES, ids=[e["name"] for e in EDGES])
def test_chunk_edges(encoder, e):
    """A row end just past, on and around the chunk boundaries of each
    chunked kernel at its level: 9 and 33 rows, 1 and 3 components, 8 and 16
    bits, both conversions."""
    for h, comps, bits in lt.CHUNK_EDGE_VARIANTS:
        img = lt.image(h, e["w"], comps, bits)
        tif = im.tiff_bytes(img)
        for conv in (LL, LY):
            check(encoder, img, tif, conv, e["ov"], decode=(h == 33 and conv == LL))


@pytest.mark.parametrize("conv", [LL, LY], ids=["ll", "ly"])
@pytest.mark.parametrize("comps", lt.GAP_COMPS)
@pytest.mark.parametrize("tile_w", lt.GAP_TILE_WIDTHS)
def test_tile_widths_2560_to_4096(encoder, tile_w, comps, conv):
    """The widths the plan admitted before the chunked kernels existed while
    16 rows of level 1 asked for more LDS than a workgroup has."""
    c = lt.gap_case(tile_w, comps)
    img = lt.image(c["h"], c["w"], c["comps"], c["bits"])
    check(encoder, img, im.tiff_bytes(img), conv, c["ov"])


def _sources():
    return [(c, i) for c, n in ((lt.C1, 4), (lt.C5, 2)) for i in range(n)]


@pytest.mark.parametrize("c,i", _sources(),
                         ids=[f"{c['name']}-{('planar', 'rgba16', 'lzw', 'tiled_tiff')[i]}" for c, i in _sources()])
def test_other_ingest_routes(encoder, c, i):
    """Planar samples, four 16-bit components, LZW strips and a tiled TIFF
    (decoded and untiled on the GPU first) in front of the chunked level 1."""
    _, img, tif = lt.source_variants(c)[i]
    for conv in c["convs"]:
        check(encoder, img, tif, conv, c["ov"])


@pytest.mark.parametrize("conv", [LL, LY], ids=["ll", "ly"])
def test_untiled_through_the_tile_split(tmp_path, conv):
    """An untiled image is one tile row: the tile-split (two peers, world 3)
    gives all of it to rank 0, the other ranks only join the exchanges, and
    the file is the single encode's."""
    c = lt.C1
    img = lt.image(c["h"], c["w"], c["comps"], c["bits"])
    tw, th = lt.resolved(c["w"], c["h"], c["ov"]["levels"])
    want = ol.encode(img, ol.copy_recipe(jp2hip.recipe(conv, **dict(c["ov"], tile_w=tw, tile_h=th))))
    src, out = tmp_path / "src.tif", tmp_path / "out.jpx"
    src.write_bytes(im.tiff_bytes(img))
    enc = jp2hip.Encoder(0)
    try:
        enc.split_peers([0, 0])
        enc.encode_file(str(src), str(out), conv, jp2hip.recipe(conv, **dict(c["ov"], tile_w=0, tile_h=0)))
    finally:
        enc.close()
    assert out.read_bytes() == want
