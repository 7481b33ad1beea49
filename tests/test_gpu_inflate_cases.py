"""k_inflate and k_inflate_links on the crafted Deflate corpus
(tests/inflate_cases.py; test_inflate_cases.py pins its model to zlib and
test_inflate_host.py runs the same streams through the kernel's one-lane host
build).  Here the 64 lanes run them: every match part at every lane of a
window, 13- to 15-bit codes in both tables, the header's extremes, every
stored-block cell, block sequences with changing tables, every way a strip
fills up, link chains 8000 deep and across the 4096-byte blocks of the
resolver, strips starting at every residue modulo 16 and ending at the ring's
chunk boundaries, 200 random streams, and one stream per error door.

The expected file is always the oracle's encode of the model's bytes as
pixels, never the GPU's own encode of an uncompressed twin.  A mismatch names
the strip whose decoded bytes differ."""
import numpy as np
import pytest

import imaging as im
import inflate_cases as fc
import jp2hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu


def oracle(img, rc):
    return ol.encode(img, ol.copy_recipe(rc))


def first_wrong_strip(encoder, tif, want_px, rows_per_unit, names):
    """Which strip decoded wrongly: the file again with no wavelet and no
    colour transform, decoded, compared unit by unit."""
    rc = jp2hip.recipe(jp2hip.LOSSLESS, levels=0, mct=0)
    try:
        got, _ = encoder.encode_tiff(tif, jp2hip.LOSSLESS, rc)
        px = im.decode_pillow(got).reshape(want_px.shape)
    except Exception as e:  # the plain message still names the file
        return f"(no strip named: {type(e).__name__}: {e})"
    for i, name in enumerate(names):
        a, b = px[i * rows_per_unit:(i + 1) * rows_per_unit].ravel(), want_px[i * rows_per_unit:(i + 1) * rows_per_unit].ravel()
        if not np.array_equal(a, b):
            at = int(np.flatnonzero(a != b)[0])
            return f"strip {i} ({name}): byte {at} is {int(a[at])}, the model says {int(b[at])}; {int((a != b).sum())} differ"
    return "(every strip decodes to the model's bytes with levels=0: the difference is past the decoder)"


def check(encoder, tif, want_px, rows_per_unit, names):
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    got, _ = encoder.encode_tiff(tif, jp2hip.LOSSLESS, rc)
    if got != oracle(want_px, rc):
        raise AssertionError(f"{names[0]}..: " + first_wrong_strip(encoder, tif, want_px, rows_per_unit, names))


FILES = fc.valid_files()


@pytest.mark.parametrize("family", [f for f in fc.FAMILIES if f != "errors"])
def test_valid_families(encoder, family):
    """Every valid case of a family, several strips to a file; one file of
    each family tagged 32946, the rest 8."""
    files = [f for f in FILES if f.names[0].startswith(family)]
    assert files and (family == "random" or any(f.compression == 32946 for f in files))
    for f in files:
        check(encoder, f.tiff(), f.pixels(), f.rps, f.names)


PAIRS = fc.error_pairs()


@pytest.mark.parametrize("k", range(len(PAIRS)), ids=[p[0] for p in PAIRS])
def test_error_doors(encoder, k):
    """The bad strip is refused, then the same context encodes the good twin."""
    name, bad, good = PAIRS[k]
    rc = jp2hip.recipe(jp2hip.LOSSLESS)
    with pytest.raises(jp2hip.Jp2hipError, match="corrupt"):
        encoder.encode_tiff(bad.tiff(), jp2hip.LOSSLESS, rc)
    got, _ = encoder.encode_tiff(good.tiff(), jp2hip.LOSSLESS, rc)
    assert got == oracle(good.pixels(), rc)  # (no stale table, link or error flag)


TILES = fc.tile_files()


@pytest.mark.parametrize("k", range(len(TILES)), ids=[t[0] for t in TILES])
def test_tiles_and_predictor(encoder, k):
    name, tif, px = TILES[k]
    n = 4 if name.startswith("phase") else 3
    check(encoder, tif, px, px.shape[0] // n, [f"{name}_{i}" for i in range(n)])


def test_crafted_strips_next_to_zlib_strips(encoder):
    f = fc.mixed_file()
    check(encoder, f.tiff(), f.pixels(), f.rps, f.names)
