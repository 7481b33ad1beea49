"""GPU parity over the recipe fields and device paths the seeded sweep leaves
alone (tests/recipe_axes_cases.py): the marker switches sop / eph / plt /
tparts_r, mct=0, guard_bits, the qstep ladder, bands of up to 30 bit-planes,
tiles down to 1x1 and PLT chains of 2-4 segments.  Each case is encoded by
libjp2hip through the C ABI and byte-compared with the CPU oracle, which
tests/test_oracle_recipe_axes.py checks against OpenJPEG and an independent
tile-part walk.  Then the recipes the main header cannot hold: refused, with
the context still good afterwards.
"""
import numpy as np
import pytest

import imaging as im
import jp2hip
import oracle_lib as ol
import recipe_axes_cases as rac

pytestmark = pytest.mark.gpu

CASES = rac.cases()


def assert_same_bytes(got, want):
    if got != want:
        n = min(len(got), len(want))
        d = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{len(got)} vs {len(want)} bytes, first difference at byte {d}")


@pytest.mark.parametrize("case", CASES, ids=[rac.case_id(c) for c in CASES])
def test_case_identical_to_oracle(encoder, case):
    img = rac.image(case)
    conv = jp2hip.LOSSLESS if case["lossless"] else jp2hip.LOSSY
    rc = jp2hip.recipe(conv, **case["recipe"])
    want = ol.encode(img, ol.copy_recipe(rc))
    rac.check_pins(case, want)
    got, _ = encoder.encode_tiff(im.tiff_bytes(img), conv, rc)
    assert_same_bytes(got, want)
    if case["lossless"] and case["recipe"]["rate_bpp"] <= 0:
        assert np.array_equal(im.decode_opj(got, ".j2k").reshape(img.shape), img)
    if case["axis"] in ("markers", "plt"):
        rac.check_structure(case, got)


# ---- recipes the main header cannot hold ------------------------------------

@pytest.fixture(scope="module")
def good():
    img = im.synth_u16(40, 50, comps=1, seed=1)
    rc = jp2hip.recipe(jp2hip.LOSSY)
    return im.tiff_bytes(img), rc, ol.encode(img, ol.copy_recipe(rc))


def _still_good(encoder, good):
    tif, rc, want = good
    got, _ = encoder.encode_tiff(tif, jp2hip.LOSSY, rc)
    assert_same_bytes(got, want)


@pytest.mark.parametrize("field,ov", rac.BAD + [("30 magnitude bit-planes", dict(levels=0, qstep=2.0 ** -31))],
                         ids=rac.BAD_IDS + ["Mb31"])
def test_recipe_rejected_and_context_survives(encoder, good, field, ov):
    with pytest.raises(jp2hip.Jp2hipError, match=field):
        encoder.encode_tiff(good[0], jp2hip.LOSSY, jp2hip.recipe(jp2hip.LOSSY, **ov))
    _still_good(encoder, good)


def test_more_than_65535_tiles_rejected(encoder, good):
    """257 x 256 tiles: refused by the plan, before any table of it is built
    or kernel launched -- the context, which has just encoded the same image
    with the default recipe, holds exactly the device memory it held."""
    tif = im.tiff_bytes(np.zeros((1024, 1028), np.uint8))
    rc = jp2hip.recipe(jp2hip.LOSSLESS, tile_w=4, tile_h=4, levels=0)
    encoder.encode_tiff(tif, jp2hip.LOSSLESS)
    before = encoder.device_bytes()
    with pytest.raises(jp2hip.Jp2hipError, match="tile"):
        encoder.encode_tiff(tif, jp2hip.LOSSLESS, rc)
    assert encoder.device_bytes() == before
    _still_good(encoder, good)
