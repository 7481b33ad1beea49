"""The oracle over the cases of tests/recipe_axes_cases.py (CPU only): the
reference decoder (opj_decompress) reads every file, lossless files decode to
the source exactly, rate-driven files keep their byte target, an independent
walk of the tile-parts (imaging.tile_part_walk) agrees with the PLT, SOP and
tile-part structure, and each case is on the code path it exists for
(recipe_axes_cases.check_pins).  This is what lets the GPU test
(tests/test_gpu_recipe_axes.py) treat the oracle's bytes as the answer.

Then invariants of the fields themselves, each exact: the marker switches
and guard_bits change no decoded pixel, mct=0 codes each component as if it
were alone, a finer qstep never lowers PSNR, and the deepest quantisers
(Mb 29 / 30) lose nothing.  And the recipes that cannot be written into the
main header's fields are refused.
"""
import numpy as np
import pytest

import imaging as im
import oracle_lib as ol
import recipe_axes_cases as rac

CASES = rac.cases()


def _encode(case, **more):
    return ol.encode(rac.image(case), ol.recipe(case["lossless"], **dict(case["recipe"], **more)))


@pytest.mark.parametrize("case", CASES, ids=[rac.case_id(c) for c in CASES])
def test_oracle_case_decodes(case):
    img = rac.image(case)
    r = case["recipe"]
    cs = _encode(case)
    dec = im.decode_opj(cs, ".j2k").reshape(img.shape)
    if case["lossless"] and r["rate_bpp"] <= 0:
        assert np.array_equal(dec, img)
    else:
        target = r["rate_bpp"] * case["h"] * case["w"] / 8
        if target > 20000:  # below that the packet headers alone can exceed it
            assert len(im.codestream(cs)) <= target + 0.5
    walk = rac.check_structure(case, cs)
    rac.check_pins(case, cs, walk)
    if case["axis"] == "deep" and r["levels"] == 0 and r["rate_bpp"] <= 0:
        assert np.array_equal(dec, img)  # Delta <= 2^-11: every sample survives


def test_axis_counts():
    n = {}
    for c in CASES:
        n[c["axis"]] = n.get(c["axis"], 0) + 1
    assert n == dict(markers=32, mct0=32, guard=35, qstep=20, deep=9, tiny=42, plt=4)
    assert len({rac.case_id(c) for c in CASES}) == len(CASES)


# ---- invariants -------------------------------------------------------------

def _allpass(img, **ov):
    """Decode of an irreversible encode with every coding pass kept."""
    rc = dict(rac.J2K, tile_w=256, tile_h=256, rate_bpp=0.0)
    return im.decode_opj(ol.encode(img, ol.recipe(False, **dict(rc, **ov))), ".j2k").reshape(img.shape)


@pytest.fixture(scope="module")
def rgb8():
    return im.synth_rgb8(300, 420, seed=11)


@pytest.fixture(scope="module")
def rgb8_default_decode(rgb8):
    return _allpass(rgb8)


@pytest.mark.parametrize("ov", [dict(sop=0), dict(eph=0), dict(plt=0), dict(tparts_r=0),
                                dict(sop=0, eph=0, plt=0, tparts_r=0), dict(guard_bits=0), dict(guard_bits=2),
                                dict(guard_bits=5), dict(guard_bits=7)],
                         ids=lambda ov: "_".join(f"{k}{v}" for k, v in ov.items()))
def test_switches_and_guard_bits_change_no_pixel(rgb8, rgb8_default_decode, ov):
    assert np.array_equal(_allpass(rgb8, **ov), rgb8_default_decode)


@pytest.mark.parametrize("nc,bits", [(3, 8), (4, 8), (3, 16), (4, 16)])
@pytest.mark.parametrize("levels", [0, 3])
def test_mct0_codes_each_component_alone(nc, bits, levels):
    img = rac.sc._content("synth", 140, 190, nc, bits, 5)
    ov = dict(mct=0, levels=levels, tile_w=128, tile_h=128)
    dec = _allpass(img, **ov)
    for c in range(nc):
        plane = np.ascontiguousarray(img[..., c])
        assert np.array_equal(dec[..., c], _allpass(plane, **ov)), f"component {c}"


@pytest.mark.parametrize("nc,bits", [(3, 8), (1, 16)])
def test_finer_qstep_never_lowers_psnr(nc, bits):
    img = rac.sc._content("synth", 150, 210, nc, bits, 7)
    p = [im.psnr(img, _allpass(img, qstep=q, levels=4, tile_w=128, tile_h=128), bits)
         for q in (2.0,) + rac.QSTEPS]
    assert all(b >= a for a, b in zip(p, p[1:])), p


# ---- recipes the main header cannot hold ------------------------------------

@pytest.mark.parametrize("field,ov", rac.BAD, ids=rac.BAD_IDS)
def test_oracle_rejects_recipe(field, ov):
    img = im.synth_u16(40, 50, comps=1, seed=1)
    with pytest.raises(RuntimeError, match=field):
        ol.encode(img, ol.recipe(False, **ov))


def test_oracle_rejects_more_than_65535_tiles():
    img = np.zeros((1024, 1028), np.uint8)  # 256 x 257 tiles of 4x4
    rc = dict(tile_w=4, tile_h=4, levels=0)
    with pytest.raises(RuntimeError, match="tile"):
        ol.encode(img, ol.recipe(True, **rc))
    # 255 x 257 = 65535 tiles is the most Isot can number
    assert ol.encode(img[:1020], ol.recipe(True, **dict(rc, format=0)))[-2:] == b"\xff\xd9"


def test_unused_precinct_entries_are_not_read():
    """Only the entries a resolution uses are checked (nprecincts=1: the first)."""
    img = im.synth_rgb8(40, 50, seed=1)
    a = ol.encode(img, ol.recipe(True, nprecincts=1, prec_w_log2=[7, 99], prec_h_log2=[7, -5]))
    assert a == ol.encode(img, ol.recipe(True, nprecincts=1, prec_w_log2=[7], prec_h_log2=[7]))


def test_precinct_exponent_0_is_legal_at_resolution_0():
    img = im.synth_rgb8(20, 30, seed=1)
    cs = ol.encode(img, ol.recipe(True, nprecincts=1, prec_w_log2=[0], prec_h_log2=[0], levels=0, format=0))
    assert np.array_equal(im.decode_opj(cs, ".j2k"), img)
    assert sum(len(tp[4]) for tp in im.tile_part_walk(cs, 1)) == 20 * 30 * 3 * 6
