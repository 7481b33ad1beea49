"""Fixed-slope quality layers on the CPU: the refusals of
jp2hip_check_layer_slopes, the log2 helpers against each other and against the
COM text of an oracle file, the preconditions of every case of
tests/slope_cases.py, and the report's distortion definition against a
decoder: on the levels = 0 case the sums derived from the oracle's export are
the summed squared error of the image opj_decompress -l decodes.
"""
import math

import numpy as np
import pytest

import imaging as im
import jp2hip
import slope_cases as sc

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY
NAN, INF = float("nan"), float("inf")


# ---- refusals ------------------------------------------------------------------------

@pytest.mark.parametrize("slopes,recipe,match", [
    ([4.0, NAN, 0.0], None, r"slopes\[1\].*NaN"),
    ([NAN], None, r"slopes\[0\].*NaN"),
    ([4.0, 2.0, -1.0], None, r"slopes\[2\].*negative"),
    ([4.0, -0.0], None, r"slopes\[1\].*negative"),
    ([4.0, 2.0, 3.0, 0.0], None, r"slopes\[2\] increases over slopes\[1\]"),
    ([1.0, INF], None, r"slopes\[1\] increases"),
    ([4.0, 2.0, 0.0], dict(conv=LL, layers=6), r"n = 3.*layers = 6"),
    ([4.0] * 7, dict(conv=LY, layers=6), r"n = 7.*layers = 6"),
    ([4.0, 2.0, 1.0], dict(conv=LL, layers=3), r"slopes\[2\], the last, must be 0"),
    ([4.0, 2.0, 1.0], dict(conv=LY, layers=3, rate_bpp=0.0), r"slopes\[2\], the last, must be 0"),
    ([1.0] * 33, None, r"n = 33"),
])
def test_check_refuses_by_name(slopes, recipe, match):
    rc = None if recipe is None else jp2hip.recipe(recipe.pop("conv"), **recipe)
    with pytest.raises(jp2hip.Jp2hipError, match=match):
        jp2hip.check_layer_slopes(slopes, rc)


@pytest.mark.parametrize("slopes,recipe", [
    ([], None), (None, None), ([INF, INF, 5.0, 5.0, 0.0, 0.0], None), ([0.0], None),
    ([4.0, 2.0, 0.0], dict(conv=LL, layers=3)), ([4.0, 2.0, 1.0], dict(conv=LY, layers=3)),
    ([], dict(conv=LL, layers=3)), ([INF] * 32, dict(conv=LY, layers=32)),
])
def test_check_accepts(slopes, recipe):
    jp2hip.check_layer_slopes(slopes, None if recipe is None else jp2hip.recipe(recipe.pop("conv"), **recipe))


# ---- the log2 helpers ----------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 12, 16])
def test_log2_helpers_invert_each_other(bits):
    for v in (-40.0, -3.5, 0.0, 0.1, 7.25, 31.9):
        s = jp2hip.slope_from_log2(v, bits)
        assert s == 2.0 ** (v + 2 * bits)
        assert abs(jp2hip.slope_to_log2(s, bits) - v) <= 1e-12 * max(1.0, abs(v))
    for s in (1e-9, 0.75, 1.0, 657.25, 2.3e6):
        assert abs(jp2hip.slope_from_log2(jp2hip.slope_to_log2(s, bits), bits) / s - 1.0) <= 1e-12
    assert jp2hip.slope_to_log2(0.0, bits) == -INF and jp2hip.slope_to_log2(INF, bits) == INF


@pytest.mark.parametrize("name", ["rgb_2.0bpp_12ly", "grey16_2bpp", "lossless_one_group"])
def test_helpers_agree_with_the_com_text_of_an_oracle_file(name):
    """The oracle prints Kc per layer; slope_to_log2 of the same key as a
    threshold, rendered as the COM renders it, is that text -- and reading
    the text back with slope_from_log2 lands within the printed precision."""
    conv, rc = sc.recipe(name)
    e = sc.expectation(name)
    bits = sc.image(name).dtype.itemsize * 8
    lines = sc.com_lines(e["file"], rc.layers)
    assert [t for t, _ in lines] == [sc.slope_text(s, bits) for s in e["slopes"]]
    for (text, _), s in zip(lines, e["slopes"]):
        if 0.0 < s < INF:
            assert abs(math.log2(jp2hip.slope_from_log2(float(text), bits) / s)) <= 0.05 + 1e-9


# ---- the cases -----------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_preconditions(name):
    """expectation() asserts them; the thresholds it hands out also pass the
    library's own check for the case's recipe, at Kc, at K and halfway."""
    conv, rc = sc.recipe(name)
    e = sc.expectation(name)
    assert e["groups"] == (4 if name in sc.MULTI_GROUP else 1)
    jp2hip.check_layer_slopes(e["slopes"], rc)
    if e["groups"] == 1:
        jp2hip.check_layer_slopes(e["top"], rc)
        jp2hip.check_layer_slopes([sc.halfway(a, b) for a, b in zip(e["slopes"], e["top"])], rc)
    for a, b in zip(e["slopes"], e["top"]):
        assert a <= b


def test_nothing_taken_layers_have_a_finite_kc_and_no_k():
    e = sc.expectation(sc.NOTHING_TAKEN)
    empty = [l for l, k in enumerate(e["top"]) if math.isinf(k)]
    assert empty and all(math.isfinite(e["slopes"][l]) for l in empty)


# ---- the distortion definition against a decoder ----------------------------------------

@pytest.mark.skipif(im.opj("opj_decompress") is None, reason="opj_decompress not installed")
def test_levels0_distortion_is_the_decoded_squared_error():
    """levels = 0, no colour transform: the code-blocks tile the image and the
    weights are 1, so the export-derived D[l] is the squared error of the image
    decoded from the first l + 1 layers -- within 0.1 % at every layer (the
    decoder reconstructs mid-interval, which the encoder's estimate of a pass's
    distortion decrease assumes only on average)."""
    name = "levels0"
    conv, rc = sc.recipe(name)
    e = sc.expectation(name)
    img = sc.image(name).astype(np.int64)
    for l in range(rc.layers):
        dec = im.decode_opj(e["file"], layers=l + 1).astype(np.int64).reshape(img.shape)
        sse = float(((dec - img) ** 2).sum())
        print(f"layer {l}: D = {e['distortion'][l]:.6g}, decoded SSE = {sse:.6g}")
        assert abs(e["distortion"][l] - sse) <= 1e-3 * sse, (l, e["distortion"][l], sse)
