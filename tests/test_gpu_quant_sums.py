"""GPU parity of the quantiser's per-plane sums (front.hip k_quant): the
predicted sizes `est` and the distortion decreases `dref` / `dsig` of every
bit-plane, whose sv / sl parts the kernel sums once per block from per-lane
partials kept in LDS; the 64- and 32-row variants of its column load; and the
bit transposes that make the plane masks of columns of at most 8 and at most
16 magnitude bits.  The sums steer slope prediction (which planes are coded),
the PCRD hulls and so the layers' bytes, and the masks are what tier-1 codes:
every case is encoded through the C ABI and byte-compared with the CPU oracle,
as tests/test_gpu_t1_blocks.py does, with recipe kinds a-d of
tests/t1_block_cases.py (lossless with 1 and 32 layers, rate-driven without and
with slope prediction).  levels=0, one component, one code-block per tile:
8-bit samples run the 16-bit index-plane instances, 16-bit lossless samples
and small quantiser steps the 32-bit ones.

  patterns  an empty block (P = 0); one non-zero sample in each corner (lanes 0
            and 63, rows 0 and h - 1 of the neighbour count); a checkerboard of
            zero and non-zero samples (the largest neighbour count); every
            sample at the largest magnitude (the largest sv / sl totals: the
            64-bit sums); blocks of one bit-plane (P = 1)
  sizes     1x1 ... 63x64, one block each: the edges of the row-count
            variants (h <= 32 / h > 32) and of the valid-sample mask
  planes    blocks of many planes.  The reduction sums two rows per plane (sv
            and sl; the counts stay on the packed scans of the plane loop), so
            a block has at most 48 rows and one round of 64 always serves: a
            16-bit lossless levels=2 image with a block of P >= 17 (34 rows),
            and 8-bit samples quantised with steps 2^-12 ... 2^-27 for P = 11
            and 14 (the 16-bit transpose, also in blocks of at most 32 rows),
            22 and 24 (44 and 48 rows) and 26 (the planes above 23 on their
            own path)
"""
import numpy as np
import pytest

import imaging as im
import jp2hip
import oracle_lib as ol
import t1_block_cases as tc

pytestmark = pytest.mark.gpu

N = tc.N


def _patterns(top: int):
    yy, xx = np.mgrid[0:N, 0:N]
    r = np.random.default_rng([tc.SEED, 77, top])
    z = np.zeros((N, N), np.int64)
    out = [("zero", z.copy())]
    for name, (x, y) in (("corner_tl", (0, 0)), ("corner_tr", (N - 1, 0)), ("corner_bl", (0, N - 1)),
                         ("corner_br", (N - 1, N - 1))):
        a = z.copy()
        a[y, x] = -top if name == "corner_tr" else top
        out.append((name, a))
    out.append(("checker_top", np.where((xx + yy) & 1, top, 0)))
    out.append(("checker_one", np.where((xx + yy) & 1, 0, -1)))
    out.append(("full_pos", np.full((N, N), top)))
    out.append(("full_neg", np.full((N, N), -top)))
    out.append(("full_min", np.full((N, N), -top - 1)))
    out.append(("one_plane_full", np.where(r.random((N, N)) < 0.5, -1, 1)))
    out.append(("one_plane_sparse", (r.random((N, N)) < 0.05) * np.where(r.random((N, N)) < 0.5, -1, 1)))
    out.append(("one_plane_single", np.where((xx == 31) & (yy == 32), 1, 0)))
    return [(n, a.astype(np.int32)) for n, a in out]


SIZES = ((1, 1), (3, 5), (8, 8), (16, 16), (17, 64), (64, 17), (31, 33), (32, 32), (33, 31), (63, 64))
PATTERN_RATE = {8: 1.0}


def _cases():
    out = []
    for bits, kinds in ((8, tc.KINDS), (16, ("a", "b"))):
        blocks = _patterns((1 << (bits - 1)) - 1)
        for k in kinds:
            lossless, rc = tc.recipe_for(k, bits, PATTERN_RATE.get(bits, 0.0))
            out.append(dict(name=f"patterns_{bits}b_{k}", kind=k, bits=bits, lossless=lossless, recipe=rc,
                            tiles=[(n, N, N) for n, _ in blocks], make=("patterns", bits)))
    for i, (w, h) in enumerate(SIZES):
        for bits, kinds in ((8, tc.KINDS), (16, ("a",))):
            for k in kinds:
                lossless, rc = tc.recipe_for(k, bits, tc.GEOMETRY_RATE[bits], tile_w=w, tile_h=h)
                out.append(dict(name=f"size_{w}x{h}_{bits}b_{k}", kind=k, bits=bits, lossless=lossless, recipe=rc,
                                tiles=[("noise", w, h)], make=("noise", w, h, bits, tc.SEED + 900 + i)))
    return out


CASES = _cases()
_IMAGES = {}


def _image(case) -> np.ndarray:
    m = case["make"]
    if m not in _IMAGES:
        if m[0] == "patterns":
            _IMAGES[m] = tc.assemble(_patterns((1 << (m[1] - 1)) - 1), m[1], per_row=5)
        else:
            _, w, h, bits, seed = m
            r = np.random.default_rng(seed)
            _IMAGES[m] = r.integers(0, 1 << bits, (h, w)).astype(np.uint16 if bits == 16 else np.uint8)
    return _IMAGES[m]


def _check(encoder, case, img):
    conv = jp2hip.LOSSLESS if case["lossless"] else jp2hip.LOSSY
    rc = jp2hip.recipe(conv, **case["recipe"])
    got, _ = encoder.encode_tiff(im.tiff_bytes(img), conv, rc)
    want = ol.encode(img, ol.copy_recipe(rc))
    if got != want:
        raise AssertionError(tc.describe_mismatch(case, got, want))
    return got


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_sums_identical_to_oracle(encoder, case):
    img = _image(case)
    got = _check(encoder, case, img)
    if case["kind"] == "a":
        assert np.array_equal(im.decode_opj(got, ".j2k").reshape(img.shape), img)


def _deep16_image() -> np.ndarray:
    """128x128 samples at the two ends of the 16-bit range, independently: the
    level-1 HH coefficients reach two bits above the samples."""
    r = np.random.default_rng([tc.SEED, 78])
    return np.where(r.random((2 * N, 2 * N)) < 0.5, 0, 65535).astype(np.uint16)


def test_lossless_16bit_two_levels_many_planes(encoder):
    img = _deep16_image()
    # the oracle's own transform and tier-1 say how many planes the level-1
    # blocks have (Mallat layout: HL top right, LH bottom left, HH bottom right)
    f = ol.fdwt(img.astype(np.int32) - 32768, 2, True)
    planes = [ol.t1_encode(tc.to_sm(f[y:y + N, x:x + N]), band, True)[3]
              for band, (y, x) in ((1, (0, N)), (2, (N, 0)), (3, (N, N)))]
    assert max(planes) >= 17, planes
    lossless, rc = tc.recipe_for("a", 16, 0.0, levels=2, tile_w=2 * N, tile_h=2 * N)
    case = dict(name="deep16_levels2", kind="a", bits=16, lossless=lossless, recipe=rc, tiles=[("extremes", 2 * N, 2 * N)])
    got = _check(encoder, case, img)
    assert np.array_equal(im.decode_opj(got, ".j2k").reshape(img.shape), img)


@pytest.mark.parametrize("kind", ("c", "d"))
@pytest.mark.parametrize("shift", (4, 7, 15, 17, 19), ids=("P11", "P14", "P22", "P24", "P26"))
def test_many_planes(encoder, shift, kind):
    """8-bit patterns with step 2^-(8 + shift): the indices are the
    magnitudes times 2^shift, so the full blocks have 7 + shift planes."""
    blocks = _patterns(127)
    assert (int(dict(blocks)["full_pos"].max()) << shift).bit_length() == 7 + shift
    _, rc = tc.recipe_for(kind, 8, 1.0)
    rc = dict(rc, qstep=2.0 ** -(8 + shift))
    case = dict(name=f"planes_P{7 + shift}_{kind}", kind=kind, bits=8, lossless=False, recipe=rc,
                tiles=[(n, N, N) for n, _ in blocks])
    _check(encoder, case, _image(dict(make=("patterns", 8))))


@pytest.mark.parametrize("shift", (4, 7), ids=("P12", "P15"))
@pytest.mark.parametrize("size", ((64, 17), (31, 33), (33, 31), (32, 32)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_many_planes_small_blocks(encoder, size, shift):
    """8-bit noise with step 2^-(8 + shift): 8 + shift planes in blocks of at
    most 32 rows and just above."""
    w, h = size
    _, rc = tc.recipe_for("d", 8, 16.0, tile_w=w, tile_h=h)
    rc = dict(rc, qstep=2.0 ** -(8 + shift))
    case = dict(name=f"planes_P{8 + shift}_{w}x{h}", kind="d", bits=8, lossless=False, recipe=rc, tiles=[("noise", w, h)])
    _check(encoder, case, _image(dict(make=("noise", w, h, 8, tc.SEED + 950))))
