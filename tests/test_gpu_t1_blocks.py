"""GPU parity on the crafted tier-1 corpus (tests/t1_block_cases.py): every
case encoded by libjp2hip through the C ABI and byte-compared with the CPU
oracle.  tests/test_t1_blocks.py shows on the CPU what the corpus reaches:
every zero-coding neighbourhood, sign-coding configuration, run-length
outcome, MQ table state and byte-out / flush branch a block can reach, the
largest bit-plane and the longest propagation chain a 64x64 block can hold,
and every small block size.

One block per tile: a mismatch is reported by the first tile whose tile-part
differs -- the pattern's name and size -- and by whether the packet header
(pass counts and truncation lengths) or the body (the MQ stream) parts first.
"""
import numpy as np
import pytest

import imaging as im
import jp2hip
import oracle_lib as ol
import t1_block_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_block_corpus_identical_to_oracle(encoder, case):
    img = tc.image(case)
    conv = jp2hip.LOSSLESS if case["lossless"] else jp2hip.LOSSY
    rc = jp2hip.recipe(conv, **case["recipe"])
    got, _ = encoder.encode_tiff(im.tiff_bytes(img), conv, rc)
    want = ol.encode(img, ol.copy_recipe(rc))
    if got != want:
        raise AssertionError(tc.describe_mismatch(case, got, want))
    if case["kind"] == "a":
        assert np.array_equal(im.decode_opj(got, ".j2k").reshape(img.shape), img)
