"""GPU parity on the crafted PCRD / rate-loop corpus (tests/pcrd_cases.py):
every case encoded by libjp2hip and byte-compared with the CPU oracle, its
rate iterations compared with the oracle's count.  tests/test_pcrd.py shows on
the CPU which paths the corpus takes: every branch of the hull, tie groups of
1, up to and above kSelBrute segments at the threshold with budgets that end
on them, miss them and pass them by one byte, no narrowing round, one and
several, the one-key exit, budgets that take nothing and everything, every
iteration count of the rate loop from 1 to 8, the safety net of slope
prediction, flush stripes without a byte -- each on precincts of one block
(k_t2_wave assigns the layers) and of 128 (k_apply does).

A subset also goes through the tile-split encode (its selection is a host-side
exchange over sorted segments: it has to agree with k_select on ties), and one
context encodes an ordinary case after each case that leaves the rate loop by
an unusual door.
"""
import threading

import pytest

import imaging as im
import jp2hip
import oracle_lib as ol
import pcrd_cases as pc
from jp2hip import split as js

pytestmark = pytest.mark.gpu

CASES = pc.cases()
_WANT = {}


def conv_of(case):
    return jp2hip.LOSSLESS if case["lossless"] else jp2hip.LOSSY


def tiff_of(case) -> bytes:
    return im.tiff_bytes(pc.image(case), rows_per_strip=16)


def want(case):
    """(the oracle's file, its rate iterations), once per case."""
    if case["name"] not in _WANT:
        rc = jp2hip.recipe(conv_of(case), **case["recipe"])
        data = ol.encode(pc.image(case), ol.copy_recipe(rc))
        _WANT[case["name"]] = (data, ol.lib().oracle_pcrd_export_iterations())
    return _WANT[case["name"]]


def check(case, got, stats=None):
    data, iters = want(case)
    if bytes(got) != data:
        raise AssertionError(pc.describe_mismatch(case, bytes(got), data))
    if stats is not None and case["rate_driven"]:
        assert stats.rate_iterations == iters, (case["name"], stats.rate_iterations, iters)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_corpus_identical_to_oracle(encoder, case):
    got, st = encoder.encode_tiff(tiff_of(case), conv_of(case), jp2hip.recipe(conv_of(case), **case["recipe"]))
    check(case, got, st)


@pytest.mark.parametrize("name", pc.SPLIT)
def test_tile_split_world_2_identical_to_single_gpu_and_oracle(encoder, name):
    from devmem import DeviceBytes
    case = pc.by_name(name)
    conv, tif = conv_of(case), tiff_of(case)
    rc = jp2hip.recipe(conv, **case["recipe"])
    lay, offs = jp2hip.tiff_layout(tif)
    world = 2
    g = js.ThreadGroup(world)
    parts, errs = [None] * world, []

    def work(r):
        try:
            enc = jp2hip.Encoder(0)
            try:
                r0, r1 = js.split_rows(lay.height, rc.tile_h, r, world, rc.flush_period)
                assert r1 > r0
                buf, blay, keep = js.band_strips(tif, lay, offs, r0, r1)
                d = DeviceBytes(buf or b"\0")
                try:
                    parts[r] = enc.encode_device_split(d.ptr, d.nbytes, blay, conv, g.member(r).split(), rc)
                finally:
                    d.free()
            finally:
                enc.close()
        except Exception as e:  # keep the other rank from waiting forever
            errs.append(e)
            g.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    if errs:
        raise errs[0]
    assert parts[0][1] == 0 and parts[1][1] == len(parts[0][0])
    split_file = parts[0][0] + parts[1][0]
    single, st = encoder.encode_tiff(tif, conv, rc)
    check(case, single, st)
    check(case, split_file)
    assert split_file == single
    if case["rate_driven"]:
        assert parts[0][3].rate_iterations == parts[1][3].rate_iterations == want(case)[1]


def _refused(encoder):
    """A recipe build_plan refuses (a band of more than 30 magnitude
    bit-planes), after the context has begun the encode."""
    case = pc.by_name("extremes_deep_b30000_p128")
    rc = jp2hip.recipe(jp2hip.LOSSY, **dict(case["recipe"], qstep=2.0 ** -31, guard_bits=2))
    with pytest.raises(jp2hip.Jp2hipError):
        encoder.encode_tiff(tiff_of(case), jp2hip.LOSSY, rc)


@pytest.mark.parametrize("second", pc.PAIR_SECOND)
@pytest.mark.parametrize("first", pc.PAIR_FIRST + ("refused",))
def test_one_context_ordinary_case_after_an_unusual_one(encoder, first, second):
    """The list-fill counters are left zero and the rate state is rewritten:
    whatever the encode before did, the next one is the oracle's file."""
    if first == "refused":
        _refused(encoder)
    else:
        a = pc.by_name(first)
        got, st = encoder.encode_tiff(tiff_of(a), conv_of(a), jp2hip.recipe(conv_of(a), **a["recipe"]))
        check(a, got, st)
    b = pc.by_name(second)
    got, st = encoder.encode_tiff(tiff_of(b), conv_of(b), jp2hip.recipe(conv_of(b), **b["recipe"]))
    check(b, got, st)
