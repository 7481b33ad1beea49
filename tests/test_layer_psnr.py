"""Quality layers by target PSNR (jp2hip_set_layer_psnr): what needs no GPU.
The quantum rule against numpy bit for bit, the dB -> quanta conversion, every
refusal by message, the three-way exclusivity with slopes and rates, the
tile-split exchange against the model of tests/psnr_cases.py over Python
groups, the corpus' census, and the new prototypes against the header.
"""
import ctypes
import itertools
import math
import os
import re
import threading

import numpy as np
import pytest

import jp2hip
import psnr_cases as pq
from jp2hip import _lib
from jp2hip import split as js

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the quantum ------------------------------------------------------------------------

def _draws():
    r = np.random.default_rng(20261021)
    w = np.concatenate([2.0 ** r.uniform(-60, 60, 4000), [0.25, 1.0, 2.0 ** -1022, 2.0 ** 1023, 1e-300, 1e300, 0.0]])
    d = np.concatenate([r.integers(1, 2 ** 62, 1000), 2 ** r.integers(0, 63, 1000) + r.integers(-3, 4, 1000),
                        r.integers(2 ** 53, 2 ** 63 - 1, 1000), r.integers(-2 ** 40, 2 ** 20, 1000),
                        [0, 1, -1, 2 ** 53 + 1, 2 ** 63 - 1, -2 ** 63]]).astype(np.int64)
    n = max(len(w), len(d))
    return np.resize(w, n), np.resize(d, n)


@pytest.mark.parametrize("bits", [1, 8, 12, 16])
def test_quantum_equals_the_numpy_rule_bit_for_bit(bits):
    w, d = _draws()
    want = pq.quantum(w, d, bits)
    got = np.array([jp2hip.distortion_quantum(float(a), int(b), bits) for a, b in zip(w, d)], np.int64)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bits, [(w[i], d[i], got[i], want[i]) for i in bad[:5]])
    assert (want > 0).sum() > 1000 and (want == np.iinfo(np.int64).max).any() and (want == 0).any()


def test_quantum_small_values_and_the_shift():
    assert pq.quantum_shift(8) == -8 and pq.quantum_shift(16) == 8
    assert jp2hip.distortion_quantum(0.25, 4, 8) == 256          # one squared level = 256 quanta at 8 bits
    assert jp2hip.distortion_quantum(0.25, 4 << 16, 16) == 256   # ... and of the 16-bit range's share
    assert jp2hip.distortion_quantum(1.0, 1, 16) == 0 and jp2hip.distortion_quantum(1.0, 128, 16) == 1
    assert jp2hip.distortion_quantum(-1.0, 5, 8) == 0 and jp2hip.distortion_quantum(float("nan"), 5, 8) == 0
    # the library's own refusal and message, through the wrapper and directly
    with pytest.raises(jp2hip.Jp2hipError, match=r"distortion quantum: bits = 17 is outside 1 \.\. 16"):
        jp2hip.distortion_quantum(1.0, 1, 17)
    assert _lib.lib().jp2hip_distortion_quantum(1.0, 1, 0) < 0 and "bits = 0" in _lib.last_error()


# ---- dB -> quanta -------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,nc,bits", [(256, 256, 1, 8), (64, 64, 1, 16), (4001, 3003, 3, 8), (30000, 30000, 3, 16)])
def test_targets_agree_with_python_and_are_monotone(w, h, nc, bits):
    ps = [0.5 + 0.37 * i for i in range(300)]
    got = [jp2hip.layer_psnr_targets(w, h, nc, bits, [p])[0] for p in ps]
    peak = (1 << bits) - 1
    for p, g in zip(ps, got):
        want = peak * peak * w * h * nc * 2.0 ** -pq.quantum_shift(bits) / 10.0 ** (p / 10.0)
        assert abs(g - want) <= max(1.0, want * 2.0 ** -40), (p, g, want)
    assert all(a >= b for a, b in zip(got, got[1:]))
    # exactly monotone also between neighbouring doubles
    p = 38.0
    near = [p]
    for _ in range(200):
        near.append(math.nextafter(near[-1], math.inf))
    t = jp2hip.layer_psnr_targets(w, h, nc, bits, near[:32]) + [jp2hip.layer_psnr_targets(w, h, nc, bits, [x])[0]
                                                               for x in near[32:]]
    assert all(a >= b for a, b in zip(t, t[1:]))


def test_targets_lossless_top_and_refusals():
    assert jp2hip.layer_psnr_targets(16, 16, 1, 8, [30.0, 0.0])[1] == -1
    assert jp2hip.layer_psnr_targets(16, 16, 1, 8, [0.0]) == [-1]
    with pytest.raises(jp2hip.Jp2hipError, match="geometry"):
        jp2hip.layer_psnr_targets(0, 16, 1, 8, [30.0])
    with pytest.raises(jp2hip.Jp2hipError, match=r"psnr_db\[1\] decreases"):
        jp2hip.layer_psnr_targets(16, 16, 1, 8, [30.0, 20.0])


def test_find_psnr_hits_every_neighbouring_integer():
    fn = lambda p: jp2hip.layer_psnr_targets(256, 256, 1, 8, [p])[0]
    base = fn(41.0)
    for want in range(base - 3, base + 4):
        assert fn(pq.find_psnr(fn, want)) == want


# ---- the overflow bound ---------------------------------------------------------------------

def test_the_overflow_bound_accepts_large_scans_and_refuses_past_it():
    """jp2hip_layer_psnr_fits, the check the encodes make: the default
    recipes take a 40 000 x 30 000 grey 16-bit scan and 20 000 x 20 000 RGB,
    and refuse 30 000 x 30 000 RGB (2.7 * 10^9 samples) -- the bound, not a
    real overflow (jp2hip.h states it)."""
    for conv in (jp2hip.LOSSY, jp2hip.LOSSLESS):
        rc = jp2hip.recipe(conv)
        assert jp2hip.layer_psnr_fits(40000, 30000, 1, 16, rc)
        assert jp2hip.layer_psnr_fits(20000, 20000, 3, 8, rc)
        assert not jp2hip.layer_psnr_fits(30000, 30000, 3, 8, rc)
    with pytest.raises(jp2hip.Jp2hipError, match="levels"):
        jp2hip.layer_psnr_fits(64, 64, 1, 8, jp2hip.recipe(jp2hip.LOSSY, levels=40))


# ---- refusals -----------------------------------------------------------------------------

REFUSALS = [
    ([float("nan")], None, r"psnr_db\[0\] is NaN"),
    ([30.0, float("inf")], None, r"psnr_db\[1\] is infinite"),
    ([30.0, -1.0], None, r"psnr_db\[1\] = -1.* is negative"),
    ([-0.0], None, r"psnr_db\[0\] .* is negative"),
    ([30.0, 40.0, 35.0], None, r"psnr_db\[2\] decreases from psnr_db\[1\]"),
    ([30.0, 0.0, 0.0], None, r"psnr_db\[1\] decreases"),
    ([30.0] * 33, None, r"n = 33 is outside 0 \.\. 32"),
    ([30.0, 40.0], dict(conv=jp2hip.LOSSY, layers=3), r"n = 2 targets .*layers = 3"),
    ([30.0, 40.0], dict(conv=jp2hip.LOSSLESS, layers=2), r"psnr_db\[1\], the last, must be 0 with rate_bpp <= 0"),
    ([30.0, 0.0], dict(conv=jp2hip.LOSSY, layers=2), r"psnr_db\[1\] is 0 with rate_bpp > 0"),
]


@pytest.mark.parametrize("targets,rc,msg", REFUSALS)
def test_check_refuses_by_message(targets, rc, msg):
    rcp = jp2hip.recipe(rc["conv"], layers=rc["layers"]) if rc else None
    with pytest.raises(jp2hip.Jp2hipError, match=msg):
        jp2hip.check_layer_psnr(targets, rcp)


def test_check_accepts():
    jp2hip.check_layer_psnr([30.0, 30.0, 44.5])
    jp2hip.check_layer_psnr([30.0, 40.0, 0.0])            # a last 0 is no decrease
    jp2hip.check_layer_psnr(None)
    jp2hip.check_layer_psnr([30.0, 0.0], jp2hip.recipe(jp2hip.LOSSLESS, layers=2))
    jp2hip.check_layer_psnr([30.0, 40.0], jp2hip.recipe(jp2hip.LOSSY, layers=2))
    assert _lib.lib().jp2hip_check_layer_psnr(None, -1, None) != 0 and "n = -1" in _lib.last_error()


# ---- the ABI ------------------------------------------------------------------------------

C_TYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
NEW = ("jp2hip_set_layer_psnr", "jp2hip_check_layer_psnr", "jp2hip_distortion_quantum", "jp2hip_layer_psnr_targets",
       "jp2hip_split_psnr_thresholds", "jp2hip_batch_set_layer_psnr", "jp2hip_layer_psnr_fits")


def _ctype(text):
    text = text.replace("const", "").strip()
    ptr = text.count("*")
    base = text.replace("*", "").split()
    base = base[0] if base[0] != "struct" else base[1]
    if ptr:
        if base in ("jp2hip_ctx", "jp2hip_batch"):
            return ctypes.c_void_p
        if base == "jp2hip_recipe":
            return ctypes.POINTER(_lib.Recipe)
        if base == "jp2hip_split":
            return ctypes.POINTER(_lib.Split)
        return ctypes.POINTER({"uint64_t": ctypes.c_uint64, **C_TYPES}[base])
    return C_TYPES[base]


@pytest.mark.parametrize("name", NEW)
def test_prototype_matches_the_header(name):
    with open(os.path.join(ROOT, "include", "jp2hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    args = [_ctype(a) for a in m.group(2).split(",")]
    fn = getattr(_lib.lib(), name)
    assert list(fn.argtypes) == args, (name, fn.argtypes, args)
    assert fn.restype == C_TYPES[m.group(1)], (name, fn.restype)


# ---- the split exchange against the model --------------------------------------------------

def _exchange(segs, targets, world):
    if world == 1:
        keys, cum = pq.cum_by_rank(segs, 1, 0)
        return [list(js.psnr_thresholds(keys, cum, targets))]
    g = js.ThreadGroup(world)
    out, errs = [None] * world, []

    def work(r):
        try:
            keys, cum = pq.cum_by_rank(segs, world, r)
            out[r] = list(js.psnr_thresholds(keys, cum, targets, g.member(r)))
        except Exception as e:
            errs.append(e)
            g.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not errs, errs
    return out


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("name", ["tie60_p128", "tie65_p1", "tie1_noise_p1", "lossless_top_p128", "extremes_noise_p128"])
def test_split_exchange_equals_the_model(name, world):
    c = pq.by_name(name)
    targets, K, _ = pq.wanted(c)
    for got in _exchange(pq.measure(c)["segs"], targets, world):
        assert [int(k) for k in got] == K


def test_split_exchange_ranks_without_segments():
    """Segments on one rank of three only (blocks 0, 3, 6, ...), and none anywhere."""
    c = pq.by_name("tie60_p128")
    segs = [s for s in pq.measure(c)["segs"] if s[2] % 3 == 0]
    total = sum(q for _, q, _ in segs)
    targets = [total + 1, total, total - 1, total // 2, 1, 0, -1]
    want = pq.thresholds(segs, targets)
    assert want[0] == want[1] == segs[0][0] + 1 and want[2] == segs[0][0] and want[-1] == 0
    for got in _exchange(segs, targets, 3):
        assert [int(k) for k in got] == want
    for got in _exchange([], [5, 0, -1], 2):
        assert [int(k) for k in got] == [0, 0, 0]


# ---- exclusivity (a context needs a GPU: the host-side order is tested on the device too) ----

def test_exclusivity_messages_name_the_other_setter():
    """The setters' refusals, read from the sources' own text: each names the
    setter that holds the context (the GPU test drives every order)."""
    with open(os.path.join(ROOT, "jp2-bucketeer_amd", "csrc", "api.cpp")) as f:
        api = f.read()
    for mine, others in (("slopes", ("jp2hip_set_layer_rates", "jp2hip_set_layer_psnr")),
                         ("rates", ("jp2hip_set_layer_slopes", "jp2hip_set_layer_psnr")),
                         ("psnr", ("jp2hip_set_layer_slopes", "jp2hip_set_layer_rates"))):
        for o in others:
            assert re.search(r'fail\("layer ' + mine + r": [^\"]*\(" + o + r"\); turn them off first", api), (mine, o)


# ---- the census -----------------------------------------------------------------------------

def test_every_census_cell_is_reached_by_the_model():
    cen = pq.census()
    empty = [k for k in pq.CENSUS_CELLS if not cen[k]]
    print({k: v for k, v in cen.items()})
    assert not empty, empty
