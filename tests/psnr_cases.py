"""Model and corpus for quality layers by target PSNR (jp2hip_set_layer_psnr),
shared by tests/test_layer_psnr.py (CPU) and tests/test_gpu_layer_psnr.py.

Nothing of the product is imported here.  The model works on the oracle's
PCRD export (oracle_lib.pcrd_export of an oracle encode that codes every
pass): each hull segment's distortion quantum by the rule of
jp2hip_distortion_quantum, written in numpy, and the threshold the rule of
pcrd.hip's k_select<true> arrives at for integer targets:

    need = total quanta - target         (target < 0: total + 1)
    need <= 0        nothing is taken: K = largest key + 1 (0 without segments)
    else             K = the largest key whose quanta, summed with those of
                     every larger key, reach need; 0 when none does

The corpus is built from the crafted 16 x 16-block images of
tests/pcrd_cases.py (256 blocks, levels = 0, one component: every block has
the same weight).  A "tie" case aims five layers at one tie group G of the
sorted segments, whose quanta lie in (lower, upper] of the running sum from
the top: need = lower - 1, lower, lower + 1, upper, upper + 1 -- which must
give the key before G twice, G's key twice, and the key after G.  Layers 0
and 1 then share a threshold: an empty layer.  CENSUS_CELLS names what the
corpus must reach; census() computes it from the model alone.
"""
from __future__ import annotations

import struct

import numpy as np

import oracle_lib as ol
import pcrd_cases as pc

POSITIONS = ("below_lower", "on_lower", "above_lower", "on_upper", "above_upper")
SIZES = ("tie_1", "tie_2_64", "tie_gt64")
CENSUS_CELLS = tuple(f"{s}_{p}" for s in SIZES for p in POSITIONS) + (
    "tie_blocks_differ", "nothing_reaches_K0", "everything_meets_nothing_taken", "same_threshold_empty_layer",
    "layers_1", "layers_32", "lossless_top_layer", "bits_8", "bits_16")


# --------------------------------------------------------------------------
# the quantum rule and the selection, in numpy / Python integers
# --------------------------------------------------------------------------
def quantum_shift(bits: int) -> int:
    return 2 * (bits - 8) - 8


def quantum(weight, dd, bits: int) -> np.ndarray:
    """floor((weight * float64(dd)) * 2^-s + 0.5), saturated at 2^63 - 1; 0
    where the product is not positive.  weight: float64, dd: int64 (arrays)."""
    w = np.asarray(weight, np.float64)
    d = np.asarray(dd, np.int64).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = w * d
        v = p * np.float64(2.0) ** np.float64(-quantum_shift(bits))
        r = v + np.float64(0.5)
    out = np.zeros(np.broadcast(w, d).shape, np.int64)
    pos = p > 0
    big = pos & ((v >= 2.0 ** 63) | (r >= 2.0 ** 63))
    ok = pos & ~big
    out[ok] = np.floor(r[ok]).astype(np.int64)
    out[big] = np.iinfo(np.int64).max
    return out


def key_of(slope: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", slope))[0]


def segments(export, bits: int):
    """[(key, quanta, block)] of an export, sorted by key descending (block
    order within a key): every hull segment with its quantum."""
    out = []
    for b, blk in enumerate(export["blocks"]):
        hull, dd = blk["hull"], blk["dd"]
        for i in range(1, len(hull)):
            d = sum(dd[hull[i - 1]:hull[i]])
            q = int(quantum(blk["weight"], d, bits))
            out.append((key_of(blk["hslope"][i]), q, b))
    out.sort(key=lambda s: (-s[0], s[2]))
    assert sorted(k for k, _, _ in out) == sorted(k for k, _, _, _ in export["segments"])
    return out


def groups_of(segs):
    """Tie groups of sorted segments: [dict(key, count, quanta, blocks, lower, upper)]."""
    out, cum = [], 0
    for key, q, b in segs:
        if out and out[-1]["key"] == key:
            g = out[-1]
            g["count"] += 1
            g["quanta"] += q
            g["blocks"].add(b)
        else:
            out.append(dict(key=key, count=1, quanta=q, blocks={b}, lower=cum))
        cum += q
        out[-1]["upper"] = cum
    return out


def thresholds(segs, targets):
    """The model's K[l] for integer targets (quanta each layer may leave)."""
    groups = groups_of(segs)
    total = groups[-1]["upper"] if groups else 0
    K = []
    for t in targets:
        need = total + 1 if t < 0 else total - t
        if need <= 0:
            K.append(groups[0]["key"] + 1 if groups else 0)
            continue
        K.append(next((g["key"] for g in groups if g["upper"] >= need), 0))
    return K


def find_psnr(target_fn, want: int, lo: float = 1e-3, hi: float = 400.0) -> float:
    """A PSNR (dB) whose integer target -- target_fn(psnr), non-increasing in
    psnr: jp2hip_layer_psnr_targets for the image -- is exactly `want`."""
    assert target_fn(lo) >= want >= target_fn(hi), (want, target_fn(lo), target_fn(hi))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        t = target_fn(mid)
        if t == want:
            return mid
        if t > want:
            lo = mid
        else:
            hi = mid
    raise AssertionError(f"no PSNR has the target {want}")


# --------------------------------------------------------------------------
# the corpus
# --------------------------------------------------------------------------
def _case(name, img, route, lossless, layers, kind, **extra):
    rc = dict(pc.BASE, **pc.ROUTES[route], layers=layers)
    bits = pc.IMAGES[img][0]
    if lossless:
        rc["rate_bpp"] = 0.0
    else:
        rc["qstep"] = 2.0 ** -bits
        rc["rate_bpp"] = 1.0   # (no target under PSNR targets: "not lossless")
    return dict(name=name, image=img, route=route, lossless=lossless, bits=bits, recipe=rc, kind=kind, **extra)


def cases():
    out = [
        # five layers around one tie group: `size` picks the group (its count
        # within the bounds), `nth` which of those from the top
        _case("tie1_noise_p1", "noise", "p1", False, 5, "tie", size=(1, 1), nth=40),
        _case("tie60_p128", "tie60", "p128", False, 5, "tie", size=(2, 64), nth=3),
        _case("tie65_p1", "tie65", "p1", False, 5, "tie", size=(65, 256), nth=2),
        _case("tie190_p128", "tie190", "p128", False, 5, "tie", size=(65, 256), nth=5),
        _case("tie100mix_p128", "tie100mix", "p128", False, 5, "tie", size=(2, 256), nth=4),
        _case("tie16bit_p1", "nearties16", "p1", False, 5, "tie", size=(1, 1), nth=300),
        # a target everything meets, one in the middle, one that takes it all
        _case("extremes_noise_p128", "noise", "p128", False, 3, "extremes"),
        # lossless recipe: nothing, the middle, the top layer of every pass (K = 0)
        _case("lossless_top_p128", "tie100mix", "p128", True, 3, "lossless"),
        _case("lossless_top_16bit_p1", "nearties16", "p1", True, 2, "lossless"),
        _case("layers1_texture_p1", "texture", "p1", False, 1, "spread"),
        _case("layers32_texture_p128", "texture", "p128", False, 32, "spread"),
    ]
    assert len({c["name"] for c in out}) == len(out)
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def image(c):
    return pc.image(c)


_MEASURED = {}


def measure(c) -> dict:
    """The oracle encode of the case's recipe that codes every pass (a budget
    nothing exceeds / lossless), its export and the sorted segments with their
    quanta."""
    if c["name"] not in _MEASURED:
        rc = dict(c["recipe"])
        if not c["lossless"]:
            rc["rate_bpp"] = 64.0
        ol.pcrd_export_enable(True)
        try:
            data = ol.encode(image(c), ol.recipe(c["lossless"], **rc))
            exp = ol.pcrd_export()
        finally:
            ol.pcrd_export_enable(False)
        assert len({g for _, _, _, g in exp["segments"]}) <= 1 or c["lossless"]
        _MEASURED[c["name"]] = dict(file=data, export=exp, segs=segments(exp, c["bits"]))
    return _MEASURED[c["name"]]


def wanted(c):
    """(integer targets, expected K, cells) of a case, by the model alone."""
    segs = measure(c)["segs"]
    groups = groups_of(segs)
    total = groups[-1]["upper"]
    L = c["recipe"]["layers"]
    cells = {f"bits_{c['bits']}"}
    if c["kind"] == "tie":
        lo, hi = c["size"]
        # (the group before must hold 2 quanta or more, or need = lower - 1
        # falls on the group before that one)
        fit = [i for i, g in enumerate(groups) if lo <= g["count"] <= hi and 0 < i < len(groups) - 1 and
               groups[i - 1]["quanta"] >= 2 and g["quanta"] >= 2]
        i = fit[min(c["nth"], len(fit) - 1)]
        g = groups[i]
        needs = [g["lower"] - 1, g["lower"], g["lower"] + 1, g["upper"], g["upper"] + 1]
        targets = [total - n for n in needs]
        want = [groups[i - 1]["key"]] * 2 + [g["key"]] * 2 + [groups[i + 1]["key"]]
        size = "tie_1" if g["count"] == 1 else ("tie_2_64" if g["count"] <= 64 else "tie_gt64")
        cells |= {f"{size}_{p}" for p in POSITIONS} | {"same_threshold_empty_layer"}
        if len(g["blocks"]) > 1:
            cells.add("tie_blocks_differ")
    elif c["kind"] == "extremes":
        targets = [total + 5, total // 3, 0]
        want = [groups[0]["key"] + 1, None, None]
        cells.add("everything_meets_nothing_taken")
    elif c["kind"] == "lossless":
        targets = [total, total // 2, -1][3 - L:]
        want = [groups[0]["key"] + 1, None, 0][3 - L:]
        cells |= {"everything_meets_nothing_taken", "nothing_reaches_K0", "lossless_top_layer"} if L == 3 else \
            {"nothing_reaches_K0", "lossless_top_layer"}
    else:
        targets = [total - (total * (l + 1)) // (L + 1) for l in range(L)]
        want = [None] * L
        cells.add(f"layers_{L}")
    K = thresholds(segs, targets)
    for l, w in enumerate(want):
        assert w is None or K[l] == w, (c["name"], l, K[l], w)
    assert all(K[l] <= K[l - 1] for l in range(1, L)), c["name"]
    return targets, K, cells


def census() -> dict:
    """CENSUS_CELLS -> the cases that reach each, by the model alone."""
    out = {k: [] for k in CENSUS_CELLS}
    for c in cases():
        for cell in wanted(c)[2]:
            out[cell].append(c["name"])
    return out


def slope_of(key: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", key))[0]


def cum_by_rank(segs, world: int, rank: int):
    """A rank's share of sorted segments (block b belongs to rank b % world):
    (keys descending, inclusive quanta sums) as jp2hip_split_psnr_thresholds reads them."""
    mine = [(k, q) for k, q, b in segs if b % world == rank]
    keys = np.array([k for k, _ in mine], np.uint64)
    cum = np.cumsum(np.array([q for _, q in mine], np.int64)) if mine else np.zeros(0, np.int64)
    return keys, cum
