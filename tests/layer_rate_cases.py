"""Explicit per-layer rates (jp2hip_set_layer_rates): the cases the CPU and the
GPU suites share, and the rule of DESIGN.md 4 restated in Python.

The rule.  All arithmetic is integer.  For an image of W x H pixels encoded in
L layers by rates[l] (bits per pixel, layer 0 first):

    t[l] = max(0, floor(rates[l] * W * H / 8) - T - E)          the layer's target
    b[l] = max(0, t[l] - (16 * ntileparts + 256 + 16 * (npackets / L) * (l + 1)))

T and E are the bytes of the TLM marker segments and of the tile-part
divisions.  After a tier-2 sizing pass the code-stream through layer l is

    S[l] = fixed + part_bytes - sum over m > l of layer_bytes[m]

Iteration it = 0 .. 7:  clamp the budgets so that they never decrease with l
(from L - 2 down, b[l] = min(b[l], b[l + 1]));  select at the budgets;  size;
count the iteration;  halt when every targeted layer has S[l] <= t[l] or when
it = 7;  otherwise every layer that is over, by over = S[l] - t[l], has
b[l] -= (over << it) + (over >> 4) + 64, floored at 0.  A lossless top layer
has no target (-1 here) and the budget NO_BUDGET: it takes every coded pass.

run_model() is that loop over two callables, so the same text is driven by
random sizes on the CPU (against jp2hip_layer_rate_step) and on the GPU by
the oracle's hull segments and slope-driven encodes (test_gpu_layer_rates).
"""
from __future__ import annotations

import math

import numpy as np

import imaging as im
import jp2hip
import oracle_lib as ol
import pcrd_cases as pc
import slope_cases as sc

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY
NO_BUDGET = (1 << 63) - 1
NO_TARGET = -1


# ---- the rule ------------------------------------------------------------------------

def targets_of(rates, W, H, T, E, lossless_top):
    L = len(rates)
    t = [max(0, math.floor(r * W * H / 8) - T - E) for r in rates]
    if lossless_top:
        t[L - 1] = NO_TARGET
    return t


def first_budgets_of(t, ntileparts, npackets):
    L = len(t)
    return [NO_BUDGET if t[l] == NO_TARGET else max(0, t[l] - (16 * ntileparts + 256 + 16 * (npackets // L) * (l + 1)))
            for l in range(L)]


def clamp(b):
    b = list(b)
    for l in range(len(b) - 2, -1, -1):
        b[l] = min(b[l], b[l + 1])
    return b


def through_layers(fixed, part_bytes, layer_bytes):
    """S[l] of one sizing pass."""
    L = len(layer_bytes)
    return [fixed + part_bytes - sum(layer_bytes[l + 1:]) for l in range(L)]


def lower(it, S, t, b):
    """Step 6: the budgets after iteration `it` found the sizes S."""
    b = list(b)
    for l in range(len(b)):
        if t[l] != NO_TARGET and S[l] > t[l]:
            over = S[l] - t[l]
            b[l] = max(0, b[l] - ((over << it) + (over >> 4) + 64))
    return b


def fits(S, t):
    return all(t[l] == NO_TARGET or S[l] <= t[l] for l in range(len(t)))


def run_model(t, b0, select, size):
    """The loop.  select(budgets) -> thresholds; size(thresholds) -> S (a list
    per layer).  Returns dict(iterations, thresholds, S, trace): trace holds
    per iteration (budgets used, S, layers over)."""
    b, trace = list(b0), []
    for it in range(8):
        b = clamp(b)
        K = select(b)
        S = size(K)
        over = [l for l in range(len(t)) if t[l] != NO_TARGET and S[l] > t[l]]
        trace.append(dict(budgets=list(b), S=list(S), over=over))
        if not over or it == 7:
            break
        b = lower(it, S, t, b)
    return dict(iterations=len(trace), thresholds=K, S=S, trace=trace, fits=not over)


# ---- one layer: the oracle's cases -----------------------------------------------------

def one_layer_cases():
    """Every rate-driven one-layer case of pcrd_cases (the tie_* and *_ly1
    cases, both tier-2 routes) and, for the loop's last door, two one-layer
    cases whose target the headers alone pass: 8 iterations, over."""
    out = [c for c in pc.cases() if c["rate_driven"] and c["recipe"]["layers"] == 1]
    for route in pc.ROUTES:
        out.append(pc.make_case("rates", "noise_0.01bpp_ly1", "noise", route, False, layers=1, rate_bpp=0.01))
    return out


def oracle_iterations(case) -> int:
    return pc.measure(case)["export"]["iterations"]


# ---- many layers -------------------------------------------------------------------------
# images of at most 256 x 256, 64 x 64 tiles, 16 x 16 or 32 x 32 code-blocks

def _grey():
    return pc.image(dict(image="texture"))


def _rgb():
    return im.synth_rgb8(192, 256, seed=pc.SEED)


def _thin():
    return np.ascontiguousarray(im.synth_rgb8(256, 8, seed=7)[:, :1, 0])


T64 = dict(tile_w=64, tile_h=64, slope_skip=0, format=0)
C16 = dict(T64, levels=2, cblk_w_log2=4, cblk_h_log2=4, nprecincts=0, mct=0)
C32 = dict(T64, levels=3, cblk_w_log2=5, cblk_h_log2=5, nprecincts=0)

# name -> (image, conversion, recipe overrides, rates layer 0 first).  At these
# sizes the headers weigh: a grey C16 code-stream holds 1286 bytes before its
# first packet and 432 bytes of empty packets (SOP, a byte, EPH) per layer, an
# RGB C32 one 2072 and 1296 -- the rates leave room above that.
CASES = {
    "grey_ly3": (_grey, LY, dict(C16, layers=3), [0.75, 1.5, 3.0]),
    # (three -flush_period stripes, so a tile-split has work for three ranks)
    "rgb_ly6": (_rgb, LY, dict(C32, layers=6, flush_period=64), [0.8, 1.2, 1.8, 2.6, 3.6, 5.0]),
    "grey_ll6": (_grey, LL, dict(C16, layers=6), [0.3, 0.5, 0.8, 1.2, 2.0, 0.0]),
    "rgb_ll2": (_rgb, LL, dict(C32, layers=2), [2.0, 0.0]),
    # four -flush_period stripes: without rates the plan would have four rate-control groups
    "grey_ll6_stripes": (_grey, LL, dict(C16, layers=6, flush_period=64), [0.3, 0.6, 1.0, 1.5, 2.4, 0.0]),
    "grey_ll4_org": (_grey, LL, dict(C16, layers=4), [1.2, 2.0, 3.0, 0.0]),
    # two equal rates: the clamp holds layer 1's budget to layer 2's, and layer 2 adds nothing
    "grey_ly3_equal": (_grey, LY, dict(C16, layers=3), [0.3, 0.7, 0.7]),
    # precincts of 16 blocks (levels = 0): a packet that first includes them
    # has a header past the 16-byte estimate, so layer 0 is over at first; the
    # upper rates are above everything the image codes to, so layers 1 and 2
    # take every pass and fit
    "grey_ly3_low": (_grey, LY, dict(T64, levels=0, cblk_w_log2=4, cblk_h_log2=4, nprecincts=0, mct=0, layers=3),
                     [1.5, 8.0, 9.0]),
}
SLOPE_CASES = ("grey_ly3", "rgb_ly6", "grey_ll6", "rgb_ll2", "grey_ll6_stripes", "grey_ly3_equal", "grey_ly3_low")
LOWER_ONLY = "grey_ly3_low"     # two or more iterations, the top layer never over
CLAMPED = "grey_ly3_equal"
ROUTES = ("rgb_ly6", "grey_ll6_stripes")   # one lossy, one with a lossless top layer

EXTREMES = {
    # a target below the header estimate: the first layers are empty
    "below_estimate": (_grey, LY, dict(C16, layers=3), [0.001, 0.5, 1.0]),
    "ly32": (_grey, LY, dict(C16, layers=32), [0.4 + 0.15 * (l + 1) for l in range(32)]),
    "ly32_lossless": (_grey, LL, dict(C16, layers=32), [0.4 + 0.15 * (l + 1) for l in range(31)] + [0.0]),
    "all_equal": (_grey, LY, dict(C16, layers=4), [0.7] * 4),
    "thin": (_thin, LY, dict(C16, layers=3), [0.5, 1.0, 2.0]),
    "thin_lossless": (_thin, LL, dict(C16, layers=3), [0.5, 1.0, 0.0]),
}
ALL = dict(CASES, **EXTREMES)

_images = {}


def image(name) -> np.ndarray:
    if name not in _images:
        _images[name] = np.array(ALL[name][0](), order="C")   # (a copy: pcrd_cases keeps its own)
        _images[name].setflags(write=False)
    return _images[name]


def recipe(name, **more):
    _, conv, ov, _ = ALL[name]
    return conv, jp2hip.recipe(conv, **dict(ov, **more))


def rates(name):
    return list(ALL[name][3])


def geometry(name):
    a = image(name)
    return a.shape[1], a.shape[0], (1 if a.ndim == 2 else a.shape[2]), a.dtype.itemsize * 8


def tiff_of(name) -> bytes:
    return im.tiff_bytes(image(name), rows_per_strip=16)


def plan_numbers(name, letters=0, tlm=0, **more):
    """(t, b, info) by the library's host-only entry, checked against the rule
    restated above."""
    W, H, nc, bits = geometry(name)
    conv, rc = recipe(name, **more)
    t, b, info = jp2hip._lib.layer_rate_targets(W, H, nc, bits, rc, rates(name), letters, tlm)
    mine = targets_of(rates(name), W, H, info["T"], info["E"], rc.rate_bpp <= 0.0)
    assert t == mine, (name, t, mine)
    assert b == clamp(first_budgets_of(mine, info["ntileparts"], info["npackets"])), (name, b)
    return t, b, info


_segments = {}


def hull_segments(name):
    """(keys descending, inclusive byte sums) of every hull segment of the
    image, all rate-control groups merged: the oracle's export of an encode
    that coded every plane (the segments do not depend on the rate)."""
    if name not in _segments:
        conv, rc = recipe(name)
        orc = ol.copy_recipe(rc)
        orc.slope_skip = 0
        if conv == LY:
            orc.rate_bpp = max(rates(name))
        ol.pcrd_export_enable(True)
        try:
            ol.encode(image(name), orc)
            ex = ol.pcrd_export()
        finally:
            ol.pcrd_export_enable(False)
        segs = sorted(((k, n) for k, n, _, _ in ex["segments"]), key=lambda s: -s[0])
        keys = np.array([k for k, _ in segs], np.uint64)
        cum = np.cumsum(np.array([n for _, n in segs], np.int64))
        _segments[name] = (keys, cum)
    return _segments[name]


def select_on_segments(name):
    """select() of run_model: jp2hip.split.thresholds over hull_segments."""
    from jp2hip import split as js
    keys, cum = hull_segments(name)
    return lambda budgets: [int(k) for k in js.thresholds(keys, cum, np.array(budgets, np.int64))]


def slopes_of(keys, lossless_top):
    s = [sc.key_to_slope(k) for k in keys]
    if lossless_top:
        s[-1] = 0.0
    return s
