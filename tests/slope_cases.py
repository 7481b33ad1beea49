"""Fixed-slope quality layers (jp2hip_set_layer_slopes): the cases the CPU and
the GPU suites share, each with an expectation built from the oracle alone.

The oracle has no slope-driven mode, but its export (oracle_pcrd_export_layers)
returns the thresholds of its final selection: per rate-control group and
layer, K (the smallest key taken) and Kc (one above the first key not taken --
what Kdu-Layer-Info prints).  Any threshold in [Kc, K] selects the same passes,
so a slope-driven encode at slopes = Kc must write the oracle's file byte for
byte, COM included.  expectation() therefore encodes the case's recipe on the
oracle with slope_skip = 0 (a slope-driven encode codes every plane) and the
export on, and keeps the file, Kc and K per layer, and the distortion each
layer leaves by the report's definition:

    D[l] = sum over blocks b of  weight_b * sum over passes p >= nl_b(l) of dd_b[p]

The preconditions the construction needs are asserted here, before use: Kc
does not increase over the layers, and the rate-control groups of a
multi-group case agree on it.
"""
from __future__ import annotations

import math
import struct

import numpy as np

import imaging as im
import jp2hip
import oracle_lib as ol
import tlm_cases as tc

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY
INF_KEY = 0x7FF0000000000000


def key_to_slope(key: int) -> float:
    """The threshold whose bit pattern is `key`; +inf for what is no finite double."""
    return math.inf if key >= INF_KEY else struct.unpack("<d", struct.pack("<Q", key))[0]


def _rgb():
    return im.synth_rgb8(384, 512, seed=20261021)


def _grey(h=256, w=256, seed=5):
    return np.ascontiguousarray(im.synth_rgb8(h, w, seed=seed)[..., 0])


def _stripes():
    """256 wide, 512 high, grey: a 128-row band four times, so the four
    -flush_period 128 stripes (two rows of 64 x 64 tiles each) hold the same
    pixels and their rate-control groups choose the same thresholds."""
    band = _grey(128, 256, seed=9)
    return np.ascontiguousarray(np.concatenate([band] * 4, axis=0))


# levels = 0 and 16 x 16 blocks on 256 x 128 tiles: one precinct of 128 blocks a tile (k_apply)
P128 = dict(levels=0, mct=0, cblk_w_log2=4, cblk_h_log2=4, nprecincts=0, tile_w=256, tile_h=128, format=0)
SMALL = dict(tile_w=256, tile_h=256, levels=3)

# name -> (image builder, conversion, recipe overrides)
CASES = {}
for _rate in (0.3, 2.0, 8.0):
    for _layers in (1, 6, 12):
        CASES[f"rgb_{_rate}bpp_{_layers}ly"] = (_rgb, LY, dict(SMALL, rate_bpp=_rate, layers=_layers))
CASES.update({
    "grey16_2bpp": (lambda: im.synth_u16(150, 200, comps=1, seed=20261023), LY, dict(SMALL, rate_bpp=2.0)),
    # (two -flush_period stripes: a tile-split over two ranks has work for both)
    "p128_1bpp": (_grey, LY, dict(P128, rate_bpp=1.0, qstep=1.0 / 256.0, flush_period=128)),
    "p128_lossless": (_grey, LL, dict(P128)),
    "lossless_one_group": (_rgb, LL, dict(SMALL)),
    "lossless_four_groups": (_stripes, LL, dict(tile_w=64, tile_h=64, levels=2, flush_period=128, mct=0)),
    "default_recipe": (_rgb, LL, dict()),
    "lossless_lrcp": (_rgb, LL, dict(SMALL, progression=0, tparts_r=0)),
    "slope_skip_1": (_rgb, LY, dict(SMALL, rate_bpp=2.0, slope_skip=1)),
    # the report's exact case: levels = 0, so the transform is orthogonal
    "levels0": (lambda: np.ascontiguousarray(im.synth_rgb8(192, 256, seed=5)[..., 0]), LL,
                dict(levels=0, mct=0, tile_w=64, tile_h=64, layers=6)),
    "levels3": (lambda: np.ascontiguousarray(im.synth_rgb8(192, 256, seed=5)[..., 0]), LL,
                dict(levels=3, mct=0, tile_w=64, tile_h=64, layers=6)),
})
NOTHING_TAKEN = "rgb_0.3bpp_12ly"   # all twelve layers take nothing; rgb_2.0bpp_12ly: the first two
MULTI_GROUP = ("lossless_four_groups",)

_images, _expect = {}, {}


def image(name) -> np.ndarray:
    if name not in _images:
        _images[name] = CASES[name][0]()
        _images[name].setflags(write=False)
    return _images[name]


def recipe(name):
    """The recipe the library is given (slope_skip as the case states it)."""
    _, conv, ov = CASES[name]
    return conv, jp2hip.recipe(conv, **dict(dict(slope_skip=0), **ov))


def layers_of(export, L):
    """Kc and K per layer from an export: [group][layer] tables of keys."""
    groups = sorted({r["group"] for r in export["layers"]})
    kc = [[None] * L for _ in groups]
    k = [[None] * L for _ in groups]
    for r in export["layers"]:
        kc[groups.index(r["group"])][r["layer"]] = r["Kc"]
        k[groups.index(r["group"])][r["layer"]] = r["K"]
    assert all(x is not None for row in kc for x in row), "the export misses a layer"
    return kc, k


def check_preconditions(name, kc, lossless):
    """What slopes = Kc needs: one Kc per layer over the groups, none increasing;
    lossless: the last is 0."""
    if len(kc) > 1:
        assert name in MULTI_GROUP, f"{name}: {len(kc)} rate-control groups"
    for g, row in enumerate(kc):
        assert row == kc[0], f"{name}: group {g} has other thresholds than group 0"
    for l in range(1, len(kc[0])):
        assert kc[0][l] <= kc[0][l - 1], f"{name}: Kc increases at layer {l}"
    if lossless:
        assert kc[0][-1] == 0


def distortion_of(export, L):
    """D[l] by the report's definition, from the export's blocks."""
    D = [0.0] * L
    for b in export["blocks"]:
        dd = b["dd"]
        for l in range(L):
            D[l] += b["weight"] * float(sum(dd[b["nl"][l]:]))
    return D


def expectation(name, with_export=False) -> dict:
    """file: the oracle's (in RPCL, the one order it writes: the selection does
    not depend on the order, progression_cases.resequence gives the others);
    slopes: Kc per layer as thresholds; top: K per layer (the other end of the
    interval); kc: the keys; distortion: D[l]."""
    key = name
    if key not in _expect or with_export:
        conv, rc = recipe(name)
        orc = ol.copy_recipe(rc)
        orc.slope_skip = 0
        orc.progression = 2
        ol.pcrd_export_enable(True)
        try:
            data = ol.encode(image(name), orc)
            ex = ol.pcrd_export()
        finally:
            ol.pcrd_export_enable(False)
        kc, k = layers_of(ex, rc.layers)
        check_preconditions(name, kc, rc.rate_bpp <= 0.0)
        _expect[key] = dict(file=data, kc=kc[0], slopes=[key_to_slope(x) for x in kc[0]],
                            top=[key_to_slope(x) for x in k[0]], distortion=distortion_of(ex, rc.layers),
                            groups=len(kc))
        if with_export:
            return dict(_expect[key], export=ex)
    return _expect[key]


# ---- the COM's columns -------------------------------------------------------------

def com_lines(data: bytes, layers: int):
    """(slope text, bytes text) per layer of a file's Kdu-Layer-Info COM."""
    cs = im.codestream(data)
    for p, m, n in tc.main_header_markers(cs):
        if m == 0x64 and cs[p + 6:p + 6 + len(tc.LAYER_HDR)] == tc.LAYER_HDR:
            o = p + 6 + len(tc.LAYER_HDR)
            return [(cs[o + 17 * l:o + 17 * l + 6].decode(), cs[o + 17 * l + 8:o + 17 * l + 16].decode())
                    for l in range(layers)]
    raise AssertionError("no Kdu-Layer-Info COM")


def slope_text(s: float, bits: int) -> str:
    """What the COM prints for threshold `s` (t2.cpp layer_log_slope)."""
    if s == 0.0:
        v = -192.0
    elif math.isinf(s):
        v = 192.0
    else:
        v = min(192.0, max(-192.0, jp2hip.slope_to_log2(s, bits)))
    return "%6.1f" % v


def with_slope_column(data: bytes, layers: int, slopes, bits: int) -> bytes:
    """`data` with the slope column of its Kdu-Layer-Info COM rendered from `slopes`."""
    hdr = len(data) - len(im.codestream(data))
    cs = bytearray(im.codestream(data))
    for p, m, n in tc.main_header_markers(bytes(cs)):
        if m == 0x64 and cs[p + 6:p + 6 + len(tc.LAYER_HDR)] == tc.LAYER_HDR:
            for l in range(layers):
                o = p + 6 + len(tc.LAYER_HDR) + 17 * l
                cs[o:o + 6] = slope_text(slopes[l], bits).encode()
            return data[:hdr] + bytes(cs)
    raise AssertionError("no Kdu-Layer-Info COM")


def halfway(lo: float, hi: float) -> float:
    """A threshold between lo and hi: the key halfway between theirs."""
    a = struct.unpack("<Q", struct.pack("<d", lo))[0]
    b = INF_KEY if math.isinf(hi) else struct.unpack("<Q", struct.pack("<d", hi))[0]
    return key_to_slope(a + (b - a) // 2)
