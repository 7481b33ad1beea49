"""Cases for the recipe fields the seeded sweep (tests/sweep_cases.py) leaves
at their defaults -- sop, eph, plt, tparts_r, mct, guard_bits, qstep -- and
for three device paths no sweep case is known to reach: bands deeper than 24
bit-planes, PLT chains of more than one segment, and tiles below 128 down to
1x1.  Shared by the oracle's own check (tests/test_oracle_recipe_axes.py,
CPU) and the GPU parity test (tests/test_gpu_recipe_axes.py).

Every case is a dict like sweep_cases': geometry, content kind, seed and
recipe overrides, plus `axis` and, where a case exists to reach one code
path, `pin`: what check_pins() asserts of the oracle's file so that a later
change cannot move the case off that path unnoticed (the deepest band's Mb,
read from the QCD; the PLT segments of the last tile-part).
"""
from __future__ import annotations

import itertools
import struct

import numpy as np

import imaging as im
import sweep_cases as sc

SEED = 20261019
J2K = dict(format=0, comment=1)


def _case(out, axis, name, h, w, nc, bits, lossless, kind, recipe, pin=None):
    i = len(out)
    out.append(dict(idx=i, axis=axis, name=name, h=h, w=w, nc=nc, bits=bits, lossless=lossless,
                    kind=kind, seed=SEED + i, recipe=dict(J2K, **recipe), pin=pin or {}))


def _markers(out):
    # a. every sop / eph / plt / tparts_r combination, on 2x2 ragged tiles of
    # an RGB8 image (precincts of <= 64 blocks: the wave-per-precinct tier-2)
    # and with 16x16 blocks on a gray one (192 blocks in the largest
    # precincts: the serial k_t2_code + k_apply)
    for nc, cb, tag in ((3, 6, "rgb_cb64"), (1, 4, "gray_cb16")):
        for n, (sop, eph, plt, tpr) in enumerate(itertools.product((0, 1), repeat=4)):
            lossless = n % 2 == 0
            _case(out, "markers", f"{tag}_sop{sop}_eph{eph}_plt{plt}_tpr{tpr}", 300, 420, nc, 8, lossless, "synth",
                  dict(sop=sop, eph=eph, plt=plt, tparts_r=tpr, tile_w=256, tile_h=256, cblk_w_log2=cb,
                       cblk_h_log2=cb, rate_bpp=0.0 if lossless else 2.0, flush_period=(0, 512, 1024)[n % 3]))


def _mct(out):
    # b. three and four components with no colour transform (compw[] = 1)
    for nc, bits, lossless, driven, levels in itertools.product((3, 4), (8, 16), (True, False), (False, True), (0, 3)):
        rate = (3.0 if lossless else 2.0) if driven else 0.0
        _case(out, "mct0", f"L{levels}_r{rate}", 140, 190, nc, bits, lossless, "synth",
              dict(mct=0, levels=levels, tile_w=128, tile_h=128, rate_bpp=rate))


def _guard(out):
    # c. guard bits move Mb: the zero-bit-plane tag trees, QuantTab::q16 / lim
    # and (reversible 8-bit, guard_bits >= 5) the 32-bit index plane
    for g, (nc, bits), lossless in itertools.product((0, 2, 4, 5, 7), ((3, 8), (1, 16), (3, 16)), (True, False)):
        _case(out, "guard", f"g{g}", 150, 210, nc, bits, lossless, "synth",
              dict(guard_bits=g, levels=4, tile_w=128, tile_h=128, rate_bpp=0.0 if lossless else 2.0))
    # deep zero-bit-plane trees: 16x16 blocks, many layers, mostly empty content
    for g, kind, lossless, layers, bits in ((0, "flat", True, 12, 8), (5, "sparse", True, 16, 8), (7, "sparse", False, 12, 16),
                                            (7, "flat", True, 14, 16), (4, "flat", False, 12, 8)):
        _case(out, "guard", f"g{g}_cb16_ly{layers}", 260, 330, 1, bits, lossless, kind,
              dict(guard_bits=g, levels=5, layers=layers, tile_w=256, tile_h=256, cblk_w_log2=4, cblk_h_log2=4,
                   rate_bpp=0.0 if lossless else 2.0))


QSTEPS = (2.0 ** -4, 2.0 ** -6, 2.0 ** -10, 2.0 ** -12)


def _qstep(out):
    # d. the irreversible step from coarser than the sample range to far finer
    # than a sample
    for (nc, bits), q, rate in itertools.product(((3, 8), (1, 16)), (2.0,) + QSTEPS, (0.0, 2.0)):
        _case(out, "qstep", f"q{q:g}", 150, 210, nc, bits, False, "synth",
              dict(qstep=q, levels=4, tile_w=128, tile_h=128, rate_bpp=rate))


def _deep(out):
    # e. bands of 25..30 magnitude bit-planes (k_quant's d.Mb > 24 path, the
    # limit of build_plan).  With levels=0 the one band has Delta = 2^(16-e)
    # for qstep = 2^-e, so a sample 32767 from the level shift has the index
    # floor(32767 / Delta): real bits above plane 24.
    for rate in (0.0, 4.0):
        for e, g, mb in ((29, 1, 29), (30, 1, 30), (27, 3, 29)):
            assert int(32767 / 2.0 ** (16 - e)) >= 1 << 24
            _case(out, "deep", f"L0_q2^-{e}_g{g}", 150, 130, 1, 16, False, "deep",
                  dict(levels=0, qstep=2.0 ** -e, guard_bits=g, tile_w=128, tile_h=128, rate_bpp=rate),
                  pin=dict(max_mb=mb))
    # with levels the deepest band is LL: Mb 30 named by the recipe; the second
    # value is the one the oracle's QCD holds (pinned, not derived)
    _case(out, "deep", "L2_q2^-27", 150, 130, 1, 16, False, "deep",
          dict(levels=2, qstep=2.0 ** -27, tile_w=128, tile_h=128, rate_bpp=0.0), pin=dict(max_mb=30))
    _case(out, "deep", "L1_q2^-28", 150, 130, 1, 16, False, "deep",
          dict(levels=1, qstep=2.0 ** -28, tile_w=128, tile_h=128, rate_bpp=4.0), pin=dict(max_mb=30))
    # Mb > 24 over shallow data: reversible 16-bit with every guard bit
    _case(out, "deep", "rgb16_ll_g7", 150, 130, 3, 16, True, "synth",
          dict(guard_bits=7, levels=3, tile_w=128, tile_h=128, rate_bpp=0.0), pin=dict(min_max_mb=25))


TINY = ((64, 64, 6), (32, 32, 3), (32, 32, 5), (16, 16, 4), (64, 16, 2), (8, 8, 0), (4, 4, 2), (2, 2, 1), (1, 1, 0))


def _tiny(out):
    # f. tiles below 128; 1x1 is 7000 tiles and tile-parts, the smallest shape
    # that makes the tile-part scan (t2_total_body) walk runs of them
    for (tw, th, lv), (h, w, nc, bits), lossless in itertools.product(TINY, ((70, 100, 3, 8), (100, 70, 1, 16)),
                                                                     (True, False)):
        _case(out, "tiny", f"T{tw}x{th}_L{lv}", h, w, nc, bits, lossless, "synth",
              dict(tile_w=tw, tile_h=th, levels=lv, rate_bpp=0.0 if lossless else 2.0))
    # odd image sizes: the last tile column / row is one sample wide / high, a
    # width the level-1 DWT handles apart from the others
    for (tw, th, lv), (h, w, nc, bits) in itertools.product(((2, 2, 1), (4, 4, 2), (16, 16, 4)),
                                                            ((37, 53, 3, 8), (53, 37, 1, 16))):
        _case(out, "tiny", f"T{tw}x{th}_L{lv}_odd", h, w, nc, bits, True, "synth",
              dict(tile_w=tw, tile_h=th, levels=lv, rate_bpp=0.0))


def _plt(out):
    # g. PLT chains: the last tile-part's packet lengths need 3, 4 and
    # (just over the 65532-byte boundary) 2 segments
    big = dict(tile_w=2048, tile_h=2048, layers=32, nprecincts=1, prec_w_log2=[5], prec_h_log2=[5],
               cblk_w_log2=4, cblk_h_log2=4, rate_bpp=0.0)
    _case(out, "plt", "3seg", 1100, 1100, 4, 8, True, "synth", dict(big), pin=dict(nplt=3, nlen=156800))
    _case(out, "plt", "4seg_tpr0", 1100, 1100, 4, 8, True, "synth", dict(big, tparts_r=0),
          pin=dict(nplt=4, nlen=213632))
    _case(out, "plt", "4seg_tpr0_sop0", 1100, 1100, 4, 8, True, "synth", dict(big, tparts_r=0, sop=0),
          pin=dict(nplt=4, nlen=213632))
    _case(out, "plt", "2seg", 760, 760, 1, 8, True, "synth",
          dict(tile_w=1024, tile_h=1024, layers=32, nprecincts=1, prec_w_log2=[4], prec_h_log2=[4],
               cblk_w_log2=3, cblk_h_log2=3, rate_bpp=0.0), pin=dict(nplt=2, nlen=73728))


def cases():
    """The same list on every box."""
    out = []
    for f in (_markers, _mct, _guard, _qstep, _deep, _tiny, _plt):
        f(out)
    return out


def case_id(c):
    return (f"{c['axis']}_{c['idx']:03d}_{c['name']}_{c['h']}x{c['w']}x{c['nc']}_{c['bits']}b_"
            f"{'ll' if c['lossless'] else 'ly'}_r{c['recipe']['rate_bpp']}")


def image(c):
    if c["kind"] != "deep":
        return sc._content(c["kind"], c["h"], c["w"], c["nc"], c["bits"], c["seed"])
    # uniform noise with a patch of the largest and of the smallest sample:
    # blocks with every magnitude bit in use
    a = sc._content("noise", c["h"], c["w"], c["nc"], c["bits"], c["seed"])
    a[8:16, 8:16] = (1 << c["bits"]) - 1
    a[24:32, 40:48] = 0
    return a


def band_mb(cs: bytes) -> list:
    """Mb of every band, from the QCD of a code-stream (A.6.4, E-2):
    guard bits + exponent - 1."""
    qcd = im.main_header_segments(cs)["ff5c"]
    g, style = qcd[4] >> 5, qcd[4] & 31
    if style == 0:
        eps = [b >> 3 for b in qcd[5:]]
    else:
        eps = [v >> 11 for v in struct.unpack(f">{(len(qcd) - 5) // 2}H", qcd[5:])]
    return [g + e - 1 for e in eps]


def check_pins(c, oracle_file: bytes, walk=None):
    """Assert that the oracle's file for case `c` is on the path the case
    exists for (`walk`: tile_part_walk's result if the caller has it)."""
    pin = c["pin"]
    cs = im.codestream(oracle_file)
    if "max_mb" in pin:
        assert max(band_mb(cs)) == pin["max_mb"], (band_mb(cs), pin)
    if "min_max_mb" in pin:
        assert max(band_mb(cs)) >= pin["min_max_mb"], (band_mb(cs), pin)
    if "nplt" in pin:
        last = (walk or im.tile_part_walk(cs, c["recipe"].get("sop", 1)))[-1]
        assert (last[3], len(last[4])) == (pin["nplt"], pin["nlen"]), (last[3], len(last[4]), pin)


def check_structure(case, data):
    """tile_part_walk plus what only the recipe can tell: no PLT without plt,
    Scod's EPH bit."""
    r = case["recipe"]
    walk = im.tile_part_walk(data, r.get("sop", 1))
    scod = im.main_header_segments(im.codestream(data))["ff52"][4]
    assert bool(scod & 4) == bool(r.get("eph", 1))
    if r.get("plt", 1):
        assert all(tp[3] >= 1 for tp in walk)
    else:
        assert all(tp[3] == 0 for tp in walk)
    return walk


# recipes the main header cannot hold: (field the message must name, overrides)
BAD = [("guard_bits", dict(guard_bits=8)), ("guard_bits", dict(guard_bits=-1)),
       ("qstep", dict(qstep=0.0)), ("qstep", dict(qstep=-1.0 / 256)), ("qstep", dict(qstep=float("nan"))),
       ("qstep", dict(qstep=float("inf"))),
       ("nprecincts", dict(nprecincts=17)), ("nprecincts", dict(nprecincts=-1)),
       ("prec_w_log2", dict(nprecincts=1, prec_w_log2=[16], prec_h_log2=[8])),
       ("prec_h_log2", dict(nprecincts=2, prec_w_log2=[8, 8], prec_h_log2=[8, -1])),
       # 2^0 above resolution 0: its bands' precincts would be half a sample (B.6)
       ("prec_w_log2", dict(nprecincts=1, prec_w_log2=[0], prec_h_log2=[0], levels=1, tile_w=64, tile_h=64))]
BAD_IDS = [f"{f}_{i}" for i, (f, _) in enumerate(BAD)]
