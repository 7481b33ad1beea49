"""The expected file of an encode with TLM marker segments (ORGgen_tlm,
jp2hip_set_organisation), from the file without them.

The TLM segments (ISO/IEC 15444-1 A.7.1) are the last marker segments of the
main header: per segment FF55, Ltlm = 4 + 6 k, Ztlm = 0, 1, ..., Stlm = 0x60
(16-bit Ttlm, 32-bit Ptlm), then k <= 10921 pairs (tile index, tile-part
length), one per tile-part in the order the tile-parts lie in the file.
with_tlm() therefore walks the tile-parts of the base file, inserts the
segments before the first SOT, adds their T bytes to Kdu-Layer-Info's L(bytes)
column (which counts the header bytes) and writes the file header again for
the longer code-stream.  Nothing else of the file moves.

The base file is the oracle's (for another progression order
progression_cases.expected).  A rate-driven encode with a TLM is defined as the
encode without one whose byte target is T lower, so its base file is the
oracle's at lower_rate(): a rate whose floor(rate * W * H / 8) is exactly
target - T.
"""
from __future__ import annotations

import math
import struct

import numpy as np

import imaging as im
import jp2hip
import oracle_lib as ol
import progression_cases as pc
import sweep_cases as sc

SEG_ENTRIES = 10921          # (65535 - 4) // 6
MAX_ENTRIES = 256 * SEG_ENTRIES
LAYER_HDR = b"Kdu-Layer-Info: log_2{Delta-D(squared-error)/Delta-L(bytes)}, L(bytes)\n"


def segments(tiles, lengths) -> bytes:
    """The TLM marker segments for tile-parts in file order (the model of
    jp2hip_tlm_segments)."""
    assert len(tiles) == len(lengths) <= MAX_ENTRIES
    out = []
    for z, i0 in enumerate(range(0, len(tiles), SEG_ENTRIES)):
        k = min(SEG_ENTRIES, len(tiles) - i0)
        out.append(b"\xff\x55" + struct.pack(">HBB", 4 + 6 * k, z, 0x60))
        out.append(np.rec.fromarrays([np.asarray(tiles[i0:i0 + k], ">u2"), np.asarray(lengths[i0:i0 + k], ">u4")])
                   .tobytes())
    return b"".join(out)


def tlm_bytes(ntp: int) -> int:
    return 6 * ntp + 6 * -(-ntp // SEG_ENTRIES)


def first_sot(cs: bytes) -> int:
    """Offset of the first SOT of a code-stream, found segment by segment."""
    assert cs[:2] == b"\xff\x4f"
    p = 2
    while cs[p:p + 2] != b"\xff\x90":
        assert cs[p] == 0xFF, f"no marker at byte {p}"
        p += 2 + struct.unpack(">H", cs[p + 2:p + 4])[0]
    return p


def main_header_markers(cs: bytes):
    """(offset, marker byte, segment length with the marker) of the main header's segments."""
    out, p, end = [], 2, first_sot(cs)
    while p < end:
        n = 2 + struct.unpack(">H", cs[p + 2:p + 4])[0]
        out.append((p, cs[p + 1], n))
        p += n
    return out


def layer_info(mh: bytes, layers: int, ends) -> bytes:
    """Main header `mh` with the L(bytes) column of its Kdu-Layer-Info COM
    rendered from `ends` (the code-stream bytes through each layer), as the
    oracle's write_main_header renders it: "%6.1f, %8.1e\\n" per layer."""
    for p, m, n in main_header_markers(mh + b"\xff\x90"):
        if m == 0x64 and mh[p + 6:p + 6 + len(LAYER_HDR)] == LAYER_HDR:
            assert n == 6 + len(LAYER_HDR) + 17 * layers
            out = bytearray(mh)
            for l in range(layers):
                o = p + 6 + len(LAYER_HDR) + 17 * l
                field = b"%8.1e" % float(ends[l])
                assert len(field) == 8 and out[o + 6:o + 8] == b", " and out[o + 16] == 0x0A
                out[o + 8:o + 16] = field
            return bytes(out)
    raise AssertionError("no Kdu-Layer-Info COM in the main header")


def layer_ends(cs: bytes, extra: int, layer_source: bytes | None = None):
    """Code-stream bytes through each layer of `cs` with `extra` more header
    bytes: main header + extra + every tile-part header + the packets of
    layers 0..l.  The packet sums come from `layer_source` (a code-stream of
    the same packets in a layer-innermost order, with SOP markers) when the
    order of `cs` is not layer-innermost."""
    src = cs if layer_source is None else layer_source
    seg = im.main_header_segments(cs)
    cod = seg["ff52"]
    assert cod[4] & 2, "the layer sums need SOP markers"
    layers = struct.unpack(">H", cod[6:8])[0]
    per_layer = im.packet_bytes_by_layer(src[first_sot(src):], layers)
    parts = im.tile_parts(cs[first_sot(cs):])
    acc = first_sot(cs) + extra + sum(p[1] for p in parts) - sum(per_layer)
    ends = []
    for n in per_layer:
        acc += n
        ends.append(acc)
    return layers, ends


def with_tlm(data: bytes, layout, fmt: int, layer_source: bytes | None = None) -> bytes:
    """The file an encode with organisation tlm = 1 must write, from the file
    `data` of the same encode without it.  `layout` and `fmt` describe the
    source and the format for jp2hip.file_header; `layer_source`: see
    layer_ends (a file or code-stream)."""
    cs = im.codestream(data)
    assert jp2hip.file_header(layout, fmt, len(cs)) == data[:len(data) - len(cs)], "the base file's own header"
    sot = first_sot(cs)
    parts = im.tile_parts(cs[sot:])
    assert cs[sot + sum(p[1] for p in parts):] == b"\xff\xd9"
    seg = segments([p[0] for p in parts], [p[1] for p in parts])
    assert len(seg) == tlm_bytes(len(parts))
    mh = cs[:sot]
    if any(m == 0x64 and cs[p + 6:p + 6 + len(LAYER_HDR)] == LAYER_HDR for p, m, _ in main_header_markers(cs)):
        layers, ends = layer_ends(cs, len(seg), None if layer_source is None else im.codestream(layer_source))
        mh = layer_info(mh, layers, ends)
    new = mh + seg + cs[sot:]
    return jp2hip.file_header(layout, fmt, len(new)) + new


def parse(data: bytes):
    """Reads a file's TLM as a reader would: the entries (tile, length) of
    the segments at the end of the main header, having checked that they are
    its last marker segments, that Ztlm counts 0, 1, ..., and that walking from
    the end of the main header by the lengths lands on an SOT with that Isot
    and Psot every time and on EOC at the end."""
    cs = im.codestream(data)
    marks = main_header_markers(cs)
    tlm = [(p, n) for p, m, n in marks if m == 0x55]
    assert tlm, "no TLM marker segment"
    assert [m for _, m, _ in marks[-len(tlm):]] == [0x55] * len(tlm), "TLM segments are not the last of the main header"
    entries = []
    for z, (p, n) in enumerate(tlm):
        assert cs[p + 4] == z and cs[p + 5] == 0x60 and (n - 6) % 6 == 0 and n > 6
        assert n == 6 + 6 * SEG_ENTRIES or z == len(tlm) - 1, "a segment that is not full before the last"
        rec = np.frombuffer(cs, np.dtype([("t", ">u2"), ("n", ">u4")]), (n - 6) // 6, p + 6)
        entries += list(zip(rec["t"].tolist(), rec["n"].tolist()))
    p = first_sot(cs)
    for t, n in entries:
        assert cs[p:p + 2] == b"\xff\x90", f"no SOT at byte {p}"
        isot, psot = struct.unpack(">HI", cs[p + 4:p + 10])
        assert (isot, psot) == (t, n), f"SOT at {p}: tile {isot} length {psot}, TLM says {t}, {n}"
        p += n
    assert cs[p:] == b"\xff\xd9", "the TLM's lengths do not end at EOC"
    return entries


# ---- rate-driven cases -------------------------------------------------------------

def rate_target(rate: float, w: int, h: int) -> int:
    return math.floor(rate * w * h / 8.0)


def lower_rate(rate: float, w: int, h: int, T: int) -> float:
    """The rate whose byte target is that of `rate` less T (floored at 0)."""
    want = max(0, rate_target(rate, w, h) - T)
    r = (want + 0.5) * 8.0 / (w * h)
    assert rate_target(r, w, h) == want
    return r


def tile_part_count(w: int, h: int, rc) -> int:
    """Tile-parts of a w x h image under `rc` (tile_w = tile_h = 0: one tile):
    one per tile, or with tparts_r one per non-empty resolution of each."""
    tw, th = (rc.tile_w, rc.tile_h) if rc.tile_w else (w, h)
    n = 0
    for y0 in range(0, h, th):
        for x0 in range(0, w, tw):
            x1, y1 = min(w, x0 + tw), min(h, y0 + th)
            res = sum(1 for r in range(rc.levels + 1)
                      if -((-x1) >> (rc.levels - r)) > (x0 >> (rc.levels - r))
                      and -((-y1) >> (rc.levels - r)) > (y0 >> (rc.levels - r)))
            n += res if rc.tparts_r else 1
    return n


def oracle_recipe(img: np.ndarray, rc):
    """The oracle's recipe for the base file of `rc` with organisation tlm = 1:
    `rc` itself (tile_w = tile_h = 0 resolved to the one tile the encode
    makes), for a rate-driven recipe at the target lowered by the TLM's bytes."""
    h, w = img.shape[:2]
    orc = ol.copy_recipe(rc)
    if rc.tile_w == 0 and rc.tile_h == 0:
        m = 1 << rc.levels
        orc.tile_w, orc.tile_h = -(-w // m) * m, -(-h // m) * m
    if rc.rate_bpp > 0.0:
        orc.rate_bpp = lower_rate(rc.rate_bpp, w, h, tlm_bytes(tile_part_count(w, h, rc)))
    return orc


def layout_of(img: np.ndarray):
    """A Layout that states what jp2hip.file_header reads of this image."""
    lay = jp2hip._lib.Layout()
    lay.height, lay.width = img.shape[:2]
    lay.components = 1 if img.ndim == 2 else img.shape[2]
    lay.bits = img.dtype.itemsize * 8
    return lay


def expected(img: np.ndarray, rc) -> bytes:
    """The file libjp2hip must write for `rc` after set_organisation(tlm=1):
    with_tlm of the oracle's file (another order: re-sequenced by
    progression_cases, its layer sums taken from the RPCL file)."""
    orc = oracle_recipe(img, rc)
    if rc.progression == pc.RPCL:
        return with_tlm(ol.encode(img, orc), layout_of(img), rc.format)
    rpcl = pc.oracle_rpcl(img, orc)
    return with_tlm(pc.resequence(rpcl, rc.progression), layout_of(img), rc.format, rpcl)


# ---- the cases the CPU and GPU suites share ----------------------------------------

def lossless_image():
    """RGB8, 700 wide, 1100 high: 2 x 3 tiles of 512, two -flush_period
    stripes (rows 0..1023, then the rest), 42 tile-parts whose Ttlm go 0, 1,
    2, 3, 0, 1, ... then 4, 5, 4, 5, ..."""
    if "ll" not in _images:
        _images["ll"] = im.synth_rgb8(1100, 700, seed=20261021)
        _images["ll"].setflags(write=False)
    return _images["ll"]


_images = {}

# The first lossy case: the default lossy recipe on lossless_image().  The
# oracle at target - T (T = 258) writes other bytes than at the target
# (test_tlm.py checks that), so an uncounted T cannot pass.
LOSSY_T_SENSITIVE = dict()


def two_iteration_case():
    """The second lossy case: RGB8 300 wide, 420 high, one tile, 8 x 8
    code-blocks at 0.5 bpp with slope_skip = 0 -- the oracle's rate loop needs
    TWO_ITERATION_COUNT iterations at target - T (test_tlm.py checks that)."""
    return im.synth_rgb8(420, 300, seed=20261021), \
        jp2hip.recipe(jp2hip.LOSSY, rate_bpp=0.5, cblk_w_log2=3, cblk_h_log2=3, slope_skip=0)


TWO_ITERATION_COUNT = 2


def over_target_case():
    """The over-target door: 64 x 64 tiles at 0.5 bpp never fit their headers
    (all 8 iterations, the file stays over the target)."""
    return im.synth_rgb8(420, 300, seed=20261021), \
        jp2hip.recipe(jp2hip.LOSSY, rate_bpp=0.5, tile_w=64, tile_h=64)


def order_case(order: int, tparts_r: int):
    """200 wide, 150 high, grey8, 64 x 64 tiles (4 x 3), 2 levels, raw J2K with
    COM markers, in `order`: 12 tile-parts, or 36 with tparts_r."""
    img = sc._content("synth", 150, 200, 1, 8, 20261022)
    return img, jp2hip.recipe(jp2hip.LOSSLESS, **pc.J2K, progression=order, tparts_r=tparts_r, tile_w=64,
                              tile_h=64, levels=2)


def untiled_case():
    """tile_w = tile_h = 0 on 300 wide, 200 high, grey16: one tile, 7 tile-parts."""
    return im.synth_u16(200, 300, comps=1, seed=20261023), jp2hip.recipe(jp2hip.LOSSLESS, tile_w=0, tile_h=0)


def multi_segment_case():
    """grey8 840 x 840 in 8 x 8 tiles of 1 level with a tile-part per
    resolution: 105 x 105 x 2 = 22 050 tile-parts in one flush stripe, three
    TLM segments (10 921, 10 921, 208 entries); the second starts inside the
    run of resolution 0 and wraps to tile 0's resolution 1."""
    return sc._content("synth", 840, 840, 1, 8, 20261021), \
        jp2hip.recipe(jp2hip.LOSSLESS, tile_w=8, tile_h=8, levels=1, tparts_r=1)
