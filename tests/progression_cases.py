"""The expected file of every progression order, from the oracle's RPCL file.

The oracle (oracle/jp2_oracle.c) encodes RPCL only.  The progression order
does not change a packet: a precinct's packets go out in increasing layer in
every order, so headers, bodies and lengths are the same.  It moves only the
sequence of the packets inside a tile-part, the Nsop of their SOP markers and
the order of the lengths in the PLT.  resequence() therefore builds the file
of order X from the RPCL file of the same pixels and recipe: it cuts every
tile-part into packets by its PLT, sorts them by the order's key, renumbers
the SOPs, re-emits the PLT and sets the COD's progression byte.
tests/test_progression_orders.py checks the construction against OpenJPEG
(a decoder follows the order, so a wrong sequence does not decode) and the
library's own sequence (jp2hip_packet_sequence) against the key sort here;
tests/test_gpu_progression_orders.py compares the GPU's files with it.

Sort key of packet (l, r, c, precinct), most significant first, with (X, Y)
the precinct's position on the reference grid -- X = max(tx0, px << (PPx_r +
L - r)) for absolute precinct column px of resolution r, Y likewise (B.12.1.3-5
with no component subsampled):

    LRCP  l, r, c, precinct raster index      RPCL  r, Y, X, c, l
    RLCP  r, l, c, precinct raster index      PCRL  Y, X, c, r, l
                                              CPRL  c, Y, X, r, l
"""
from __future__ import annotations

import struct

import numpy as np

import imaging as im
import oracle_lib as ol
import sweep_cases as sc

LRCP, RLCP, RPCL, PCRL, CPRL = range(5)
NAMES = ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL")
NEW_ORDERS = (LRCP, RLCP, PCRL, CPRL)
J2K = dict(format=0, comment=1)

# The four geometries of the CPU and GPU suites (all lossless by default):
# name -> (h, w, nc, recipe overrides).  tparts_r is 0 unless a test sets it.
GEOMETRIES = {
    "rgb_t128": (300, 200, 3, dict(tile_w=128, tile_h=128, levels=3, layers=3)),
    "gray_rect": (130, 150, 1, dict(tile_w=64, tile_h=64, levels=2, layers=2, nprecincts=2,
                                    prec_w_log2=[5, 4], prec_h_log2=[4, 5])),
    "rgb_300": (300, 300, 3, dict()),
    # ragged last tiles (77 = 64 + 13, 101 = 64 + 37), four components
    "rgba_ragged": (77, 101, 4, dict(tile_w=64, tile_h=64, levels=2, layers=4, nprecincts=1,
                                     prec_w_log2=[5], prec_h_log2=[5])),
}


def image(name):
    h, w, nc, _ = GEOMETRIES[name]
    return sc._content("synth", h, w, nc, 8, 20261020 + sorted(GEOMETRIES).index(name))


def overrides(name, order, **more):
    """Recipe overrides of geometry `name` in `order` (raw J2K, one tile-part
    per tile unless `more` says otherwise)."""
    return {**J2K, "tparts_r": 0, **GEOMETRIES[name][3], "progression": order, **more}


def oracle_rpcl(img, rc) -> bytes:
    """The oracle's file for `rc` with its progression set to RPCL."""
    orc = ol.copy_recipe(rc)
    orc.progression = RPCL
    return ol.encode(img, orc)


def expected(img, rc) -> bytes:
    """The file libjp2hip must write for `rc` (needs plt = 1)."""
    return resequence(oracle_rpcl(img, rc), rc.progression)


# ---- geometry ----------------------------------------------------------------

def prec_log2_of(levels, nprecincts, pw, ph):
    """(PPx, PPy) per resolution 0..levels from a recipe's precinct list
    (highest resolution first, the last entry repeats; none: 2^15)."""
    out = []
    for r in range(levels + 1):
        if nprecincts <= 0:
            out.append((15, 15))
        else:
            i = min(levels - r, nprecincts - 1)
            out.append((pw[i], ph[i]))
    return out


def geometry_of_recipe(w, h, nc, rc) -> dict:
    return dict(w=w, h=h, nc=nc, tw=rc.tile_w, th=rc.tile_h, L=rc.levels, layers=rc.layers,
                pp=prec_log2_of(rc.levels, rc.nprecincts, list(rc.prec_w_log2), list(rc.prec_h_log2)))


def geometry_of_codestream(cs: bytes) -> dict:
    seg = im.main_header_segments(cs)
    siz, cod = seg["ff51"], seg["ff52"]
    w, h = struct.unpack(">II", siz[6:14])
    tw, th = struct.unpack(">II", siz[22:30])
    nc = struct.unpack(">H", siz[38:40])[0]
    L = cod[9]
    pp = [(cod[14 + r] & 15, cod[14 + r] >> 4) for r in range(L + 1)] if cod[4] & 1 else [(15, 15)] * (L + 1)
    return dict(w=w, h=h, nc=nc, tw=tw, th=th, L=L, layers=struct.unpack(">H", cod[6:8])[0], pp=pp)


def ntiles(g) -> int:
    return -(-g["w"] // g["tw"]) * -(-g["h"] // g["th"])


def tile_packets(g, t):
    """Tile t's packets in storage (RPCL) order: dicts of l, r, c, raster, X, Y."""
    ntx = -(-g["w"] // g["tw"])
    tx0, ty0 = (t % ntx) * g["tw"], (t // ntx) * g["th"]
    tx1, ty1 = min(g["w"], tx0 + g["tw"]), min(g["h"], ty0 + g["th"])
    out = []
    for r in range(g["L"] + 1):
        sh = g["L"] - r
        ppx, ppy = g["pp"][r]
        rx0, ry0, rx1, ry1 = tx0 >> sh, ty0 >> sh, -((-tx1) >> sh), -((-ty1) >> sh)
        npx = (-((-rx1) >> ppx)) - (rx0 >> ppx) if rx1 > rx0 else 0
        npy = (-((-ry1) >> ppy)) - (ry0 >> ppy) if ry1 > ry0 else 0
        for py in range(npy):
            for px in range(npx):
                X = max(tx0, ((rx0 >> ppx) + px) << (ppx + sh))
                Y = max(ty0, ((ry0 >> ppy) + py) << (ppy + sh))
                for c in range(g["nc"]):
                    for l in range(g["layers"]):
                        out.append(dict(l=l, r=r, c=c, raster=py * npx + px, X=X, Y=Y))
    return out


def sort_key(order):
    return {LRCP: lambda p: (p["l"], p["r"], p["c"], p["raster"]),
            RLCP: lambda p: (p["r"], p["l"], p["c"], p["raster"]),
            RPCL: lambda p: (p["r"], p["Y"], p["X"], p["c"], p["l"]),
            PCRL: lambda p: (p["Y"], p["X"], p["c"], p["r"], p["l"]),
            CPRL: lambda p: (p["c"], p["Y"], p["X"], p["r"], p["l"])}[order]


def tile_sequence(g, t, order):
    """Storage indices of tile t's packets in the sequence of `order`."""
    pk = tile_packets(g, t)
    key = sort_key(order)
    return sorted(range(len(pk)), key=lambda i: key(pk[i]))


# ---- the file ----------------------------------------------------------------

def plt_segments(lens) -> bytes:
    """PLT marker segments of `lens` (A.7.3): 7-bit groups, a segment closes
    when the next length would take it past 65532 bytes, Zplt counts up."""
    segs, cur = [], bytearray()
    for n in lens:
        k = max(1, -(-n.bit_length() // 7))
        v = bytes(((n >> (7 * q)) & 0x7F) | (0x80 if q else 0) for q in range(k - 1, -1, -1))
        if len(cur) + k > 65532:
            segs.append(bytes(cur))
            cur = bytearray()
        cur += v
    if lens:
        segs.append(bytes(cur))
    assert len(segs) <= 256
    return b"".join(b"\xff\x58" + struct.pack(">HB", 3 + len(s), z) + s for z, s in enumerate(segs))


def _split(data: bytes):
    """(bytes before the first SOT, [(sot 12 bytes, markers before SOD other than PLT, PLT lengths,
    packet bytes)], trailer) of a file whose tile-parts carry PLTs."""
    i = data.find(b"\xff\x4f\xff\x51")
    p = i + 2
    while data[p:p + 2] != b"\xff\x90":
        p += 2 + struct.unpack(">H", data[p + 2:p + 4])[0]
    head, parts = data[:p], []
    while data[p:p + 2] == b"\xff\x90":
        psot = struct.unpack(">I", data[p + 6:p + 10])[0]
        q, lens, cur, other = p + 12, [], 0, b""
        while data[q:q + 2] != b"\xff\x93":
            n = struct.unpack(">H", data[q + 2:q + 4])[0]
            if data[q + 1] == 0x58:
                for b in data[q + 5:q + 2 + n]:
                    cur = (cur << 7) | (b & 0x7F)
                    if not b & 0x80:
                        lens.append(cur)
                        cur = 0
            else:
                other += data[q:q + 2 + n]
            q += 2 + n
        body = data[q + 2:p + psot]
        assert sum(lens) == len(body), "the tile-part's PLT does not cover its packets"
        parts.append((data[p:p + 12], other, lens, body))
        p += psot
    return head, parts, data[p:]


def _with_order(head: bytes, order: int) -> bytes:
    i = head.find(b"\xff\x4f\xff\x51")
    p = i + 2
    while head[p:p + 2] != b"\xff\x52":
        p += 2 + struct.unpack(">H", head[p + 2:p + 4])[0]
    return head[:p + 5] + bytes([order]) + head[p + 6:]


def resequence(rpcl_file: bytes, order: int) -> bytes:
    """The file of progression `order` from the RPCL file of the same pixels
    and recipe (tile-parts with PLT; per resolution only for RLCP / RPCL)."""
    g = geometry_of_codestream(im.codestream(rpcl_file))
    sop = bool(im.main_header_segments(im.codestream(rpcl_file))["ff52"][4] & 2)
    head, parts, tail = _split(rpcl_file)
    key = sort_key(order)
    ident = {}   # tile -> its packets' identities, storage order
    taken = {}   # tile -> packets of its earlier tile-parts (= the next Nsop)
    out = [_with_order(head, order)]
    for sot, other, lens, body in parts:
        t = struct.unpack(">H", sot[4:6])[0]
        if t not in ident:
            ident[t], taken[t] = tile_packets(g, t), 0
        n0 = taken[t]
        ids = ident[t][n0:n0 + len(lens)]
        assert len(ids) == len(lens), "more packets than the geometry gives"
        offs = np.concatenate(([0], np.cumsum(lens))).tolist()
        seq = sorted(range(len(lens)), key=lambda i: key(ids[i]))
        new = bytearray()
        for s, i in enumerate(seq):
            pk = bytearray(body[offs[i]:offs[i + 1]])
            if sop:
                assert pk[:4] == b"\xff\x91\x00\x04"
                pk[4:6] = struct.pack(">H", (n0 + s) & 0xFFFF)
            new += pk
        taken[t] = n0 + len(lens)
        tp = sot + other + plt_segments([lens[i] for i in seq]) + b"\xff\x93" + bytes(new)
        assert len(tp) == struct.unpack(">I", sot[6:10])[0], "Psot moved: the PLT segments split differently"
        out.append(tp)
    for t, pk in ident.items():
        assert taken[t] == len(pk), f"tile {t}: {taken[t]} packets of {len(pk)}"
    res = b"".join(out) + tail
    assert len(res) == len(rpcl_file)
    return res


def without_plt(data: bytes) -> bytes:
    """`data` (a raw code-stream, plt = 1) as the same recipe with plt = 0
    writes it: no PLT segments, each Psot lower by their size."""
    head, parts, tail = _split(data)
    out = [head]
    for sot, other, lens, body in parts:
        n = 12 + len(other) + 2 + len(body)
        out.append(sot[:6] + struct.pack(">I", n) + sot[10:] + other + b"\xff\x93" + body)
    return b"".join(out) + tail


def first_difference(got: bytes, want: bytes):
    """None when equal, else a message naming the first differing byte."""
    if got == want:
        return None
    n = min(len(got), len(want))
    d = next((i for i in range(n) if got[i] != want[i]), n)
    return f"{len(got)} vs {len(want)} bytes, first difference at byte {d}"
