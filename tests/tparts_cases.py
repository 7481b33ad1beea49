"""The expected file of an encode with the tile-part divisions L and C
(ORGtparts, jp2hip_set_tile_part_divisions), from the file without them.

A tile sends its packets in the recipe's progression order; the divisions cut
that sequence into tile-parts: a new one starts before every packet that
differs from the one before it in a flagged index -- resolution for R
(recipe.tparts_r), layer for L, component for C.  No packet byte and no Nsop
changes, so divide() builds the divided file from the undivided file of the
same recipe and order (plt = 1): per tile it joins the tile-parts' packets,
cuts them anew by runs(), writes each part's SOT (TPsot 0, 1, ...; TNsot = the
count on the tile's last part, else 0; Psot), PLT and SOD, puts the parts in
file order -- per -flush_period stripe part 0 of every tile of the stripe,
then part 1, ... -- and renders the Kdu-Layer-Info COM and the file header
again for the bytes the added headers take.

A rate-driven encode with letters is defined as the encode without them whose
byte target is E = (14 + 5 plt) * (tile-parts added) lower (on top of the
TLM's T), so expected() runs the oracle at tlm_cases.lower_rate() of that.
"""
from __future__ import annotations

import struct

import numpy as np

import imaging as im
import jp2hip
import oracle_lib as ol
import progression_cases as pc
import tlm_cases as tc

L, C = 2, 4  # JP2HIP_TPARTS_L, JP2HIP_TPARTS_C
LETTERS = {"L": L, "C": C, "LC": L | C}
MAX_PARTS = 255


def runs(g, t, order, letters, tparts_r):
    """Places of tile t's packet sequence (progression_cases.tile_sequence) at
    which a tile-part starts under the divisions R (tparts_r), L, C."""
    pk = pc.tile_packets(g, t)
    seq = pc.tile_sequence(g, t, order)

    def flagged(p):
        return (p["r"] if tparts_r else 0, p["l"] if letters & L else 0, p["c"] if letters & C else 0)
    return [s for s in range(len(seq)) if s == 0 or flagged(pk[seq[s]]) != flagged(pk[seq[s - 1]])]


def stripe_ends(nty, tile_h, h, period):
    """One past the last tile row of each -flush_period stripe (the model of
    flush_stripe_ends: a stripe ends once the rows pushed reach the next
    multiple of the period, and at the last tile row)."""
    ends, nxt = [], period
    for ty in range(nty):
        bottom = min((ty + 1) * tile_h, h)
        if period <= 0 or bottom >= nxt or ty == nty - 1:
            ends.append(ty + 1)
            while period > 0 and nxt <= bottom:
                nxt += period
    return ends


def file_order(g, counts, period):
    """(tile, part) in file order for tiles with `counts` tile-parts each."""
    ntx, nty = -(-g["w"] // g["tw"]), -(-g["h"] // g["th"])
    out, ty0 = [], 0
    for e in stripe_ends(nty, g["th"], g["h"], period):
        tiles = range(ty0 * ntx, e * ntx)
        for k in range(max(counts[t] for t in tiles)):
            out += [(t, k) for t in tiles if k < counts[t]]
        ty0 = e
    return out


def resolved(rc, w, h):
    """`rc` with tile_w = tile_h = 0 made the one tile the encode makes."""
    orc = ol.copy_recipe(rc)
    if rc.tile_w == 0 and rc.tile_h == 0:
        m = 1 << rc.levels
        orc.tile_w, orc.tile_h = -(-w // m) * m, -(-h // m) * m
    return orc


def part_counts(w, h, nc, rc, letters):
    """Tile-parts of every tile of a w x h image of nc components under `rc` and `letters`."""
    g = pc.geometry_of_recipe(w, h, nc, resolved(rc, w, h))
    return [len(runs(g, t, rc.progression, letters, rc.tparts_r)) for t in range(pc.ntiles(g))]


def division_bytes(w, h, nc, rc, letters) -> int:
    """E: what the letters add to a code-stream whose PLTs are one segment each."""
    return (14 + (5 if rc.plt else 0)) * (sum(part_counts(w, h, nc, rc, letters)) - sum(part_counts(w, h, nc, rc, 0)))


def _render(data: bytes, layout, fmt: int, layer_source):
    """`data` with its Kdu-Layer-Info COM (if any) and its file header written
    for the tile-part headers it has now."""
    cs = im.codestream(data)
    sot = tc.first_sot(cs)
    mh = cs[:sot]
    if any(m == 0x64 and cs[p + 6:p + 6 + len(tc.LAYER_HDR)] == tc.LAYER_HDR for p, m, _ in tc.main_header_markers(cs)):
        layers, ends = tc.layer_ends(cs, 0, None if layer_source is None else im.codestream(layer_source))
        mh = tc.layer_info(mh, layers, ends)
    new = mh + cs[sot:]
    return jp2hip.file_header(layout, fmt, len(new)) + new


def divide(data: bytes, letters: int, rc, layout, layer_source: bytes | None = None) -> bytes:
    """The file an encode of `rc` with `letters` must write, from the file
    `data` of the same recipe (plt = 1) without them.  `rc` gives tparts_r and
    flush_period (the code-stream states neither); `layout`: the source, for
    jp2hip.file_header; `layer_source`: see tlm_cases.layer_ends."""
    cs = im.codestream(data)
    g = pc.geometry_of_codestream(cs)
    order = im.main_header_segments(cs)["ff52"][5]
    head, parts, tail = pc._split(data)
    assert tail == b"\xff\xd9"
    lens, body, cuts = {}, {}, {}
    for sot, other, ln, bd in parts:  # a tile's parts lie in TPsot order in the file
        t, tp = struct.unpack(">H", sot[4:6])[0], sot[10]
        assert other == b"" and tp == len(cuts.setdefault(t, []))
        cuts[t].append(len(lens.setdefault(t, [])))
        lens[t] += ln
        body[t] = body.get(t, b"") + bd
    new, counts = {}, {}
    for t in sorted(lens):
        first = runs(g, t, order, letters, rc.tparts_r)
        assert len(lens[t]) == len(pc.tile_packets(g, t)) and set(cuts[t]) <= set(first), \
            f"tile {t}: the undivided file's own tile-parts are not runs of the rule"
        assert len(first) <= MAX_PARTS, f"tile {t}: {len(first)} tile-parts"
        offs = np.concatenate(([0], np.cumsum(lens[t]))).tolist()
        counts[t] = len(first)
        for i, s0 in enumerate(first):
            s1 = first[i + 1] if i + 1 < len(first) else len(lens[t])
            plt = pc.plt_segments(lens[t][s0:s1])
            pk = body[t][offs[s0]:offs[s1]]
            sot = b"\xff\x90\x00\x0a" + struct.pack(">HIBB", t, 12 + len(plt) + 2 + len(pk), i,
                                                    len(first) if i == len(first) - 1 else 0)
            new[t, i] = sot + plt + b"\xff\x93" + pk
    assert sorted(counts) == list(range(pc.ntiles(g)))
    out = head + b"".join(new[tk] for tk in file_order(g, counts, rc.flush_period)) + tail
    return _render(out, layout, rc.format, layer_source)


def expected(img: np.ndarray, rc, letters: int, tlm: int = 0) -> bytes:
    """The file libjp2hip must write for `rc` after
    set_tile_part_divisions(letters) (and set_organisation(tlm)): divide() of
    progression_cases.expected, for a rate-driven recipe of the oracle at the
    rate whose target is E (+ T) lower."""
    h, w = img.shape[:2]
    nc = 1 if img.ndim == 2 else img.shape[2]
    orc = resolved(rc, w, h)
    orc.plt = 1
    if rc.rate_bpp > 0.0:
        cut = division_bytes(w, h, nc, rc, letters)
        if tlm:
            cut += tc.tlm_bytes(sum(part_counts(w, h, nc, rc, letters)))
        if cut:
            orc.rate_bpp = tc.lower_rate(rc.rate_bpp, w, h, cut)
    lay = tc.layout_of(img)
    rpcl = pc.oracle_rpcl(img, orc)
    base = rpcl if rc.progression == pc.RPCL else pc.resequence(rpcl, rc.progression)
    out = divide(base, letters, rc, lay, rpcl)
    if not rc.plt:
        assert rc.format == 0, "without_plt takes a raw code-stream"
        out = _render(pc.without_plt(out), lay, rc.format, rpcl)
    return tc.with_tlm(out, lay, rc.format, rpcl) if tlm else out


def walk(data: bytes):
    """Reads the tile-parts as a reader does, by Psot from the first SOT to
    EOC: [(tile, TPsot, TNsot)], having checked that a tile's TPsot count 0,
    1, ... in file order and that its TNsot is 0 or, on its last part, its count."""
    cs = im.codestream(data)
    p, seen, out = tc.first_sot(cs), {}, []
    while cs[p:p + 2] == b"\xff\x90":
        t, psot, tp, tn = struct.unpack(">HIBB", cs[p + 4:p + 12])
        assert tp == seen.get(t, 0), f"tile {t}: TPsot {tp} after {seen.get(t, 0)} parts"
        seen[t] = tp + 1
        out.append((t, tp, tn))
        p += psot
    assert cs[p:] == b"\xff\xd9", "the Psot chain does not end at EOC"
    for t, n in seen.items():
        tns = [tn for u, _, tn in out if u == t]
        assert tns[-1] == n and not any(tns[:-1]), f"tile {t}: TNsot {tns} for {n} parts"
    return out
