"""Crafted Deflate streams for k_inflate / k_inflate_links (csrc/inflate_kernels.h):
a block-level writer, a plain-Python model of RFC 1950/1951 with the product's
end rules, and a census of the kernel's paths measured in the same walk.

The writer takes the blocks, code lengths, code-length symbols and tokens as
given (zlib chooses its own, and never chooses most of what is here).  The
model restates the RFCs and is pinned to zlib in test_inflate_cases.py; the
census restates the kernel's rules from its comments (a window of kInfLanes bit
offsets from P, refilled when the offset o reaches kInfLanes; the ring topped
up when k + 8 >= loaded, restarted when k >= loaded) with the constants read
out of the source.  Nothing here imports the product.

`python tests/inflate_cases.py` re-measures the census and rewrites
tests/golden/inflate_pins.json."""
from __future__ import annotations

import functools
import hashlib
import json
import os
import re
import struct
import sys
import zlib
from collections import Counter
from typing import NamedTuple

import numpy as np

import imaging as im

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KERNEL = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc", "inflate_kernels.h")
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate_pins.json")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


# --------------------------------------------------------------------------
# the kernel's constants, read from its source
# --------------------------------------------------------------------------
def _const(text: str, name: str) -> int:
    m = re.search(r"\b" + name + r"\s*=\s*([^;,]+)[;,]", text)
    assert m, name
    assert re.fullmatch(r"[\d\s]+", m.group(1)), (name, m.group(1))
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def kernel_constants() -> dict:
    text = open(KERNEL).read()
    k = {n: _const(text, n) for n in ("kInfLB", "kInfDB", "kLinkDoublings", "kLinkChunk")}
    m = re.search(r"#define\s+JP2HIP_INF_LANES\s+(\d+)", text)
    assert m, "JP2HIP_INF_LANES"
    k["JP2HIP_INF_LANES"] = int(m.group(1))
    m = re.search(r"\bkInChunkWords\s*=\s*(\d+)\s*\*\s*kInfLanes\s*;", text)
    assert m, "kInChunkWords"
    k["kInChunkWords"] = int(m.group(1)) * k["JP2HIP_INF_LANES"]
    return k


# --------------------------------------------------------------------------
# writer
# --------------------------------------------------------------------------
def canonical_codes(lengths) -> list:
    """RFC 1951 3.2.2: the code of every symbol from the code lengths (codes
    of over-subscribed lengths are cut to their length: such a table is
    refused before any code is read)."""
    count = Counter(l for l in lengths if l)
    code, nxt = 0, {}
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l] & ((1 << l) - 1))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def stored(data: bytes, final=None, len_field=None, nlen_field=None) -> dict:
    return dict(type=0, data=bytes(data), final=final, len_field=len_field, nlen_field=nlen_field)


def fixed(tokens, final=None, eob=True) -> dict:
    return dict(type=1, tokens=list(tokens), final=final, eob=eob)


def dynamic(tokens, litlen_lengths, dist_lengths, cl_lengths=None, cl_symbols=None, final=None, eob=True) -> dict:
    return dict(type=2, tokens=list(tokens), ll=list(litlen_lengths), dl=list(dist_lengths), cl=cl_lengths,
                cls=cl_symbols, final=final, eob=eob)


def reserved(final=None) -> dict:
    return dict(type=3, final=final)


DEFAULT_CL = [4] * 13 + [5] * 6  # a complete code over all 19 code-length symbols


def rle_symbols(lengths) -> list:
    """Code-length symbols for `lengths`: zero runs by 17 / 18, the rest as they are."""
    out, i = [], 0
    while i < len(lengths):
        if lengths[i] == 0:
            j = i
            while j < len(lengths) and lengths[j] == 0 and j - i < 138:
                j += 1
            if j - i >= 11:
                out.append((18, j - i - 11))
            elif j - i >= 3:
                out.append((17, j - i - 3))
            else:
                out += [(0, 0)] * (j - i)
            i = j
        else:
            out.append((lengths[i], 0))
            i += 1
    return out


def length_symbol(length: int):
    i = 28 if length == 258 else max(k for k in range(28) if im._LEN_BASE[k] <= length)
    return 257 + i, length - im._LEN_BASE[i], im._LEN_EXTRA[i]


def dist_symbol(dist: int):
    j = max(k for k in range(30) if im._DIST_BASE[k] <= dist)
    return j, dist - im._DIST_BASE[j], im._DIST_EXTRA[j]


def _put_tokens(bw, out, tokens, ll, dl):
    lc, dc = canonical_codes(ll), canonical_codes(dl)

    def sym(codes, lens, s):
        assert codes[s] is not None, f"symbol {s} has no code"
        bw.put_code(codes[s], lens[s])

    for t in tokens:
        if isinstance(t, int):
            sym(lc, ll, t)
            out.append(t)
        elif t[0] == "ll":      # a literal/length symbol and nothing else (286, 287, an early 256)
            sym(lc, ll, t[1])
        elif t[0] == "bits":    # raw bits
            bw.put(t[1], t[2])
        elif t[0] == "code":    # a code that belongs to no symbol: (value, bits), MSB first
            bw.put_code(t[1], t[2])
        else:
            length, dist = t[0], t[1]
            if len(t) > 2:      # (257, dist, 284): the length symbol named
                s = t[2]
                x, nx = length - im._LEN_BASE[s - 257], im._LEN_EXTRA[s - 257]
                assert 0 <= x < (1 << nx) or (nx == 0 and x == 0)
            else:
                s, x, nx = length_symbol(length)
            sym(lc, ll, s)
            if nx:
                bw.put(x, nx)
            j, y, ny = dist_symbol(dist)
            sym(dc, dl, j)
            if ny:
                bw.put(y, ny)
            assert dist <= len(out), "distance past the start (use raw tokens for that)"
            for _ in range(length):
                out.append(out[-dist])


def deflate_stream(blocks, header=b"\x78\x01", trailer=None) -> bytes:
    """zlib stream of `blocks` exactly as given.  The last block is final
    unless a block says otherwise; trailer=None: the Adler-32 of what the
    blocks decode to."""
    bw, out = im._Bits(), bytearray()
    for n, b in enumerate(blocks):
        fin = b["final"] if b["final"] is not None else n == len(blocks) - 1
        bw.put(1 if fin else 0, 1)
        bw.put(b["type"], 2)
        if b["type"] == 0:
            if bw.n:
                bw.put(0, 8 - bw.n)
            ln = len(b["data"]) if b["len_field"] is None else b["len_field"]
            bw.put(ln, 16)
            bw.put((ln ^ 0xFFFF) if b["nlen_field"] is None else b["nlen_field"], 16)
            assert bw.n == 0
            bw.buf += b["data"]
            out += b["data"]
        elif b["type"] == 1:
            _put_tokens(bw, out, b["tokens"] + ([("ll", 256)] if b["eob"] else []), FIXED_LL, FIXED_D + [5, 5])
        elif b["type"] == 2:
            ll, dl = b["ll"], b["dl"]
            cl = list(b["cl"]) if b["cl"] is not None else list(DEFAULT_CL)
            syms = b["cls"] if b["cls"] is not None else rle_symbols(ll + dl)
            ncode = max([4] + [i + 1 for i in range(19) if cl[CL_ORDER[i]]])
            bw.put(len(ll) - 257, 5)
            bw.put(len(dl) - 1, 5)
            bw.put(ncode - 4, 4)
            for i in range(ncode):
                bw.put(cl[CL_ORDER[i]], 3)
            cc = canonical_codes(cl)
            for s, x in syms:
                assert cc[s] is not None, f"code-length symbol {s} has no code"
                bw.put_code(cc[s], cl[s])
                if s >= 16:
                    bw.put(x, (2, 3, 7)[s - 16])
            _put_tokens(bw, out, b["tokens"] + ([("ll", 256)] if b["eob"] else []), ll, dl)
    body = bw.done()
    if trailer is None:
        trailer = struct.pack(">I", zlib.adler32(bytes(out)))
    return header + body + trailer


# --------------------------------------------------------------------------
# model and census
# --------------------------------------------------------------------------
class Corrupt(NamedTuple):
    reason: str


TYPES = ("stored", "fixed", "dynamic")
DOORS = ("header_cm", "header_cinfo", "header_fcheck", "header_fdict", "btype_3", "stored_len_mismatch",
         "stored_past_stream", "nlen_gt_286", "ndist_gt_30", "oversub_cl", "oversub_litlen", "oversub_dist",
         "cl_unused_code", "rep16_at_0", "repeat_past_end", "no_eob_code", "litlen_unused_code", "litlen_286",
         "litlen_287", "dist_unused_code", "dist_code_30", "dist_code_31", "dist_ge_30_check", "dist_gt_pos",
         "truncated_far", "truncated_near", "short_output")
CELLS = tuple(
    ["blk_" + t for t in TYPES] + [f"pair_{a}_{b}" for a in TYPES for b in TYPES] +
    ["blk_final_empty", "blk_nonfinal_ends_at_cap",
     "stored_len_0", "stored_len_65535", "stored_cut_by_cap", "stored_aligned"] +
    [f"stored_pad_{i}" for i in range(1, 8)] +
    ["stored_skip_in_ring", "stored_skip_restart", "stored_after_eob_at_bit7",
     "nlen_257", "nlen_286", "ndist_1", "ndist_30", "ncode_4", "ncode_19",
     "cl16_rep_3", "cl16_rep_6", "cl17_rep_3", "cl17_rep_10", "cl18_rep_11", "cl18_rep_138",
     "cl_repeat_crosses_boundary", "dist_table_all_zero", "dist_table_one_1bit", "dist_table_complete",
     "dist_table_incomplete_other", "litlen_incomplete",
     "ll_fast", "ll_walk_13", "ll_walk_14", "ll_walk_15", "ll_walk_literal", "ll_walk_length", "ll_walk_eob",
     "ll_walk_near_end", "ll_walk_at_cap",
     "run_1", "run_2_63", "run_64", "run_end_window", "run_end_nonliteral", "run_end_long_code",
     "single_literal_near_end", "full_in_literal", "full_in_long_literal"] +
    [f"refill{i}_{f}" for i in (1, 2, 3) for f in ("fired", "not_fired")] +
    [f"{p}_lane_{l}" for p in ("lenx", "dcode", "distx") for l in ("0", "63", "mid")] +
    [f"dist_walk_{i}" for i in range(10, 16)] +
    ["len_3", "len_258", "len_257_sym284", "dist_1", "dist_63", "dist_64", "dist_65", "dist_32768", "dist_eq_pos",
     "overlap_dist_lt_64", "overlap_dist_eq_64", "overlap_dist_gt_64", "no_overlap", "match_cut_by_cap",
     "match_at_cap",
     "ring_one_chunk", "ring_exact_1024", "ring_exact_2048", "ring_over_1", "ring_over_2", "ring_over_3"] +
    [f"head_{i}" for i in range(16)] + [f"nw_mod_{i}" for i in range(4)] +
    ["links_depth_le_32", "links_depth_gt_32", "links_cross_chunk", "links_left_after_doublings"] +
    ["err_" + d for d in DOORS])


class _Table:
    """A canonical code as the decoder sees it: (length, code) -> symbol."""

    def __init__(self, lengths):
        self.lengths = list(lengths)
        left = 1
        for l in range(1, 16):
            left = (left << 1) - sum(1 for x in lengths if x == l)
            if left < 0:
                break
        self.over = left < 0
        self.incomplete = left > 0
        self.map = {}
        if not self.over:
            for s, (l, c) in enumerate(zip(lengths, canonical_codes(lengths))):
                if l:
                    self.map[(l, c)] = s


class _Model:
    def __init__(self, stream: bytes, cap: int, head: int):
        self.K = kernel_constants()
        self.LANES = self.K["JP2HIP_INF_LANES"]
        self.s, self.n, self.cap, self.head = stream, len(stream), cap, head
        self.big = int.from_bytes(stream, "little")
        self.end = 8 * self.n
        self.P = 0
        self.loaded = 0
        self.out = bytearray()
        self.depth = []          # links to follow from each byte to one of known value
        self.maxdepth = 0
        self.cen = Counter()
        self.full = False

    def hit(self, cell):
        self.cen[cell] += 1

    def bits(self, q, n):
        return (self.big >> q) & ((1 << n) - 1)

    def get(self, n):
        v = self.bits(self.P, n)
        self.P += n
        return v

    def ensure(self):
        """The ring rule; returns "restart", "top_up" or None."""
        cw = self.K["kInChunkWords"]
        k = (self.P + 8 * self.head) >> 5
        what = None
        if k + 8 >= self.loaded:
            what = "top_up"
            if k >= self.loaded:
                self.loaded = k // cw * cw
                what = "restart"
            while k + 8 >= self.loaded:
                self.loaded += cw
        return what

    def decode(self, t: _Table, q):
        code, v, get = 0, (self.big >> q) & 0x7FFF, t.map.get
        for l in range(1, 16):
            code = (code << 1) | (v & 1)
            v >>= 1
            s = get((l, code))
            if s is not None:
                return s, l
        return None, 0

    def put_byte(self, v):
        self.out.append(v)
        self.depth.append(0)

    def put_match(self, length, dist):
        pos = len(self.out)
        src = pos - dist
        chunk = self.K["kLinkChunk"]
        for x in range(length):
            q = src + (x % dist if dist < length else x)
            self.out.append(self.out[q])
            d = self.depth[q] + 1
            self.depth.append(d)
            if d > self.maxdepth:
                self.maxdepth = d
        # a link crosses a k_inflate_links block when target and byte lie in different ones
        q_last = src + ((length - 1) % dist if dist < length else length - 1)
        if length and (src // chunk != pos // chunk or q_last // chunk != (pos + length - 1) // chunk):
            self.hit("links_cross_chunk")

    # ---- one Huffman block, as inf_block walks it ----
    def block(self, lt: _Table, dt: _Table, fixed_codes: bool):
        LB, DB, LANES, cap = self.K["kInfLB"], self.K["kInfDB"], self.LANES, self.cap
        o = 0

        def window():
            nonlocal o
            self.P += o
            o = 0
            self.ensure()

        def lane_cell(part):
            self.hit(f"{part}_lane_{'0' if o == 0 else '63' if o == LANES - 1 else 'mid'}")

        window()
        while True:
            if o >= LANES:
                window()
                if self.P > self.end + 64:
                    return "truncated_far"
            s, l = self.decode(lt, self.P + o)
            fast = s is not None and l <= LB
            pos = len(self.out)
            if fast and s < 256 and cap - pos >= LANES:
                run = 0
                while True:
                    self.put_byte(s)
                    self.hit("ll_fast")
                    run += 1
                    o += l
                    if o >= LANES:
                        self.hit("run_end_window")
                        break
                    s, l = self.decode(lt, self.P + o)
                    fast = s is not None and l <= LB
                    if not (fast and s < 256):
                        self.hit("run_end_nonliteral" if fast else "run_end_long_code")
                        break
                self.hit("run_1" if run == 1 else "run_64" if run == LANES else f"run_2_{LANES - 1}")
                if o >= LANES:
                    continue
                pos = len(self.out)
            elif fast and s < 256:
                self.hit("ll_fast")
                if pos >= cap:
                    self.hit("full_in_literal")
                    self.full = True
                    self.P += o + l
                    return None
                self.hit("single_literal_near_end")
                self.put_byte(s)
                o += l
                continue
            if not fast:
                if s is None:
                    return "litlen_unused_code"
                self.hit(f"ll_walk_{l}")
                self.hit("ll_walk_literal" if s < 256 else "ll_walk_eob" if s == 256 else "ll_walk_length")
                if cap - pos < LANES:
                    self.hit("ll_walk_near_end")
                if pos == cap:
                    self.hit("ll_walk_at_cap")
                if s < 256:
                    if pos >= cap:
                        self.hit("full_in_long_literal")
                        self.full = True
                        self.P += o + l
                        return None
                    self.put_byte(s)
                    o += l
                    continue
            else:
                self.hit("ll_fast")
            o += l
            if s == 256:
                self.P += o
                return None
            li = s - 257
            if li >= 29:
                return "litlen_286" if s == 286 else "litlen_287"
            for i in (1, 2, 3):
                if i == 2:
                    nl = im._LEN_EXTRA[li]
                    if nl:
                        lane_cell("lenx")
                    length = im._LEN_BASE[li] + self.bits(self.P + o, nl)
                    o += nl
                if i == 3:
                    d, dl = self.decode(dt, self.P + o)
                    if d is None:
                        five = int(format(self.bits(self.P + o, 5), "05b")[::-1], 2)
                        if fixed_codes and five >= 30:
                            return f"dist_code_{five}"
                        return "dist_unused_code"
                    if dl > DB:
                        self.hit(f"dist_walk_{dl}")
                    o += dl
                if o >= LANES:
                    self.hit(f"refill{i}_fired")
                    window()
                else:
                    self.hit(f"refill{i}_not_fired")
                if i == 2:
                    lane_cell("dcode")
            nd = im._DIST_EXTRA[d]
            if nd:
                lane_cell("distx")
            dist = im._DIST_BASE[d] + self.bits(self.P + o, nd)
            o += nd
            if dist > pos:
                return "dist_gt_pos"
            if length == 3:
                self.hit("len_3")
            if length == 258:
                self.hit("len_258")
            if length == 257 and s == 284:
                self.hit("len_257_sym284")
            if dist in (1, 63, 64, 65, 32768):
                self.hit(f"dist_{dist}")
            if dist == pos:
                self.hit("dist_eq_pos")
            cut = False
            if length > cap - pos:
                self.hit("match_at_cap" if cap == pos else "match_cut_by_cap")
                length = cap - pos
                cut = True
            if dist >= length:
                self.hit("no_overlap")
            else:
                self.hit("overlap_dist_lt_64" if dist < LANES else "overlap_dist_eq_64" if dist == LANES
                         else "overlap_dist_gt_64")
            self.put_match(length, dist)
            if cut:
                self.P += o
                self.full = True
                return None

    def run(self):
        n, cap, hit = self.n, self.cap, self.hit
        total = self.head + n
        hit(f"head_{self.head}")
        hit(f"nw_mod_{((total + 3) >> 2) % 4}")
        chunk_bytes = 4 * self.K["kInChunkWords"]
        if total <= chunk_bytes:
            hit("ring_one_chunk")
        for m in (1, 2):
            if total == m * chunk_bytes:
                hit(f"ring_exact_{m * chunk_bytes}")
            if 1 <= total - m * chunk_bytes <= 3:
                hit(f"ring_over_{total - m * chunk_bytes}")
        reason = self.walk()
        if reason is None and self.P > self.end:
            reason = "truncated_near"
        if reason is None and len(self.out) != cap:
            reason = "short_output"
        if reason is not None:
            hit("err_" + reason)
            return Corrupt(reason), dict(self.cen)
        hit("links_depth_le_32" if self.maxdepth <= (1 << self.K["kLinkDoublings"]) else "links_depth_gt_32")
        if self.maxdepth >> self.K["kLinkDoublings"]:
            hit("links_left_after_doublings")
        self.cen["max_link_depth"] = self.maxdepth
        return bytes(self.out), dict(self.cen)

    def walk(self):
        n, cap, hit = self.n, self.cap, self.hit
        if n < 2:
            return "header_fcheck"
        h0, h1 = self.s[0], self.s[1]
        if (h0 & 15) != 8:
            return "header_cm"
        if (h0 >> 4) > 7:
            return "header_cinfo"
        if ((h0 << 8) | h1) % 31:
            return "header_fcheck"
        if h1 & 0x20:
            return "header_fdict"
        self.ensure()
        self.P = 16
        last, prev, after_stored = False, None, False
        while not last:
            ring = self.ensure()
            if after_stored:
                hit("stored_skip_restart" if ring == "restart" else "stored_skip_in_ring")
            last = bool(self.get(1))
            typ = self.get(2)
            if typ == 3:
                return "btype_3"
            name = TYPES[typ]
            hit("blk_" + name)
            if prev:
                hit(f"pair_{prev}_{name}")
            pos0 = len(self.out)
            after_stored = typ == 0
            if typ == 0:
                if prev in ("fixed", "dynamic") and (self.P - 3) % 8 == 0:
                    hit("stored_after_eob_at_bit7")
                pad = -self.P % 8
                hit("stored_aligned" if pad == 0 else f"stored_pad_{pad}")
                self.P += pad
                ln, nl = self.get(16), self.get(16)
                if ln != (~nl & 0xFFFF):
                    return "stored_len_mismatch"
                at = self.P // 8
                if at + ln > n:
                    return "stored_past_stream"
                if ln == 0:
                    hit("stored_len_0")
                if ln == 65535:
                    hit("stored_len_65535")
                if ln > cap - pos0:
                    hit("stored_cut_by_cap")
                    ln = cap - pos0
                    last = True
                self.out += self.s[at:at + ln]
                self.depth += [0] * ln
                self.P += 8 * ln
            else:
                if typ == 1:
                    lt, dt = _fixed_tables()
                else:
                    nlen, ndist, ncode = self.get(5) + 257, self.get(5) + 1, self.get(4) + 4
                    for v, cells in ((nlen, (257, 286)), (ndist, (1, 30)), (ncode, (4, 19))):
                        if v in cells:
                            hit(f"{('nlen', 'ndist', 'ncode')[(cells[0] == 1) + 2 * (cells[0] == 4)]}_{v}")
                    if nlen > 286:
                        return "nlen_gt_286"
                    if ndist > 30:
                        return "ndist_gt_30"
                    self.ensure()
                    cl = [0] * 19
                    for i in range(ncode):
                        cl[CL_ORDER[i]] = self.get(3)
                    ct = _Table(cl)
                    if ct.over:
                        return "oversub_cl"
                    lens, i = [], 0
                    while len(lens) < nlen + ndist:
                        self.ensure()
                        sy, l = self.decode(ct, self.P)
                        if sy is None:
                            return "cl_unused_code"
                        self.P += l
                        if sy < 16:
                            lens.append(sy)
                            continue
                        v = 0
                        if sy == 16:
                            if not lens:
                                return "rep16_at_0"
                            v = lens[-1]
                            rep = 3 + self.get(2)
                            lo, hi = 3, 6
                        elif sy == 17:
                            rep = 3 + self.get(3)
                            lo, hi = 3, 10
                        else:
                            rep = 11 + self.get(7)
                            lo, hi = 11, 138
                        if rep in (lo, hi):
                            hit(f"cl{sy}_rep_{rep}")
                        if len(lens) + rep > nlen + ndist:
                            return "repeat_past_end"
                        if len(lens) < nlen < len(lens) + rep:
                            hit("cl_repeat_crosses_boundary")
                        lens += [v] * rep
                    if lens[256] == 0:
                        return "no_eob_code"
                    lt = _Table(lens[:nlen])
                    if lt.over:
                        return "oversub_litlen"
                    dt = _Table(lens[nlen:])
                    if dt.over:
                        return "oversub_dist"
                    if lt.incomplete:
                        hit("litlen_incomplete")
                    dl = [x for x in lens[nlen:] if x]
                    hit("dist_table_all_zero" if not dl else "dist_table_one_1bit" if dl == [1]
                        else "dist_table_incomplete_other" if dt.incomplete else "dist_table_complete")
                self.full = False
                reason = self.block(lt, dt, typ == 1)
                if reason:
                    return reason
                if self.full:
                    last = True
            if last and len(self.out) == pos0 and not self.full:
                hit("blk_final_empty")
            if not last and len(self.out) == cap:
                hit("blk_nonfinal_ends_at_cap")
            prev = name
        return None


@functools.lru_cache(maxsize=None)
def _fixed_tables():
    return _Table(FIXED_LL), _Table(FIXED_D)


def inflate_model(stream: bytes, cap: int, head: int = 0):
    """(bytes | Corrupt(reason), census) of one strip's stream that starts
    `head` bytes past a 16-byte boundary and decodes into `cap` bytes: output
    cut at cap, data after a full strip ignored, a read past the end corrupt."""
    return _Model(stream, cap, head).run()


# --------------------------------------------------------------------------
# files
# --------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    family: str
    stream: bytes
    cap: int
    good: bytes | None = None   # error cases: a good stream of the same cap


def shape_of(cap: int):
    """(width, rows per strip) of a strip of exactly cap bytes."""
    w = max(d for d in range(1, min(cap, 1024) + 1) if cap % d == 0)
    assert cap // w <= 4096, cap
    return w, cap // w


class DeflateFile(NamedTuple):
    """A Gray8 strip TIFF given by its strips' Deflate streams (each with
    whatever trailing bytes its StripByteCount covers)."""
    name: str
    w: int
    rps: int
    streams: tuple
    names: tuple
    compression: int = 8

    @property
    def h(self):
        return self.rps * len(self.streams)

    @property
    def cap(self):
        return self.w * self.rps

    def tiff(self) -> bytes:
        it = iter(self.streams)
        return im.tiff_bytes(np.zeros((self.h, self.w), np.uint8), rows_per_strip=self.rps,
                             strip_codec=lambda raw: next(it), compression=self.compression)

    def heads(self):
        off = len(self.tiff()) - sum(len(s) for s in self.streams)
        out = []
        for s in self.streams:
            out.append(off % 16)
            off += len(s)
        return out

    def model(self):
        return [inflate_model(s, self.cap, hd) for s, hd in zip(self.streams, self.heads())]

    def pixels(self) -> np.ndarray:
        got = self.model()
        assert all(isinstance(b, bytes) for b, _ in got), [b for b, _ in got if not isinstance(b, bytes)]
        return np.frombuffer(b"".join(b for b, _ in got), np.uint8).reshape(self.h, self.w)


def data_base(nstrips: int) -> int:
    """Where tiff_bytes puts the first strip of a one-component file."""
    return 8 + 2 + 12 * 11 + 4 + (8 * nstrips if nstrips > 1 else 0)


def group(cases, per_file=16, compression=8) -> list:
    """Cases of one cap, in order, as strips of files of at most per_file strips."""
    files, cur = [], []

    def flush():
        if cur:
            w, rps = shape_of(cur[0].cap)
            files.append(DeflateFile(f"{cur[0].name}..{len(cur)}", w, rps, tuple(c.stream for c in cur),
                                     tuple(c.name for c in cur), compression))
            cur.clear()

    for c in cases:
        if cur and (c.cap != cur[0].cap or len(cur) == per_file):
            flush()
        cur.append(c)
    flush()
    return files


# --------------------------------------------------------------------------
# case families
# --------------------------------------------------------------------------
def _rng(*seed):
    return np.random.default_rng([20261020, *seed])


def _lits(rng, n, lo=0, hi=256):
    return [int(v) for v in rng.integers(lo, hi, n)]


def ladder(symbols) -> list:
    """Lengths 1, 2, ..., n-1, n-1 over `symbols` in that order: a complete code."""
    n = len(symbols)
    return dict(zip(symbols, list(range(1, n)) + [n - 1]))


def lengths_of(assign: dict, size: int) -> list:
    out = [0] * size
    for s, l in assign.items():
        out[s] = l
    return out


# ---- phase: every part of a match at every lane, on both sides of kInfLanes ----
PHASE_PREFIX = 16508     # a strip is 16896 bytes: 22 rows of 768


def phase_cases(prefix_len=PHASE_PREFIX, ns=range(128), family="phase"):
    """A stored block of prefix_len bytes (16508: a 13-extra-bit distance is
    in reach), then one dynamic block: n one-bit literals, a match with 5
    length extra bits, a 15-bit distance code and 13 distance extra bits, a
    second short match, and 127 - n more of the literal, so that every strip
    has one size.  The length code starts at lane n mod 64 of its window; the
    parts after it 3, 8 and 23 bits later."""
    rng = _rng(1)
    prefix = bytes(rng.integers(0, 256, prefix_len, dtype=np.uint8))
    A = 0x41
    ll = lengths_of({A: 1, 256: 2, 284: 3, 0x42: 4, 257: 4}, 285)
    d_assign = ladder([0, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 28, 29])  # 28 and 29: 15 bits
    dl = lengths_of(d_assign, 30)
    out = []
    for n in ns:
        r = _rng(1, n)
        length = 227 + int(r.integers(0, 31))
        dist = 16385 + int(r.integers(0, 8192)) if n & 1 else 24577 + int(r.integers(0, 8192 - 400))
        dist = min(dist, prefix_len + n)
        toks = [A] * n + [(length, dist, 284), 0x42, (3, 1)] + [A] * (127 - n) + [0x42] * (257 - length)
        s = deflate_stream([stored(prefix), dynamic(toks, ll, dl)])
        out.append(Case(f"{family}_{n:03d}", family, s, prefix_len + 127 + 1 + 3 + 257))
    return out


# ---- long_codes: lengths 1..15 in both tables ----
def long_code_cases():
    """A complete code with the lengths 1..15 (and 15 twice) over 16 literal/
    length symbols and over 16 distance symbols, rotated so that every symbol
    takes every length; each strip uses every symbol of both tables."""
    lsyms = [0x10, 0x20, 0x30, 0x40, 0x50, 0x60, 0x70, 0x80, 0x90, 256, 257, 264, 270, 280, 284, 285]
    dsyms = [0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26]
    out = []
    cap = 24576
    for r in range(16):
        rng = _rng(2, r)
        la = ladder(lsyms[r:] + lsyms[:r])
        da = ladder(dsyms[(5 * r) % 16:] + dsyms[:(5 * r) % 16])
        ll, dl = lengths_of(la, 286), lengths_of(da, 30)
        toks, n = [], 0
        lits = [s for s in lsyms if s < 256]
        for _ in range(40):
            toks.append(lits[int(rng.integers(0, len(lits)))])
            n += 1
        for ds in dsyms + dsyms:
            for ls in (257, 264, 270, 280, 284, 285):
                length = im._LEN_BASE[ls - 257] + int(rng.integers(0, 1 << im._LEN_EXTRA[ls - 257]))
                lo = im._DIST_BASE[ds]
                if lo > n:
                    continue
                dist = min(n, lo + int(rng.integers(0, 1 << im._DIST_EXTRA[ds])))
                toks.append((length, dist, ls))
                n += length
                for _ in range(int(rng.integers(0, 4))):
                    toks.append(lits[int(rng.integers(0, len(lits)))])
                    n += 1
        assert n < cap - 200
        # the end of the strip: long codes with fewer than 64 bytes to go, and one at pos == cap
        toks += [lits[int(rng.integers(0, len(lits)))] for _ in range(cap - n)]
        toks += [lits[r % len(lits)], (3, 1)]   # ignored: the strip is full
        out.append(Case(f"long_codes_{r:02d}", "long_codes", deflate_stream([dynamic(toks, ll, dl)]), cap))
    return out


# ---- tables: the header's extremes ----
def expand_cl(symbols) -> list:
    """The code lengths that a code-length symbol sequence spells."""
    out = []
    for s, x in symbols:
        if s < 16:
            out.append(s)
        else:
            out += [out[-1] if s == 16 else 0] * ((3, 3, 11)[s - 16] + x)
    return out


def rle_with_16(lengths, reps=(6, 3, 4, 5)) -> list:
    """Code-length symbols that spell every run of equal lengths as the
    length, then repeats (symbol 16) of the sizes in `reps` in turn."""
    out, i, k = [], 0, 0
    while i < len(lengths):
        j = i
        while j < len(lengths) and lengths[j] == lengths[i]:
            j += 1
        out.append((lengths[i], 0))
        i += 1
        while j - i >= 3:
            r = min(reps[k % len(reps)], j - i)
            k += 1
            out.append((16, r - 3))
            i += r
        out += [(lengths[i - 1], 0)] * (j - i)
        i = j
    return out


FULL_LL = [8] * 226 + [9] * 60          # 286 literal/length codes, complete
FULL_DL = [5] * 28 + [4] * 2            # 30 distance codes, complete


def table_cases():
    out = []
    cap = 600
    rng = _rng(3)

    def case(name, block):
        out.append(Case("tables_" + name, "tables", deflate_stream([block]), cap))

    # nlen 257, ndist 1, the distance table all zero: literals only
    la = {i: 8 for i in range(255)}
    la.update({255: 9, 256: 9})
    case("nlen257_ndist1_no_distances", dynamic(_lits(rng, cap), lengths_of(la, 257), [0]))
    # one 1-bit distance code (distance 1 only) and an incomplete literal/length code whose unused codes never occur
    la = {i: 8 for i in range(254)}
    la.update({255: 10, 256: 10, 282: 10, 283: 10})
    toks = _lits(rng, 100, 0, 254) + [(180, 1, 282), 255, (200, 1, 283)] + _lits(rng, 119, 0, 254)
    case("one_distance_code_incomplete_litlen", dynamic(toks, lengths_of(la, 284), [1]))
    # nlen 286 and ndist 30, every symbol with a code; symbols 285 and 284 + 31; a match cut by the strip's end
    toks = _lits(rng, 50) + [(258, 50), (257, 49, 284), (3, 1), (100, 63), 1, 2, 3]
    case("nlen286_ndist30_complete", dynamic(toks, FULL_LL, FULL_DL))
    # symbol 16 with 3 and 6 copies, one of them from the last literal/length codes into the distance codes
    dl = [9, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    cls = rle_with_16(FULL_LL + dl)
    assert expand_cl(cls) == FULL_LL + dl
    cl = lengths_of({16: 3, 9: 3, 8: 3, 7: 3, 6: 3, 5: 3, 4: 4, 3: 4, 2: 4, 1: 4}, 19)
    toks = _lits(rng, 300) + [(258, 25), (39, 1), (3, 2)]
    case("repeats_of_16_cross_boundary", dynamic(toks, FULL_LL, dl, cl_lengths=cl, cl_symbols=cls))
    # 17 with 3 and 10 zeros, 18 with 11 and 138, an 18 from the literal/length codes into the distance codes;
    # symbol 15 has a code (ncode 19)
    cls = [(18, 54), (1, 0), (17, 7), (3, 0), (3, 0), (17, 0), (18, 127), (18, 0), (17, 7), (17, 7), (17, 3),
           (3, 0), (3, 0), (18, 22), (1, 0)]
    lens = expand_cl(cls)
    assert len(lens) == 286 + 6
    cl = lengths_of({1: 2, 3: 2, 17: 2, 18: 3, 15: 3}, 19)
    toks = [65] * 200 + [76, 77, (3, 7), 76] + [65] * (cap - 206) + [77, (3, 8)]
    case("repeats_of_17_18_cross_boundary", dynamic(toks, lens[:286], lens[286:], cl_lengths=cl, cl_symbols=cls))
    # an incomplete distance code that is not the single 1-bit one; its unused codes are never met
    case("incomplete_distance_code", dynamic(_lits(rng, cap - 40) + [(40, 2)], FULL_LL, [3, 3, 3]))
    # an incomplete code-length code
    cl = lengths_of({8: 1, 9: 2, 5: 3, 4: 4}, 19)
    case("incomplete_code_length_code", dynamic(_lits(rng, cap), FULL_LL, FULL_DL, cl_lengths=cl,
                                                cl_symbols=[(x, 0) for x in FULL_LL + FULL_DL]))
    return out


# ---- stored ----
def stored_cases():
    out = []
    rng = _rng(4)

    def rnd(n):
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))

    def case(name, blocks, cap, trailer=None):
        out.append(Case("stored_" + name, "stored", deflate_stream(blocks, trailer=trailer), cap))

    # the stored header's pad: a fixed block of k literals before it moves the block start through a byte
    for k in range(8):
        lits = [0x90] * k + [1] * 3   # 9-bit literals shift the phase one bit each
        case(f"after_{k}_nine_bit_literals", [fixed(lits), stored(rnd(600 - k - 3))], 600)
    case("aligned_after_stored", [stored(rnd(100)), stored(rnd(200)), stored(b""), stored(rnd(300))], 600)
    case("len_0_final", [fixed(_lits(rng, 600)), stored(b"")], 600)
    case("len_65535", [stored(rnd(65535)), stored(rnd(1))], 65536)
    case("len_65535_cut", [stored(rnd(65535))], 65280)
    case("cut_by_cap_then_rubbish", [stored(rnd(700), final=False), stored(rnd(50))], 600, trailer=rnd(9))
    # the skip: inside the ring (a short block), past `loaded` (a long one), each followed by a Huffman block
    case("skip_in_ring", [stored(rnd(300)), fixed(_lits(rng, 300))], 600)
    case("skip_restarts_ring", [stored(rnd(5000)), fixed(_lits(rng, 402) + [(258, 5000), (100, 64)])], 5760)
    case("skip_restarts_ring_twice", [fixed(_lits(rng, 8)), stored(rnd(2400)), dynamic(
        [65] * 100 + [(30, 1)], lengths_of({65: 1, 256: 2, 271: 2}, 272), [1]), stored(rnd(3220)), fixed([1, 2])], 5760)
    return out


# ---- blocks ----
def block_cases():
    out = []
    rng = _rng(5)

    def rnd(n):
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))

    def dyn(seed, toks_n):
        """A dynamic block over its own random alphabet: tables change from block to block."""
        r = _rng(5, seed)
        lits = sorted(set(_lits(r, 5 + seed % 7)))
        assign = ladder(list(r.permutation(lits + [256, 257 + seed % 8])))
        ll = lengths_of({int(k): v for k, v in assign.items()}, 257 + 8)
        toks = [lits[int(r.integers(0, len(lits)))] for _ in range(toks_n)]
        return dynamic(toks + [(3 + seed % 8, 1 + seed % 3)], ll, [2, 2, 2, 0, 0, 2]), toks_n + 3 + seed % 8

    def case(name, blocks, cap, trailer=None):
        out.append(Case("blocks_" + name, "blocks", deflate_stream(blocks, trailer=trailer), cap))

    kinds = ("stored", "fixed", "dynamic")
    for a in kinds:           # every ordered pair, then back
        for b in kinds:
            blocks, n = [], 0
            for i, k in enumerate((a, b, a)):
                if k == "stored":
                    blocks.append(stored(rnd(70)))
                    n += 70
                elif k == "fixed":
                    blocks.append(fixed(_lits(rng, 60) + [(10, 3)]))
                    n += 70
                else:
                    blk, m = dyn(len(out) * 3 + i, 70)
                    blocks.append(blk)
                    n += m
            blocks.append(fixed([7] * (240 - n)))
            case(f"{a}_{b}_{a}", blocks, 240)
    # what Z_SYNC_FLUSH writes, 39 times, then data
    case("39_empty_stored", [fixed(_lits(rng, 100))] + [stored(b"")] * 39 + [fixed(_lits(rng, 140))], 240)
    # 40 blocks whose tables change every time: a stale lfast / dfast entry would decode wrongly
    blocks, n = [], 0
    for i in range(39):
        blk, m = dyn(100 + i, 20 + i)
        blocks.append(blk)
        n += m
    blocks.append(fixed([3] * (2400 - n)))
    case("40_blocks_changing_tables", blocks, 2400)
    # long codes in one block, short ones in the next, on the same symbols
    la = ladder([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 256, 257, 258])
    ll = lengths_of(la, 259)
    lb = ladder([258, 257, 256, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1])
    t1 = [13, 12, 11, 1, 1, 2, (3, 1), (4, 2), 13]
    blocks = [dynamic(t1, ll, [1, 1]), dynamic(t1, lengths_of(lb, 259), [2, 1, 2]), dynamic(t1, ll, [1, 1]),
              fixed([13] * (240 - 3 * 14))]
    case("long_then_short_codes", blocks, 240)
    # empty blocks of every kind, and a final empty block
    e_dyn = dynamic([], lengths_of({256: 1, 0: 1}, 257), [0])
    case("empty_blocks", [fixed([]), e_dyn, stored(b""), fixed(_lits(rng, 240)), e_dyn, fixed([]), stored(b""),
                          dynamic([], lengths_of({256: 1}, 257), [0])], 240)
    case("final_empty_fixed", [stored(rnd(240)), fixed([])], 240)
    return out


# ---- ends ----
def end_cases():
    """Every way a strip fills up, with rubbish after it (none of it is read)."""
    out = []
    rng = _rng(6)
    cap = 400
    junk = bytes(rng.integers(0, 256, 40, dtype=np.uint8))

    def case(name, blocks, c=cap):
        s = deflate_stream(blocks, trailer=b"")
        out.append(Case("ends_" + name, "ends", s + junk, c))

    long_l = ladder([65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 256, 257, 258, 76, 77])   # 76, 77: 15 bits
    ll = lengths_of(long_l, 259)
    case("in_a_literal", [fixed(_lits(rng, cap + 5), final=False)])
    case("in_a_long_literal", [dynamic([65] * (cap - 2) + [77, 76, 77, 76], ll, [1], final=False)])
    case("in_a_match", [fixed(_lits(rng, cap - 100) + [(258, 50)], final=False)])
    case("match_starts_at_cap", [fixed(_lits(rng, cap - 100) + [(100, 50), (9, 9)], final=False)])
    case("in_a_stored_block", [fixed(_lits(rng, 100)), stored(bytes(rng.integers(0, 256, cap, dtype=np.uint8)),
                                                               final=False)])
    case("stored_starts_at_cap", [fixed(_lits(rng, cap), final=False), stored(b"abc", final=False)])
    case("block_ends_at_cap_then_literal", [fixed(_lits(rng, cap), final=False), fixed([1, 2, 3], final=False)])
    case("block_ends_at_cap_then_long_code", [fixed(_lits(rng, cap), final=False),
                                              dynamic([77, 76], ll, [1], final=False)])
    case("block_ends_at_cap_then_match", [fixed(_lits(rng, cap), final=False), fixed([(5, 5)], final=False)])
    case("block_ends_at_cap_then_empty_final", [fixed(_lits(rng, cap), final=False), fixed([])])
    case("exactly_at_final_eob", [fixed(_lits(rng, cap))])
    # the run store gives way to single literals 64 bytes before the end: 1-bit literals across that point
    one = lengths_of({65: 1, 256: 2, 66: 2}, 257)
    case("one_bit_literals_to_the_end", [dynamic([65] * (cap + 30), one, [0], final=False)])
    case("one_bit_literals_exact", [dynamic([65] * cap, one, [0])])
    lits = _lits(rng, cap)
    out.append(Case("ends_wrong_adler32", "ends", deflate_stream([fixed(lits)], trailer=b"\x12\x34\x56\x78"), cap))
    out.append(Case("ends_no_trailer", "ends", deflate_stream([fixed(lits)], trailer=b""), cap))
    out.append(Case("ends_data_after_final_block", "ends", deflate_stream([fixed(lits)]) + junk, cap))
    return out


# ---- links ----
LINK_DEPTH_BOUND = 8192


def link_cases():
    out = []
    rng = _rng(7)

    def case(name, toks, cap):
        toks = toks + _lits(rng, -cap % 16)     # (a strip of whole rows)
        out.append(Case("links_" + name, "links", deflate_stream([fixed(toks)]), cap + -cap % 16))

    # dist-1 and dist-2 runs of length-3 matches: a chain one link deeper per match
    case("dist1_len3_x8000", [0x33] + [(3, 1)] * 8000, 24001)
    case("dist2_len3_x8000", [1, 2] + [(3, 2)] * 8000, 24002)
    case("dist1_len3_x33", _lits(rng, 20) + [(3, 1)] * 33 + _lits(rng, 21), 140)       # just past 2^5
    case("dist1_len3_x32", _lits(rng, 20) + [(3, 1)] * 32 + _lits(rng, 24), 140)
    # periodic patterns across 4096-byte blocks: period 3, 64, 4095, 4096, 4097 by non-overlapping matches
    for period in (3, 64, 4095, 4096, 4097):
        toks, n = _lits(rng, period), period
        while n < 20480:
            m = min(258, period)
            toks.append((max(m, 3), period))
            n += max(m, 3)
        case(f"period_{period}", toks, n)
    # long overlapping matches across the block boundaries: dist 1, 63, 64, 65, 70
    for d in (1, 63, 64, 65, 70):
        toks, n = _lits(rng, 4000 + d), 4000 + d
        while n < 12500:
            toks.append((258, d))
            n += 258
        case(f"overlap_{d}", toks, n)
    return out


# ---- match shapes that need their own room ----
def shape_cases():
    rng = _rng(8)
    pre = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    toks = [(258, 32768), (3, 32768), 5, (257, 32768, 284), (100, 32768 + 0)]
    n = 32768 + 258 + 3 + 1 + 257 + 100
    s = deflate_stream([stored(pre), fixed(toks + [7] * (-n % 16))])
    cases = [Case("shapes_dist_32768", "shapes", s, n + -n % 16)]
    # distance equal to pos (byte 0), every small distance at length 3 and 258
    toks, n = [9, 8, (3, 2), (258, 5)], 5 + 258
    for d in (1, 2, 3, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257):
        for length in (3, 4, 63, 64, 65, 66, 128, 129, 257, 258):
            toks += [int(rng.integers(0, 256)), (length, d)]
            n += 1 + length
    toks += [7] * (-n % 16)
    cases.append(Case("shapes_small_distances", "shapes", deflate_stream([fixed(toks)]), n + -n % 16))
    toks = _lits(rng, 200) + [(200, 200), (258, 400), (3, 658), 1, 2, 3]
    cases.append(Case("shapes_dist_eq_pos", "shapes", deflate_stream([fixed(toks)]), 200 + 200 + 258 + 3 + 3))
    return cases


# ---- random ----
RANDOM_FILES, RANDOM_STRIPS = 40, 5


def random_lengths(rng, nsym: int, maxlen=15) -> list:
    """nsym code lengths of a complete code (nsym >= 2), by splitting leaves."""
    leaves = [1, 1]
    while len(leaves) < nsym:
        ok = [i for i, l in enumerate(leaves) if l < maxlen]
        i = ok[int(rng.integers(0, len(ok)))]
        l = leaves.pop(i)
        leaves += [l + 1, l + 1]
    rng.shuffle(leaves)
    return [int(x) for x in leaves]


def random_stream(rng, cap: int) -> bytes:
    blocks, hist = [], 0
    while hist < cap:
        left = cap - hist
        kind = int(rng.integers(0, 4))
        want = int(min(left, rng.integers(1, 300)))
        if rng.random() < 0.15:
            want = left
        if kind == 0:
            blocks.append(stored(bytes(rng.integers(0, 256, want, dtype=np.uint8))))
            hist += want
            continue
        if kind == 1:
            lit_syms, len_syms, dist_syms = list(range(256)), list(range(257, 286)), list(range(30))
            ll = dl = None
        else:
            lit_syms = sorted(set(_lits(rng, int(rng.integers(1, 60)))))
            len_syms = sorted(set(int(v) for v in rng.integers(257, 286, int(rng.integers(0, 8)))))
            dist_syms = sorted(set(int(v) for v in rng.integers(0, 30, int(rng.integers(1, 10))))) if len_syms else []
            syms = lit_syms + [256] + len_syms
            maxlen = 15 if rng.random() < 0.5 else 9
            ll = lengths_of(dict(zip(syms, random_lengths(rng, len(syms), maxlen))), max(syms) + 1)
            if len(dist_syms) >= 2:
                dl = lengths_of(dict(zip(dist_syms, random_lengths(rng, len(dist_syms), maxlen))), max(dist_syms) + 1)
            elif dist_syms:
                dl = lengths_of({dist_syms[0]: 1}, dist_syms[0] + 1)
            else:
                dl = [0]
        toks, made = [], 0
        while made < want:
            room = want - made
            pos = hist + made
            ok_d = [d for d in dist_syms if im._DIST_BASE[d] <= pos]
            ok_l = [s for s in len_syms if im._LEN_BASE[s - 257] + (1 << im._LEN_EXTRA[s - 257]) - 1 <= room]
            if ok_d and ok_l and rng.random() < 0.4:
                s = ok_l[int(rng.integers(0, len(ok_l)))]
                d = ok_d[int(rng.integers(0, len(ok_d)))]
                length = im._LEN_BASE[s - 257] + int(rng.integers(0, 1 << im._LEN_EXTRA[s - 257]))
                if s == 284:
                    length = min(length, 257) if rng.random() < 0.9 else 257
                dist = min(pos, im._DIST_BASE[d] + int(rng.integers(0, 1 << im._DIST_EXTRA[d])))
                toks.append((length, dist, s))
                made += length
            else:
                toks.append(lit_syms[int(rng.integers(0, len(lit_syms)))])
                made += 1
        blocks.append(fixed(toks) if kind == 1 else dynamic(toks, ll, dl))
        hist += made
    return deflate_stream(blocks)


@functools.lru_cache(maxsize=None)
def random_file(i: int) -> DeflateFile:
    w, rps = 64 + i, 8
    rng = _rng(9, i)
    streams = []
    for s in range(RANDOM_STRIPS):
        z = random_stream(rng, w * rps)
        streams.append(z + bytes(rng.integers(0, 256, int(rng.integers(0, 3)), dtype=np.uint8)))
    return DeflateFile(f"random_{i:02d}", w, rps, tuple(streams), tuple(f"random_{i:02d}_{s}" for s in range(5)),
                       8 if i & 1 else 32946 if i == 0 else 8)


# ---- align ----
def _literal_stream(rng, cap, nbytes):
    """One fixed block of cap literals and no trailer, exactly nbytes long:
    each literal >= 144 costs a ninth bit."""
    for high in range(cap + 1):
        if 2 + (10 + 8 * cap + high + 7) // 8 == nbytes:
            toks = _lits(rng, high, 144, 256) + _lits(rng, cap - high, 0, 144)
            toks = [toks[i] for i in rng.permutation(cap)]
            s = deflate_stream([fixed(toks)], trailer=b"")
            assert len(s) == nbytes
            return s
    raise AssertionError((cap, nbytes))


@functools.lru_cache(maxsize=None)
def align_files():
    """(a) 16 strips beginning at every residue modulo 16; (b), (c) strips whose
    streams end exactly at, and 1 to 3 bytes past, 1024 and 2048 bytes from
    the aligned base, the last byte holding the end-of-block code."""
    files = []
    rng = _rng(10)
    w, rps = 50, 8
    off = data_base(16)
    streams = []
    for i in range(16):
        z = random_stream(rng, w * rps)
        want_next = (data_base(16) + 7 * (i + 1)) % 16     # 7 is a unit modulo 16: every residue once
        z += b"\0" * ((want_next - (off + len(z))) % 16)
        streams.append(z)
        off += len(z)
    files.append(DeflateFile("align_residues", w, rps, tuple(streams), tuple(f"align_residue_{i:02d}" for i in range(16))))
    for total, cap in ((1024, 960), (2048, 1950)):
        targets = [total - 1, total, total + 1, total + 2, total + 3, total, total + 1, total + 2, total + 3]
        off = data_base(len(targets))
        streams = []
        for t in targets:
            z = _literal_stream(rng, cap, t - off % 16)
            streams.append(z)
            off += len(z)
        wd, r = shape_of(cap)
        files.append(DeflateFile(f"align_{total}", wd, r, tuple(streams),
                                 tuple(f"align_{total}_{'m1' if t < total else 'p%d' % (t - total)}_{i}"
                                       for i, t in enumerate(targets))))
    return files


# ---- tiles, Predictor 2, and crafted strips next to zlib's ----
def _restart_stream(cap: int, seed: int) -> bytes:
    """A fixed block, a stored block long enough that the skip past it restarts
    the ring, and a dynamic block with long codes after it."""
    rng = _rng(13, seed)
    la = ladder([65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 256, 257, 258, 76, 77])
    tail = [65, 77, 76, (3, 1), 66, 67, (4, 2), 75, 74, 73, 72, 71, 70, 69, 68, 77]
    n_tail = len(tail) + 3 + 4 - 2
    return deflate_stream([fixed(_lits(rng, 9)), stored(bytes(rng.integers(0, 256, cap - 9 - n_tail, dtype=np.uint8))),
                           dynamic(tail, lengths_of(la, 259), [1, 1])])


@functools.lru_cache(maxsize=None)
def tile_files() -> tuple:
    """(name, TIFF, pixels): a representative of phase, long_codes and stored
    as the tiles of a tiled file, plain and with Predictor 2 (the pixels are
    then the running sums of what the streams decode to)."""
    reps = {
        "phase": (256, 80, [c.stream for c in phase_cases(256 * 80 - 388, (5, 63, 64, 100), "phase_tile")]),
        "long_codes": (512, 48, [c.stream for c in long_code_cases()[3:6]]),
        "stored": (128, 48, [_restart_stream(128 * 48, i) for i in range(3)]),
    }
    out = []
    for fam, (tw, th, streams) in reps.items():
        raw = [inflate_model(z, tw * th)[0] for z in streams]
        assert all(isinstance(b, bytes) for b in raw), fam
        tiles = np.frombuffer(b"".join(raw), np.uint8).reshape(len(streams) * th, tw)
        for predictor in (1, 2):
            px = np.cumsum(tiles, axis=1, dtype=np.uint8) if predictor == 2 else tiles
            it = iter(streams)
            tif = im.tiled_tiff_bytes(px, tile=(tw, th), codec=lambda raw_tile: next(it), compression=8,
                                      predictor=predictor)
            out.append((f"{fam}_tiles" + ("_predictor2" if predictor == 2 else ""), tif, np.ascontiguousarray(px)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed_file() -> DeflateFile:
    """Crafted strips and zlib's own (levels 0, 1, 9) in turn, in one file."""
    crafted = table_cases()
    cap = crafted[0].cap
    rng = _rng(14)
    streams, names = [], []
    for i, c in enumerate(crafted):
        raw = bytes(np.repeat(rng.integers(0, 256, cap // 4, dtype=np.uint8), 4))
        streams += [c.stream, zlib.compress(raw, (0, 1, 9)[i % 3])]
        names += ["mixed_" + c.name, f"mixed_zlib_{i}"]
    w, rps = shape_of(cap)
    return DeflateFile("mixed", w, rps, tuple(streams), tuple(names))


# ---- errors: one stream per door, each with a good stream of the same cap ----
def error_cases():
    out = []
    rng = _rng(11)
    cap = 320
    lits = _lits(rng, cap)
    good_blocks = [fixed(lits[:100]), stored(bytes(lits[100:200])), fixed(lits[200:])]
    good = deflate_stream(good_blocks)

    def case(name, stream, g=good, c=cap):
        out.append(Case("errors_" + name, "errors", stream, c, g))

    def hdr(cmf, flg_base):
        flg = flg_base + (31 - ((cmf << 8) | flg_base) % 31) % 31
        return bytes([cmf, flg])

    case("header_cm", hdr(0x79, 0) + good[2:])
    case("header_cinfo", hdr(0x88, 0) + good[2:])
    case("header_fcheck", b"\x78\x02" + good[2:])
    case("header_fdict", hdr(0x78, 0x20) + good[2:])
    case("btype_3", deflate_stream([fixed(lits[:100]), reserved()]))
    case("stored_len_mismatch", deflate_stream([fixed(lits[:100]), stored(bytes(lits[100:]), nlen_field=0x1234)]))
    z = deflate_stream([fixed(lits[:100]), stored(bytes(lits[100:]))], trailer=b"")
    case("stored_past_stream", z[:-1])
    full_ll = FULL_LL
    case("nlen_gt_286", deflate_stream([dynamic(lits, full_ll + [8], [5] * 30)]))
    case("ndist_gt_30", deflate_stream([dynamic(lits, full_ll, [5] * 31)]))
    cl_over = [4] * 13 + [5] * 5 + [2]
    case("oversub_cl", deflate_stream([dynamic(lits, full_ll, [5] * 30, cl_lengths=cl_over)]))
    case("oversub_litlen", deflate_stream([dynamic(lits, [8] * 227 + [9] * 59, [5] * 30)]))
    case("oversub_dist", deflate_stream([dynamic(lits, full_ll, [5] * 26 + [4] * 4)]))
    # a code-length code with an unused code: lengths 1, 2, 3 over {8, 9, 7}: 111 is no code
    cl = [0] * 19
    cl[8], cl[9], cl[7] = 1, 2, 3
    case("cl_unused_code", _raw_dynamic_header(286, 30, cl, [("sym", 8)] * 5 + [("code", 0b111, 3)]))
    cl16 = [0] * 19
    cl16[16], cl16[8] = 1, 1
    case("rep16_at_0", _raw_dynamic_header(286, 30, cl16, [("sym", 16, 0)]))
    cl18 = [0] * 19
    cl18[18], cl18[8] = 1, 1
    case("repeat_past_end", _raw_dynamic_header(257, 1, cl18, [("sym", 18, 127), ("sym", 8), ("sym", 18, 127)]))
    ll = [8] * 256 + [0]
    case("no_eob_code", deflate_stream([dynamic(lits, ll, [0], eob=False)]))
    # ncode 4: only 16, 17, 18 and 0 can have codes, so every length is 0 and there is no code for 256
    cl4 = [0] * 19
    cl4[0], cl4[18], cl4[17] = 1, 2, 2
    case("no_eob_code_ncode_4", _raw_dynamic_header(257, 1, cl4, [("sym", 18, 127), ("sym", 18, 98)], ncode=4))
    inc = lengths_of({i: 8 for i in range(200)}, 257)
    inc[256] = 8
    small = [v % 200 for v in lits]
    case("litlen_unused_code", deflate_stream([dynamic(small[:100] + [("code", 0xFF, 8)] + small[100:], inc, [0])]),
         g=deflate_stream([dynamic(small, inc, [0])]))
    case("litlen_286", deflate_stream([fixed(lits[:100] + [("ll", 286)] + lits[100:])]))
    case("litlen_287", deflate_stream([fixed(lits[:100] + [("ll", 287)] + lits[100:])]))
    case("dist_unused_code", deflate_stream([dynamic(lits[:100] + [("ll", 257), ("code", 0b1, 1)] + lits[100:],
                                                     full_ll, [1])]))
    case("dist_all_zero_table_match", deflate_stream([dynamic(lits[:100] + [("ll", 257), ("bits", 0, 5)] + lits[100:],
                                                              full_ll, [0])]))
    case("dist_code_30", deflate_stream([fixed(lits[:100] + [("ll", 257), ("code", 30, 5)] + lits[100:])]))
    case("dist_code_31", deflate_stream([fixed(lits[:100] + [("ll", 257), ("code", 31, 5)] + lits[100:])]))
    case("dist_gt_pos", deflate_stream([fixed(lits[:100] + [("ll", 257), ("code", 14, 5), ("bits", 0, 6)] + lits[100:])]))
    case("dist_gt_pos_at_0", deflate_stream([fixed([("ll", 257), ("code", 0, 5)] + lits)]))
    one = lengths_of({65: 1, 256: 2, 66: 2}, 257)   # zeros past the end read as literals: the walk runs on
    z = deflate_stream([dynamic([65, 66, 66, 65] * (cap // 4), one, [0])])
    case("truncated_far", z[:len(z) // 2], g=z)
    z = deflate_stream([fixed(lits)], trailer=b"")
    case("truncated_near", z[:-1])
    case("truncated_near_4_bytes", z[:-4])
    case("short_output", deflate_stream([fixed(lits[:-1])]))
    case("short_output_empty", deflate_stream([stored(b"")]))
    return out


def _raw_dynamic_header(nlen, ndist, cl, items, ncode=None) -> bytes:
    """A zlib stream that ends inside a dynamic block's header: the counts,
    the code-length code lengths, then `items`: ("sym", s[, extra]) or
    ("code", value, bits); zeros follow."""
    bw = im._Bits()
    bw.put(1, 1)
    bw.put(2, 2)
    bw.put(nlen - 257, 5)
    bw.put(ndist - 1, 5)
    if ncode is None:
        ncode = max([4] + [i + 1 for i in range(19) if cl[CL_ORDER[i]]])
    bw.put(ncode - 4, 4)
    for i in range(ncode):
        bw.put(cl[CL_ORDER[i]], 3)
    cc = canonical_codes(cl)
    for it in items:
        if it[0] == "code":
            bw.put_code(it[1], it[2])
        else:
            bw.put_code(cc[it[1]], cl[it[1]])
            if it[1] >= 16:
                bw.put(it[2], (2, 3, 7)[it[1] - 16])
    return b"\x78\x01" + bw.done() + b"\0" * 64


# --------------------------------------------------------------------------
# the corpus
# --------------------------------------------------------------------------
FAMILIES = ("phase", "long_codes", "tables", "stored", "blocks", "ends", "links", "shapes", "align", "random", "errors")


@functools.lru_cache(maxsize=None)
def valid_cases() -> tuple:
    """The named valid cases (align and random come as whole files)."""
    return tuple(phase_cases() + long_code_cases() + table_cases() + stored_cases() + block_cases() + end_cases() +
                 link_cases() + shape_cases())


@functools.lru_cache(maxsize=None)
def valid_files() -> tuple:
    """Every valid case as a strip of some file; one file per family is
    tagged 32946, the older Deflate code."""
    files = []
    for fam in FAMILIES:
        cs = [c for c in valid_cases() if c.family == fam]
        fs = group(cs)
        if fs:
            fs[0] = fs[0]._replace(compression=32946)
        files += fs
    a = list(align_files())
    a[0] = a[0]._replace(compression=32946)
    files += a
    files += [random_file(i) for i in range(RANDOM_FILES)]
    return tuple(files)


@functools.lru_cache(maxsize=None)
def error_pairs() -> tuple:
    """(name, bad file, good file): two strips, the second one at fault."""
    out = []
    rng = _rng(12)
    for c in error_cases():
        w, rps = shape_of(c.cap)
        s0 = random_stream(rng, c.cap)
        bad = DeflateFile(c.name, w, rps, (s0, c.stream), (c.name + "_neighbour", c.name))
        good = DeflateFile(c.name + "_good", w, rps, (s0, c.good), (c.name + "_neighbour", c.name + "_good"))
        out.append((c.name, bad, good))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def measured() -> dict:
    """{strip name: (bytes | Corrupt, census, stream, cap, head)} over the whole corpus."""
    rows = {}
    for f in valid_files():
        for name, s, hd, (res, cen) in zip(f.names, f.streams, f.heads(), f.model()):
            assert name not in rows, name
            rows[name] = (res, cen, s, f.cap, hd)
    for name, bad, good in error_pairs():
        (_, (res, cen)), hd = list(zip(bad.names, bad.model()))[1], bad.heads()[1]
        rows[name] = (res, cen, bad.streams[1], bad.cap, hd)
        g = good.model()[1]
        rows[name + "_good"] = (g[0], g[1], good.streams[1], good.cap, good.heads()[1])
    return rows


def totals(rows=None) -> dict:
    tot = dict.fromkeys(CELLS, 0)
    for res, cen, *_ in (rows or measured()).values():
        for k, v in cen.items():
            if k != "max_link_depth":
                assert k in tot, k
                tot[k] += v
    return tot


def _row(cen: dict) -> list:
    """A census row as [cell index, count, ...] (indices into CELLS)."""
    out = []
    for i, k in enumerate(CELLS):
        if cen.get(k):
            out += [i, cen[k]]
    return out + [-1, cen.get("max_link_depth", 0)]


def pins() -> dict:
    """Per file of the corpus: the SHA-256 of what its strips decode to and
    the census of its strips added up; per error stream: the reason and its
    census row."""
    files = {}
    for f in valid_files():
        got = f.model()
        cen = Counter()
        for _, c in got:
            cen.update({k: v for k, v in c.items() if k != "max_link_depth"})
        cen["max_link_depth"] = max(c.get("max_link_depth", 0) for _, c in got)
        files[f.names[0] + ("" if len(f.names) == 1 else f"..{f.names[-1]}")] = {
            "strips": len(f.names), "cap": f.cap, "sha256": hashlib.sha256(b"".join(b for b, _ in got)).hexdigest(),
            "census": _row(cen)}
    errors = {}
    for name, bad, good in error_pairs():
        res, cen = bad.model()[1]
        errors[name] = {"expect": "corrupt: " + res.reason, "census": _row(cen),
                        "good_sha256": hashlib.sha256(good.model()[1][0]).hexdigest()}
    return {"constants": kernel_constants(), "cells": list(CELLS), "totals": totals(), "files": files,
            "errors": errors}


def pins_text() -> str:
    return json.dumps(pins(), separators=(",", ":"), sort_keys=True) + "\n"


def tiff_units(data: bytes) -> list:
    """[(stream, decoded size, offset modulo 16)] of the strips or tiles of a classic or Big TIFF
    with Compression 8 or 32946 (none otherwise): what a Deflate stream of
    some other writer looks like to the model."""
    e = "<" if data[:2] == b"II" else ">"
    big = struct.unpack(e + "H", data[2:4])[0] == 43
    ifd = struct.unpack(e + "Q", data[8:16])[0] if big else struct.unpack(e + "I", data[4:8])[0]
    n = struct.unpack(e + ("Q" if big else "H"), data[ifd:ifd + (8 if big else 2)])[0]
    base, size, inline = ifd + (8 if big else 2), (20 if big else 12), (8 if big else 4)
    tags = {}
    for i in range(n):
        p = base + i * size
        t, typ = struct.unpack(e + "HH", data[p:p + 4])
        cnt = struct.unpack(e + ("Q" if big else "I"), data[p + 4:p + 4 + inline])[0]
        fmt = {1: "B", 2: "B", 3: "H", 4: "I", 16: "Q"}.get(typ)
        if fmt is None:
            continue
        nb = struct.calcsize(fmt) * cnt
        v = p + 4 + inline
        if nb > inline:
            v = struct.unpack(e + ("Q" if big else "I"), data[v:v + inline])[0]
        tags[t] = struct.unpack(e + fmt * cnt, data[v:v + nb])
    if tags.get(259, (1,))[0] not in (8, 32946):
        return []
    w, h = tags[256][0], tags[257][0]
    spp = tags.get(277, (1,))[0]
    bits = tags.get(258, (1,))[0]
    per_px = bits * (1 if tags.get(284, (1,))[0] == 2 else spp)
    if 322 in tags:
        tw, th = tags[322][0], tags[323][0]
        return [(data[o:o + c], (tw * per_px + 7) // 8 * th, o % 16) for o, c in zip(tags[324], tags[325])]
    rps = min(tags.get(278, (h,))[0], h)
    per_plane = -(-h // rps)
    row = (w * per_px + 7) // 8
    return [(data[o:o + c], min(rps, h - (i % per_plane) * rps) * row, o % 16)
            for i, (o, c) in enumerate(zip(tags[273], tags[279]))]


if __name__ == "__main__":
    text = pins_text()
    with open(PINS, "w") as f:
        f.write(text)
    tot = totals()
    print(f"{len(measured())} streams in {len(valid_files())} files and {len(error_pairs())} error pairs, "
          f"{len(text)} bytes of pins; empty cells:", [k for k, v in tot.items() if not v])
    sys.exit(0)
