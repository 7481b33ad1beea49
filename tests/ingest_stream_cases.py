"""Crafted LZW and PackBits streams, and TIFF layouts no encoder-written
fixture expresses, for test_ingest_streams.py and test_gpu_ingest_streams.py.

Everything is built from seeds; nothing here imports the product.

* lzw_pack writes any list of codes with the decoder's width rule;
  lzw_model restates libtiff's decoding rules in plain Python (one string per
  code); lzw_random_codes draws code streams that no encoder wrote.
  test_ingest_streams.py pins the model to Pillow's libtiff on every stream
  libtiff accepts.  Two kinds of stream the model (and the product) read and
  libtiff 4.7.1 refuses, each pinned as refused:
    - a stream that does not begin with a Clear code: the model decodes it
      as if a Clear had come first (next free entry 258, 9-bit codes);
      libtiff reports a corrupted table;
    - a segment that goes on for thousands of codes after the table is full
      (entry 4095 defined) without a Clear: the model keeps the full table
      and 12-bit codes for as long as the codes last; libtiff gives up when
      its table, 1024 entries longer, overflows (a segment of about 4860
      codes; one of 4097, which the product decodes serially, it reads).
* packbits_runs writes what a real PackBits encoder writes (replicate runs,
  literal runs, both at their maximum of 128, no-ops, rows packed
  separately); packbits_model is its reference decoder.
* LAYOUT_CASES is a pairwise-covering matrix of Predictor 2 files over codec
  x layout x sample type x components; PACKED_CASES are 1-/4-bit and palette
  files through packbits_runs, and two with LZW tiles."""
from __future__ import annotations

import functools
import itertools
import zlib
from typing import NamedTuple

import numpy as np

import imaging as im
import pixel_format_cases as pf

CLEAR, EOI = 256, 257
LZW, DEFLATE, PACKBITS = 5, 8, 32773
SEG_MAX = 4096  # codes of a segment the segment-parallel route holds (csrc/lzw.hip kLzwSegMax)


# ----------------------------------------------------------------------------
# LZW
# ----------------------------------------------------------------------------
def lzw_width(k: int) -> int:
    """Bits of the k-th code after a Clear (k = 0: the first)."""
    return 9 if k < 254 else 10 if k < 766 else 11 if k < 1790 else 12


def lzw_pack(codes) -> bytes:
    """`codes` (any values below 4096, Clear = 256 and EOI = 257 among
    them) MSB-first: a code is lzw_width(k) bits wide, k counting the codes
    since the last Clear (a Clear or EOI is written at the width of the code
    it stands in for); the last byte is padded with zeros."""
    acc, nacc, k, out = 0, 0, 0, bytearray()
    for c in codes:
        w = lzw_width(k)
        assert 0 <= c < (1 << w), f"code {c} does not fit {w} bits"
        acc = (acc << w) | c
        nacc += w
        while nacc >= 8:
            nacc -= 8
            out.append((acc >> nacc) & 0xFF)
        acc &= (1 << nacc) - 1
        k = 0 if c == CLEAR else k + 1
    if nacc:
        out.append((acc << (8 - nacc)) & 0xFF)
    return bytes(out)


def lzw_greedy(data: bytes, clear_every: int | None = None, clear_when_full: bool = True) -> list:
    """The codes imaging.lzw_encode writes for `data` (longest match first),
    as a list: [Clear, ..., EOI]."""
    codes, table, k, cur = [CLEAR], {}, 0, b""
    for byte in data:
        nxt = cur + bytes([byte])
        if not cur or nxt in table:
            cur = nxt
            continue
        codes.append(cur[0] if len(cur) == 1 else table[cur])
        if 258 + k <= 4095:
            table[nxt] = 258 + k
        k += 1
        if (clear_every and k >= clear_every) or (258 + k > 4095 and clear_when_full):
            codes.append(CLEAR)
            table, k = {}, 0
        cur = bytes([byte])
    if cur:
        codes.append(cur[0] if len(cur) == 1 else table[cur])
    codes.append(EOI)
    return codes


def _code_at(stream: bytes, bit: int, w: int) -> int:
    o = bit >> 3
    v = int.from_bytes(stream[o:o + 3].ljust(3, b"\0"), "big")
    return (v >> (24 - (bit & 7) - w)) & ((1 << w) - 1)


def lzw_model(stream: bytes, cap: int) -> tuple[bytes, str]:
    """What a strip of `cap` bytes holds after decoding `stream`, by libtiff's
    rules, and how the decode ended:
      "ok"    cap bytes exist (decoding stops there: whatever follows, valid
              or not, is never looked at; a string that crosses cap is cut);
      "bad"   a code that names an entry not yet defined (after a Clear: any
              code above 257) came before that;
      "short" EOI, or the end of the codes, came before that;
      "old"   the stream starts with byte 0 and an odd byte: the LSB-first
              LZW of before TIFF 6.0.
    Entry 258 + i is the string of code i plus the first byte of the string
    of code i + 1 (counting from the last Clear); the code one past the last
    defined entry stands for the previous string plus its own first byte
    (KwKwK).  Once entry 4095 is defined the table stays as it is.  A stream
    without a leading Clear is read as if it had one (libtiff refuses it)."""
    if len(stream) >= 2 and stream[0] == 0 and stream[1] & 1:
        return b"", "old"
    out = bytearray()
    entries, prev, k, bit = [], None, 0, 0
    while len(out) < cap:
        w = lzw_width(k)
        if bit + w > 8 * len(stream):
            return bytes(out), "short"
        code = _code_at(stream, bit, w)
        bit += w
        if code == EOI:
            return bytes(out), "short"
        if code == CLEAR:
            entries, prev, k = [], None, 0
            continue
        room = 258 + len(entries) <= 4095
        if code < 256:
            s = bytes([code])
        elif code - 258 < len(entries):
            s = entries[code - 258]
        elif code - 258 == len(entries) and prev is not None and room:
            s = prev + prev[:1]
        else:
            return bytes(out), "bad"
        out += s
        if prev is not None and room:
            entries.append(prev + s[:1])
        prev = s
        k += 1
    return bytes(out[:cap]), "ok"


def lzw_segments(stream: bytes) -> list:
    """Codes in each non-empty run between Clears, up to EOI or the end of
    the bits: what decides a strip's route."""
    segs, k, bit = [], 0, 0
    while True:
        w = lzw_width(k)
        if bit + w > 8 * len(stream):
            break
        code = _code_at(stream, bit, w)
        bit += w
        if code in (CLEAR, EOI):
            if k:
                segs.append(k)
            k = 0
            if code == EOI:
                break
        else:
            k += 1
    if k:
        segs.append(k)
    return segs


def lzw_route(stream: bytes) -> str:
    """"parallel" or "serial": lzw.hip's rule restated (a strip whose segment
    table holds len / 512 + 64 segments of at most 4096 codes is decoded
    segment-parallel; any other strip by the serial decoder)."""
    segs = lzw_segments(stream)
    return "serial" if len(segs) > len(stream) // 512 + 64 or max(segs, default=0) > SEG_MAX else "parallel"


def lzw_random_codes(rng, cap: int, p_lit=0.35, p_cur=0.1, p_clear=0.01, clear_at=(), eoi=True,
                     leading_clears=1) -> list:
    """A valid code stream for a strip of `cap` bytes that no encoder wrote:
    each code is a literal (p_lit), the entry being defined (p_cur, where
    there is one) or any entry defined so far.  The first len(clear_at)
    segments are cut by a Clear after exactly clear_at[i] codes; after that a
    Clear falls before any code with p_clear.  The codes stop with the one
    that reaches cap (its string may cross it).  "ok" by construction."""
    codes = [CLEAR] * leading_clears
    forced = list(clear_at)
    elen, prev, k, made = [], 0, 0, 0  # lengths of the entries, of the previous string
    while made < cap:
        if (forced and k == forced[0]) or (not forced and k and rng.random() < p_clear):
            codes.append(CLEAR)
            if forced:
                forced.pop(0)
            elen, prev, k = [], 0, 0
            continue
        room = 258 + len(elen) <= 4095
        r = rng.random()
        if r < p_cur and prev and room:
            code, n = 258 + len(elen), prev + 1
        elif r < p_cur + p_lit or not elen:
            code, n = int(rng.integers(0, 256)), 1
        else:
            e = int(rng.integers(0, len(elen)))
            code, n = 258 + e, elen[e]
        codes.append(code)
        made += n
        if prev and room:
            elen.append(prev + 1)
        prev = n
        k += 1
    assert not forced, f"cap {cap} reached before the Clear after {forced[0]} codes"
    if eoi:
        codes.append(EOI)
    return codes


class StripFile(NamedTuple):
    """A Gray8 strip TIFF given by its strips' code streams."""
    w: int
    h: int
    rps: int
    streams: tuple
    compression: int = LZW

    def caps(self):
        return [min(self.rps, self.h - y) * self.w for y in range(0, self.h, self.rps)]

    def tiff(self) -> bytes:
        assert len(self.streams) == len(self.caps())
        it = iter(self.streams)
        return im.tiff_bytes(np.zeros((self.h, self.w), np.uint8), rows_per_strip=self.rps, strip_codec=lambda raw: next(it),
                      compression=self.compression)

    def model(self):
        fn = lzw_model if self.compression == LZW else packbits_model
        return [fn(s, cap) for s, cap in zip(self.streams, self.caps())]

    def pixels(self) -> np.ndarray:
        got = self.model()
        assert all(st == "ok" for _, st in got), [st for _, st in got]
        return np.frombuffer(b"".join(b for b, _ in got), np.uint8).reshape(self.h, self.w)

    def offsets(self):
        """Where the strips lie in tiff() (they follow each other at the end)."""
        end = len(self.tiff())
        total = sum(len(s) for s in self.streams)
        return list(itertools.accumulate([end - total] + [len(s) for s in self.streams[:-1]]))


def _one_strip(w, h, codes_or_stream):
    s = codes_or_stream if isinstance(codes_or_stream, bytes) else lzw_pack(codes_or_stream)
    return StripFile(w, h, h, (s,))


def _px(h, w, seed):
    """Blocky 8-bit content with noise: matches of many lengths."""
    return pf.indices(h, w, 8, seed)


def flat_codes(n: int, v: int = 0x5A, eoi=True) -> list:
    """Clear, a literal, then n - 1 times "the entry being defined": string i
    is i + 1 bytes of v, n (n + 1) / 2 bytes in all, parent depth n - 1."""
    assert 1 <= n <= 3838
    return [CLEAR, v] + list(range(258, 257 + n)) + ([EOI] if eoi else [])


def _flat(n, w, h):
    assert (n - 1) * n // 2 < w * h <= n * (n + 1) // 2  # the strip ends inside the last string
    return _one_strip(w, h, flat_codes(n))


THREE_WAYS = ("parallel", "long", "clear3")


def three_ways(raw: bytes, form: str) -> bytes:
    """The same bytes as a stream of the parallel route (greedy, libtiff's
    own shape), as one segment of len(raw) literals (serial when that is
    more than 4096), or with a Clear every 3 codes (serial: more segments
    than the strip's slice of the segment table)."""
    if form == "parallel":
        return lzw_pack(lzw_greedy(raw))
    if form == "long":
        return lzw_pack([CLEAR] + list(raw) + [EOI])
    return lzw_pack(lzw_greedy(raw, clear_every=3))


def three_ways_file(forms, w=100, rps=45, h=265, seed=901):
    px = _px(h, w, seed)
    strips = [px[y:y + rps].tobytes() for y in range(0, h, rps)]
    return StripFile(w, h, rps, tuple(three_ways(s, forms[i % len(forms)]) for i, s in enumerate(strips)))


def _random_file(i: int) -> StripFile:
    """Random stream file i of 40: width 64 + i, 40 rows, 5 strips."""
    w, h, rps = 64 + i, 40, 8
    rng = np.random.default_rng([20261019, i])
    streams = []
    for s in range(5):
        mode = (i + s) % 5
        if mode == 0:  # a Clear exactly at the first width change
            codes = lzw_random_codes(rng, rps * w, p_lit=0.9, p_cur=0.03, clear_at=(254,), eoi=bool(s & 1))
        elif mode == 1:  # KwKwK-heavy
            codes = lzw_random_codes(rng, rps * w, p_lit=0.1, p_cur=0.6, p_clear=0.02)
        elif mode == 2:  # many Clears, some consecutive
            codes = lzw_random_codes(rng, rps * w, p_lit=0.5, p_cur=0.1, p_clear=0.2, leading_clears=2, eoi=False)
        else:
            codes = lzw_random_codes(rng, rps * w, p_lit=float(rng.uniform(0.05, 0.7)), p_cur=float(rng.uniform(0, 0.3)),
                                     p_clear=float(rng.uniform(0, 0.03)), eoi=bool(rng.integers(0, 2)))
        streams.append(lzw_pack(codes))
    return StripFile(w, h, rps, tuple(streams))


RANDOM_LZW = 40


@functools.lru_cache(maxsize=None)
def random_lzw_file(i: int) -> StripFile:
    return _random_file(i)


def _rng(seed):
    return np.random.default_rng([20261019, 7, seed])


def _garbage_after_full():
    """A full strip, then codes that are not defined, a Clear, more rubbish
    and no EOI: none of it is read."""
    raw = _px(40, 96, 911).tobytes()
    codes = lzw_greedy(raw)[:-1] + [4000, 3000, CLEAR, 300, 511, 258, 1, 2, 3]
    return _one_strip(96, 40, codes)


def _consecutive_clears():
    raw = _px(40, 96, 912).tobytes()
    a = lzw_greedy(raw[:1500])[:-1]
    b = lzw_greedy(raw[1500:])
    return _one_strip(96, 40, [CLEAR, CLEAR] + a + [CLEAR, CLEAR] + b)


def _no_eoi():
    return _one_strip(96, 40, lzw_greedy(_px(40, 96, 913).tobytes())[:-1])


def _ends_inside_a_string():
    """The strip is full 5 bytes into a 9-byte string."""
    raw = (b"abcdefghi" * 500)[:96 * 40 + 4]
    codes = lzw_greedy(raw)
    f = _one_strip(96, 40, codes)
    assert lzw_model(f.streams[0], 96 * 40 + 4)[1] == "ok" and lzw_model(lzw_pack(codes[:-2]), 96 * 40)[1] == "short"
    return f


def _tiny_last_strip():
    """w = 3: the last strip is one row, its stream Clear, v, 258 (v v v) in
    27 bits: 4 bytes, no EOI."""
    w, h, rps = 3, 41, 8
    px = _px(h, w, 914)
    streams = [lzw_pack(lzw_greedy(px[y:y + rps].tobytes())) for y in range(0, 40, rps)] + [lzw_pack([CLEAR, 77, 258])]
    assert len(streams[-1]) == 4
    return StripFile(w, h, rps, tuple(streams))


def _three_byte_strips():
    """w = 1, a strip per row: Clear and a literal, 18 bits in 3 bytes; every
    other one goes on with EOI, 27 bits in 4.  41 strips 3 or 4 bytes apart."""
    rng = _rng(915)
    streams = tuple(lzw_pack([CLEAR, int(rng.integers(0, 256))] + ([EOI] if y & 1 else [])) for y in range(41))
    assert {len(s) for s in streams} == {3, 4}
    return StripFile(1, 41, 1, streams)


def _no_initial_clear():
    return _one_strip(96, 40, lzw_greedy(_px(40, 96, 916).tobytes())[1:])


def _never_clears(n_codes):
    """One segment of n_codes literals."""
    w = 100
    raw = _px(n_codes // w, w, 917).tobytes()
    return _one_strip(w, n_codes // w, [CLEAR] + list(raw) + [EOI])


def _seg_exact(n, seed):
    """A first segment of exactly n codes (4096: the longest the parallel
    route holds; 4097: serial), then ordinary ones."""
    w, h = 100, 90
    codes = lzw_random_codes(_rng(seed), w * h, p_lit=0.93, p_cur=0.02, p_clear=0.002, clear_at=(n,))
    f = _one_strip(w, h, codes)
    assert lzw_segments(f.streams[0])[0] == n
    return f


def _clear_at(n, seed):
    """A Clear exactly where the code width would change (after n codes),
    twice over, the Clear itself already at the new width."""
    w, h = 100, 90
    codes = lzw_random_codes(_rng(seed), w * h, p_lit=0.93, p_cur=0.02, p_clear=0.003, clear_at=(n, n))
    f = _one_strip(w, h, codes)
    assert lzw_segments(f.streams[0])[:2] == [n, n] and lzw_route(f.streams[0]) == "parallel"
    return f


def _periodic(pattern: bytes):
    raw = (pattern * 4000)[:96 * 40]
    return _one_strip(96, 40, lzw_greedy(raw))


LZW_FILES = {
    "clear_at_254": lambda: _clear_at(254, 921),
    "clear_at_766": lambda: _clear_at(766, 922),
    "clear_at_1790": lambda: _clear_at(1790, 923),
    "segment_4096": lambda: _seg_exact(4096, 924),
    "segment_4097": lambda: _seg_exact(4097, 925),
    "flat_full_dictionary": lambda: _flat(3838, 2714, 2714),  # 7 367 041 bytes from 5 409
    "flat_past_9_bits": lambda: _flat(258, 182, 183),
    "flat_past_10_bits": lambda: _flat(770, 544, 545),     # 0.3 MB
    "flat_past_11_bits": lambda: _flat(1795, 1269, 1270),  # 1.6 MB
    "period_2": lambda: _periodic(b"\x10\xef"),
    "period_3": lambda: _periodic(b"\x01\x80\xfe"),
    "three_ways_parallel": lambda: three_ways_file(("parallel",)),
    "three_ways_long": lambda: three_ways_file(("long",)),
    "three_ways_clear3": lambda: three_ways_file(("clear3",)),
    "three_ways_mixed": lambda: three_ways_file(("long", "parallel", "clear3", "parallel", "long", "clear3")),
    "consecutive_clears": _consecutive_clears,
    "no_eoi": _no_eoi,
    "garbage_after_full": _garbage_after_full,
    "ends_inside_a_string": _ends_inside_a_string,
    "tiny_last_strip": _tiny_last_strip,
    "three_byte_strips": _three_byte_strips,
    "no_initial_clear": _no_initial_clear,
    "never_clears_6000": lambda: _never_clears(6000),
}
# valid for the model and the product, refused by libtiff 4.7.1 (module docstring)
LIBTIFF_REFUSES = ("no_initial_clear", "never_clears_6000")
# the one image above 0.1 MP by design, and the two flat strips that must
# reach the 11- and 12-bit codes (string i is i + 1 bytes long)
LARGE = ("flat_full_dictionary", "flat_past_10_bits", "flat_past_11_bits")


@functools.lru_cache(maxsize=None)
def lzw_file(name: str) -> StripFile:
    return LZW_FILES[name]()


# ---- error streams: (bad file, good file, what the message says) ----
LZW_ERROR_KINDS = ("invalid_at_k0", "invalid_mid_segment", "invalid_after_width_change", "eoi_early", "truncated")
ROUTES = ("parallel", "serial")


@functools.lru_cache(maxsize=None)
def lzw_error_pair(kind: str, route: str):
    """Two strips of 20 rows x 80; the second one is at fault.  Its first
    1000 bytes are coded greedily (route "parallel") or with a Clear every 3
    codes (so the strip has more segments than its slice holds: "serial"),
    the last 600 as literals after a Clear: the k-th code of that segment is
    byte 1000 + k, and the fault sits at a chosen k."""
    w, rps, h, a = 80, 20, 40, 1000
    px = _px(h, w, 931 + LZW_ERROR_KINDS.index(kind))
    s0 = lzw_pack(lzw_greedy(px[:rps].tobytes()))
    raw = px[rps:].tobytes()
    prefix = lzw_greedy(raw[:a], clear_every=3 if route == "serial" else None)[:-1]
    tail = list(raw[a:])
    good = lzw_pack(prefix + [CLEAR] + tail + [EOI])

    def swapped(k, code):
        assert code > 257 + k and code < (1 << lzw_width(k))
        return lzw_pack(prefix + [CLEAR] + tail[:k] + [code] + tail[k + 1:] + [EOI])

    if kind == "invalid_at_k0":
        bad, status = swapped(0, 300), "bad"
    elif kind == "invalid_mid_segment":
        bad, status = swapped(100, 500), "bad"
    elif kind == "invalid_after_width_change":
        bad, status = swapped(254, 1000), "bad"  # the first 10-bit code
    elif kind == "eoi_early":
        bad, status = lzw_pack(prefix + [CLEAR] + tail[:300] + [EOI]), "short"
    else:
        bad, status = good[:len(good) * 3 // 4], "short"
    bad_f, good_f = StripFile(w, h, rps, (s0, bad)), StripFile(w, h, rps, (s0, good))
    assert lzw_route(bad) == lzw_route(good) == route and lzw_route(s0) == "parallel"
    assert bad_f.model()[1][1] == status and len(bad_f.model()[1][0]) < rps * w
    return bad_f, good_f, "corrupt"


@functools.lru_cache(maxsize=None)
def lzw_old_style_pair(neighbour: str):
    """The LSB-first flavour (byte 0, then an odd byte), next to a strip of
    either route.  The flavour is told from the first two bytes before any
    route is chosen, so it has no serial form of its own."""
    w, rps, h = 80, 20, 40
    px = _px(h, w, 941)
    s0 = three_ways(px[:rps].tobytes(), "clear3" if neighbour == "serial" else "parallel")
    good = lzw_pack(lzw_greedy(px[rps:].tobytes()))
    old = b"\x00\x01" + bytes(_rng(942).integers(0, 256, 700, dtype=np.uint8))
    bad_f = StripFile(w, h, rps, (s0, old))
    assert bad_f.model()[1][1] == "old" and lzw_route(s0) == neighbour
    return bad_f, StripFile(w, h, rps, (s0, good)), "old-style"


# ----------------------------------------------------------------------------
# PackBits
# ----------------------------------------------------------------------------
def packbits_runs(raw: bytes, row_bytes: int, rng) -> bytes:
    """PackBits as encoders write it: each row of `row_bytes` packed on its
    own (no run crosses a row), equal bytes as replicate runs of 2..128,
    the rest as literal runs of 1..128 (the maxima whenever the data allow,
    shorter pieces now and then), a repeat of 2 sometimes left in a literal
    run, and 0x80 no-ops scattered between the runs."""
    out = bytearray()

    def noop():
        if rng.random() < 0.1:
            out.append(0x80)

    def flush(lit):
        while lit:
            n = min(len(lit), 128)
            if n > 1 and rng.random() < 0.25:
                n = int(rng.integers(1, n + 1))
            out.append(n - 1)
            out.extend(lit[:n])
            del lit[:n]
            noop()

    for r0 in range(0, len(raw), row_bytes):
        row = raw[r0:r0 + row_bytes]
        i, lit = 0, bytearray()
        while i < len(row):
            j = i
            while j < len(row) and row[j] == row[i]:
                j += 1
            r = j - i
            if r == 1 or (r == 2 and rng.random() < 0.5):
                lit += row[i:j]
                i = j
                continue
            flush(lit)
            while r >= 2:
                n = min(r, 128)
                if n > 2 and rng.random() < 0.2:
                    n = int(rng.integers(2, n + 1))
                out.append((1 - n) & 0xFF)
                out.append(row[i])
                noop()
                r -= n
                i += n
            if r:
                lit.append(row[i])
                i += 1
        flush(lit)
    return bytes(out)


def packbits_model(stream: bytes, cap: int) -> tuple[bytes, str]:
    """The `cap` bytes of a strip from `stream` (TIFF 6.0 section 9; libtiff
    cuts a run that crosses cap and stops there): header c in 0..127 copies
    c + 1 bytes, 129..255 repeats the next byte 257 - c = 1 - (c - 256)
    times, 128 does nothing.  "bad": a run whose bytes the stream does not
    hold; "short": the stream ends before cap."""
    out, i, n = bytearray(), 0, len(stream)
    while i < n and len(out) < cap:
        c = stream[i]
        i += 1
        if c < 128:
            if i + c + 1 > n:
                return bytes(out), "bad"
            out += stream[i:i + c + 1]
            i += c + 1
        elif c != 128:
            if i >= n:
                return bytes(out), "bad"
            out += bytes([stream[i]]) * (257 - c)
            i += 1
    return bytes(out[:cap]), "ok" if len(out) >= cap else "short"


def packbits_headers(stream: bytes) -> list:
    """The run headers of a well-formed stream."""
    hs, i = [], 0
    while i < len(stream):
        c = stream[i]
        hs.append(c)
        i += 1 + (c + 1 if c < 128 else 1 if c != 128 else 0)
    return hs


def line_art(h: int, w: int, bits: int, seed: int) -> np.ndarray:
    """Indices with what scans have: a blank margin (the left 60 % of every
    row, its value changing every few rows), blocky content, and a stretch
    in which no two neighbours are equal."""
    rng = np.random.default_rng([20261019, 9, seed])
    a = pf.indices(h, w, bits, seed)
    m = w * 6 // 10
    a[:, :m] = (np.arange(h)[:, None] // 3 * 5 + 1) % (1 << bits)
    lo = m + (w - m) // 2
    if bits == 8:
        step = rng.integers(1, 255, size=(h, w - lo), dtype=np.int64)
        a[:, lo:] = (np.cumsum(step, axis=1) % 256).astype(np.uint8)
    return np.ascontiguousarray(a)


def _pb_runs_file():
    """Gray8, 300 wide: every row has 135 equal bytes, and every other row
    140 in a row of which no two neighbours are equal (the maxima of both
    run kinds); the rows between have them rotated by 70."""
    w, h, rps = 300, 21, 8
    px = line_art(h, w, 8, 951)
    px[:, :135] = px[:, :1]
    px[:, 135:275] = np.cumsum(_rng(952).integers(1, 255, size=(h, 140)), axis=1).astype(np.uint8)
    px[::2, :] = np.roll(px[::2, :], 70, axis=1)
    rng = _rng(953)
    f = StripFile(w, h, rps, tuple(packbits_runs(px[y:y + rps].tobytes(), w, rng) for y in range(0, h, rps)), PACKBITS)
    assert np.array_equal(f.pixels(), px)
    return f


def _pb_cut_at_cap():
    """Strip 0: a replicate run of 128 with 5 bytes of room.  Strip 1: a
    literal run of 20 with 10 bytes of room, then rubbish."""
    w, rps = 50, 4
    d = bytes(_rng(954).integers(0, 256, 400, dtype=np.uint8))
    s0 = bytes([127]) + d[:128] + bytes([66]) + d[128:195] + bytes([0x81, 0xC3])
    s1 = bytes([127]) + d[200:328] + bytes([61]) + d[328:390] + bytes([19]) + d[:20] + bytes([5, 1])
    return StripFile(w, 8, rps, (s0, s1), PACKBITS)


def _pb_noops():
    """No-ops before, between and after the runs; 2-byte repeats both ways."""
    w, rps = 64, 8
    d = bytes(_rng(955).integers(0, 256, 64, dtype=np.uint8))
    rows = []
    for y in range(8):
        rows.append(b"\x80\x80" + bytes([31]) + d[y:y + 32] + b"\x80" + bytes([0xFF, y, 0x80, 1, 9, 9]) +
                    bytes([0x80, 0xE5, 200 + y]) + b"\x80")  # 32 + 2 + 2 + 28
    return StripFile(w, 8, rps, (b"".join(rows),), PACKBITS)


PB_FILES = {"runs": _pb_runs_file, "cut_at_cap": _pb_cut_at_cap, "noops": _pb_noops}


@functools.lru_cache(maxsize=None)
def pb_file(name: str) -> StripFile:
    return PB_FILES[name]()


PB_ERROR_KINDS = ("literal_past_the_end", "replicate_header_last")


@functools.lru_cache(maxsize=None)
def pb_error_pair(kind: str):
    w, rps, h = 80, 20, 40
    px = line_art(h, w, 8, 961)
    rng = _rng(962)
    s0, good = (packbits_runs(px[y:y + rps].tobytes(), w, rng) for y in (0, rps))
    part = packbits_runs(px[rps:rps + 7].tobytes(), w, rng)
    bad = part + (bytes([10, 1, 2, 3]) if kind == "literal_past_the_end" else bytes([0xFE]))
    bad_f = StripFile(w, h, rps, (s0, bad), PACKBITS)
    assert bad_f.model()[1][1] == "bad"
    return bad_f, StripFile(w, h, rps, (s0, good), PACKBITS), "corrupt"


# ----------------------------------------------------------------------------
# Predictor 2 layout matrix
# ----------------------------------------------------------------------------
AXES = {
    "codec": ("lzw", "deflate", "packbits"),
    "layout": ("strips_chunky", "strips_planar", "tiles_chunky", "tiles_planar"),
    "sample": ("u8", "u16le", "u16be"),
    "components": (1, 2, 3, 4),
}
_WIDTHS = (17, 45, 32, 2, 1)  # ragged against a tile width of 16, a tile multiple, and the degenerate ones
_HEIGHTS = (37, 21, 43)       # neither 8 (RowsPerStrip) nor 16 (TileLength) divides them
TILE, RPS = (16, 16), 8


def _pairs(combo):
    names = list(AXES)
    return {(names[i], combo[i], names[j], combo[j]) for i in range(4) for j in range(i + 1, 4)}


def _layout_matrix():
    """A pairwise cover, greedily (the combination that covers most uncovered
    pairs next; ties go to the first), then the representatives the route
    tests need, then more until there are 24."""
    combos = list(itertools.product(*AXES.values()))
    todo = set().union(*(_pairs(c) for c in combos))
    chosen = []
    while todo:
        best = max(combos, key=lambda c: len(_pairs(c) & todo))
        chosen.append(best)
        todo -= _pairs(best)
    for c in (("lzw", "tiles_chunky", "u8", 3), ("deflate", "tiles_planar", "u16be", 3),
              ("lzw", "tiles_planar", "u16be", 4), ("packbits", "strips_planar", "u16le", 2),
              ("lzw", "strips_planar", "u16be", 3), ("packbits", "tiles_chunky", "u16be", 4),
              ("deflate", "strips_chunky", "u16be", 2), ("lzw", "tiles_chunky", "u16le", 1)):
        if c not in chosen and len(chosen) < 24:
            chosen.append(c)
    out = []
    for i, (codec, layout, sample, nc) in enumerate(chosen):
        w, h = _WIDTHS[i % len(_WIDTHS)], _HEIGHTS[i % len(_HEIGHTS)]
        out.append(dict(id=f"{codec}_{layout}_{sample}_c{nc}_{w}x{h}", codec=codec, layout=layout, sample=sample,
                        components=nc, w=w, h=h, seed=1000 + i))
    return out


LAYOUT_CASES = _layout_matrix()
# every pair of values of two axes occurs, and every width: keeps later edits from thinning the matrix out
assert set().union(*(_pairs((c["codec"], c["layout"], c["sample"], c["components"])) for c in LAYOUT_CASES)) == \
    set().union(*(_pairs(c) for c in itertools.product(*AXES.values())))
assert {c["w"] for c in LAYOUT_CASES} == set(_WIDTHS) and 20 <= len(LAYOUT_CASES) <= 28


def noise(h, w, nc, dtype, seed) -> np.ndarray:
    """Uniform noise whose second pixel of every row is smaller than the
    first in every component, so every row has a difference that wraps."""
    rng = np.random.default_rng([20261019, 11, seed])
    bits = np.dtype(dtype).itemsize * 8
    a = rng.integers(0, 1 << bits, size=(h, w, nc)).astype(dtype)
    if w >= 2:
        top = 1 << (bits - 1)
        a[:, 0] |= top
        a[:, 1] &= top - 1
    return a


def every_row_wraps(px: np.ndarray) -> bool:
    """Some sample of each row (each component) is smaller than its left neighbour."""
    p = px.reshape(px.shape[0], px.shape[1], -1).astype(np.int64)
    return p.shape[1] < 2 or bool(((p[:, 1:] - p[:, :-1]) < 0).any(axis=1).all())


def layout_codec(name, row_bytes, seed):
    """(bytes -> bytes, Compression value): LZW alternates libtiff's shape with
    a Clear every 300 codes; PackBits packs rows of `row_bytes`."""
    if name == "lzw":
        return (lambda raw: im.lzw_encode(raw, clear_every=300 if seed & 1 else None)), LZW
    if name == "deflate":
        return zlib.compress, DEFLATE
    rng = np.random.default_rng([20261019, 13, seed])
    return (lambda raw: packbits_runs(raw, row_bytes, rng)), PACKBITS


def layout_write(case, px: np.ndarray) -> bytes:
    """`px` (h, w, components) as the Predictor 2 file the case describes
    (its codec, layout and byte order; the component count is px's own)."""
    h, w, nc = px.shape
    be = case["sample"] == "u16be" or (case["sample"] == "u8" and case["seed"] % 2 == 1)
    tiled, planar = case["layout"].startswith("tiles"), case["layout"].endswith("planar")
    row_bytes = (TILE[0] if tiled else w) * (1 if planar else nc) * px.dtype.itemsize
    fn, tag = layout_codec(case["codec"], row_bytes, case["seed"])
    if tiled:
        return im.tiled_tiff_bytes(px, tile=TILE, planar=planar, big_endian=be, codec=fn, compression=tag, predictor=2)
    return im.tiff_bytes(px, rows_per_strip=RPS, planar=planar, big_endian=be, strip_codec=fn, compression=tag,
                         predictor=2)


def layout_build(case, h=None):
    """(tiff bytes, source pixels) of a LAYOUT_CASES entry (h: another height)."""
    nc = case["components"]
    px = noise(h or case["h"], case["w"], nc, np.uint8 if case["sample"] == "u8" else np.uint16, case["seed"])
    assert every_row_wraps(px)
    return layout_write(case, px), (px if nc > 1 else px[..., 0])


def layout_expect(case, h=None):
    """What jp2hip.tiff_layout must say: compression, predictor, tile size, units."""
    h = h or case["h"]
    tiled, planar = case["layout"].startswith("tiles"), case["layout"].endswith("planar")
    per_plane = -(-case["w"] // TILE[0]) * -(-h // TILE[1]) if tiled else -(-h // RPS)
    return dict(compression={"lzw": LZW, "deflate": DEFLATE, "packbits": PACKBITS}[case["codec"]], predictor=2,
                tile=TILE if tiled else (0, 0), units=per_plane * (case["components"] if planar else 1))


# ----------------------------------------------------------------------------
# 1-bit, 4-bit and palette files through packbits_runs
# ----------------------------------------------------------------------------
PACKED_CASES = [
    dict(id="g1_runs_strips", bits=1, photometric=pf.WHITE_IS_ZERO, h=37, w=1100, seed=971, rps=16, tile=None),
    dict(id="g4_runs_strips_be", bits=4, photometric=pf.BLACK_IS_ZERO, h=37, w=300, seed=972, rps=16, tile=None,
         big_endian=True),
    dict(id="p8_runs_strips", bits=8, photometric=pf.PALETTE, h=41, w=261, seed=973, cmap_seed=983, rps=16, tile=None),
    dict(id="g1_runs_tiles", bits=1, photometric=pf.BLACK_IS_ZERO, h=70, w=300, seed=974, tile=(128, 16)),
    dict(id="p4_runs_tiles_be", bits=4, photometric=pf.PALETTE, h=70, w=90, seed=975, cmap_seed=985, tile=(64, 16),
         big_endian=True),
    dict(id="p8_runs_tiles", bits=8, photometric=pf.PALETTE, h=70, w=90, seed=976, cmap_seed=986, tile=(32, 48)),
    # LZW tiles of packed samples (decoded to the tile's own size, never untiled before the expansion)
    dict(id="g1_lzw_tiles", bits=1, photometric=pf.WHITE_IS_ZERO, h=70, w=300, seed=977, tile=(128, 16), codec="lzw"),
    dict(id="p4_lzw_tiles", bits=4, photometric=pf.PALETTE, h=70, w=90, seed=978, cmap_seed=988, tile=(64, 16),
         codec="lzw"),
]


def packed_build(case, h=None):
    """(tiff bytes, expected 8-bit pixels, the run headers of its PackBits streams)."""
    bits, h = case["bits"], h or case["h"]
    idx = line_art(h, case["w"], bits, case["seed"])
    cm = pf.random_colormap(bits, case["cmap_seed"]) if case["photometric"] == pf.PALETTE else None
    row_bytes = (case["tile"][0] if case["tile"] else case["w"]) * bits
    row_bytes = (row_bytes + 7) // 8
    rng = np.random.default_rng([20261019, 15, case["seed"]])
    seen = []

    def codec(raw):
        s = packbits_runs(raw, row_bytes, rng)
        assert packbits_model(s, len(raw)) == (raw, "ok")
        seen.extend(packbits_headers(s))
        return s

    kw = dict(tile=case["tile"]) if case["tile"] else dict(rows_per_strip=case["rps"])
    tif = pf.make_tiff(idx, bits, case["photometric"], colormap=cm, big_endian=bool(case.get("big_endian")),
                       codec=(im.lzw_encode, LZW) if case.get("codec") == "lzw" else (codec, PACKBITS), **kw)
    return tif, pf.expand(idx, bits, case["photometric"], cm), seen
