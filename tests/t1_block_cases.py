"""Crafted code-block corpus for tier-1, shared by the oracle's own checks
(tests/test_t1_blocks.py, CPU) and the GPU parity test
(tests/test_gpu_t1_blocks.py).

With levels=0, one component, mct=0 and tiles no larger than the 64x64
code-block, every tile is one LL code-block whose coefficients are the
level-shifted samples: reversible, coefficient = sample - 2^(B-1);
irreversible with qstep = 2^-B the step is 1 and the index is the same
magnitude.  So a block of chosen signed coefficients is a tile of the image,
and the tile index names the pattern.  With levels=1 and 128x128 tiles each of
LL/HL/LH/HH is one 64x64 block; the integer 5/3 transform is exactly
invertible (inverse_53 below), so chosen sub-bands map back to an image.

Families (blocks16() / blocks8() / band_tiles() / geometry_cases()):
  full       every magnitude the largest: each plane's cleanup or refinement
             pass carries the most decisions a block can have
  chain      one seed with bit p+1 and samples with bit p only, laid so that
             significance propagation runs with, against and across the scan
  bernoulli  independent bit-planes of a given density, signs independent or
             correlated with the neighbours
  mps_run    (almost) empty and constant blocks: thousands of MPS in a row
  byteout    seeds found by search_byteout_seeds() whose streams take the rare
             mq_byteout / mq_flush branches
  hvd        seeds found by search_hvd_seeds(): between them every
             zero-coding neighbourhood in both passes with both decisions
  geometry   noise blocks of every small w x h (tile_w = w, tile_h = h)
  straddle   tiles that cross the 64-sample code-block grid: several blocks
             a tile, cut where no other case cuts
  bands      levels=1: the families above as LL/HL/LH/HH contents

Everything is deterministic; nothing here needs a GPU.
"""
from __future__ import annotations

import struct

import numpy as np

import imaging as im

SEED = 20261020
N = 64

# recipe kinds: (a) lossless 1 layer, (b) lossless 32 layers, (c) irreversible
# step 1, rate-driven, 12 layers, (d) as (c) with slope prediction
KINDS = ("a", "b", "c", "d")
BASE = dict(levels=0, mct=0, tile_w=N, tile_h=N, cblk_w_log2=6, cblk_h_log2=6, flush_period=0, format=0,
            nprecincts=0, comment=0)


def recipe_for(kind: str, bits: int, rate: float, **geometry) -> tuple:
    """(lossless, overrides) of recipe `kind` for `bits`-bit samples; `rate`
    is the budget of the rate-driven kinds (about half the lossless size)."""
    r = dict(BASE, **geometry)
    if kind == "a":
        return True, dict(r, layers=1, rate_bpp=0.0)
    if kind == "b":
        return True, dict(r, layers=32, rate_bpp=0.0)
    return False, dict(r, layers=12, rate_bpp=rate, qstep=2.0 ** -bits, slope_skip=int(kind == "d"))


# --------------------------------------------------------------------------
# scan order and the significance-propagation model the tests compare with
# --------------------------------------------------------------------------
def scan_order(w: int, h: int):
    """(x, y) in tier-1 scan order: stripes of 4 rows, columns left to right,
    rows top to bottom within a column (D.1)."""
    return [(x, y) for y0 in range(0, h, 4) for x in range(w) for y in range(y0, min(y0 + 4, h))]


def spp_depth_model(block: np.ndarray, p: int) -> int:
    """Longest propagation chain of the significance pass of plane p, by the
    definition alone: samples with a bit above p are significant already; in
    scan order, a sample with bit p and a significant neighbour becomes
    significant with depth 1 + the deepest neighbour that became significant
    in this pass."""
    h, w = block.shape
    mag = np.abs(block.astype(np.int64))
    sig = np.zeros((h + 2, w + 2), bool)
    sig[1:-1, 1:-1] = (mag >> (p + 1)) != 0
    depth = np.zeros((h + 2, w + 2), np.int64)
    best = 0
    for x, y in scan_order(w, h):
        if sig[y + 1, x + 1] or not (mag[y, x] >> p) & 1:
            continue
        if sig[y:y + 3, x:x + 3].any():
            d = 1 + int(depth[y:y + 3, x:x + 3].max())
            depth[y + 1, x + 1] = d
            sig[y + 1, x + 1] = True
            best = max(best, d)
    return best


def longest_forward_chain(w: int, h: int) -> int:
    """The longest chain any block of this size can hold: 8-connected samples
    in strictly increasing scan order (each link needs the earlier sample
    coded before the later one is visited)."""
    rank = {xy: i for i, xy in enumerate(scan_order(w, h))}
    best = {}
    for x, y in scan_order(w, h):
        m = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                q = (x + dx, y + dy)
                if q in rank and rank[q] < rank[(x, y)]:
                    m = max(m, best[q])
        best[(x, y)] = m + 1
    return max(best.values())


# --------------------------------------------------------------------------
# block families: each returns [(name, int32 array of signed coefficients)]
# --------------------------------------------------------------------------
def _rng(tag: str):
    return np.random.default_rng([SEED] + [ord(c) for c in tag])


def full_blocks(top: int = 32767):
    yy, xx = np.mgrid[0:N, 0:N]
    r = _rng("full")
    out = [("full_pos", np.full((N, N), top)),
           ("full_neg", np.full((N, N), -top)),
           ("full_checker", np.where((xx + yy) & 1, -top, top)),
           ("full_random", np.where(r.random((N, N)) < 0.5, -top, top)),
           ("full_min", np.full((N, N), -top - 1))]  # sample 0: magnitude 2^(B-1)
    return [(n, a.astype(np.int32)) for n, a in out]


def serpentine():
    """Boustrophedon path over the even rows: 2079 samples, each touching only
    its predecessor and successor.  Whichever end is seeded, propagation runs
    along one row and stops where the path turns against the scan; every
    other sample waits for the cleanup pass."""
    path = []
    for j, y in enumerate(range(0, N, 2)):
        xs = range(N) if j % 2 == 0 else range(N - 1, -1, -1)
        path += [(x, y) for x in xs]
        if y + 2 < N:
            path.append((path[-1][0], y + 1))
    return path


def staircase():
    """A longest forward chain (220 samples): from the first sample, zigzag
    over rows 1 and 2 of the first stripe, then down the last two columns, six
    samples a stripe.  (1, 0) is left free for the seed."""
    path = [(0, 0)] + [(x, y) for x in range(N) for y in (1, 2)] + [(N - 1, 3)]
    for y0 in range(4, N, 4):
        path += [(N - 2, y0), (N - 2, y0 + 1), (N - 1, y0), (N - 1, y0 + 1), (N - 1, y0 + 2), (N - 1, y0 + 3)]
    return path


def _path_block(path, p, seed_at_start=True, seed=None):
    a = np.zeros((N, N), np.int32)
    for x, y in path:
        a[y, x] = 1 << p
    x, y = seed or (path[0] if seed_at_start else path[-1])
    a[y, x] = 1 << (p + 1)
    return a


def chain_blocks():
    """[(name, block, p)]: p is the plane whose significance pass the block is
    about (the seeds' bit is p + 1)."""
    out = []
    s, st = serpentine(), staircase()
    assert len(s) >= 1000
    out.append(("chain_serp_fwd", _path_block(s, 3), 3))
    out.append(("chain_serp_rev", _path_block(s, 5, False), 5))
    out.append(("chain_stair_fwd", _path_block(st, 2, seed=(1, 0)), 2))
    out.append(("chain_stair_rev", _path_block(st, 7, False), 7))
    # vertical runs down every fourth column (through every stripe boundary
    # and rows 31/32), seeded at the top and at the bottom
    for name, top in (("chain_down", True), ("chain_up", False)):
        a = np.zeros((N, N), np.int32)
        a[:, ::4] = 1 << 4
        a[0 if top else N - 1, ::4] = 1 << 5
        out.append((name, a, 4))
    # steps by the upper-right neighbour: A (seed) <- B <- C <- D down an
    # anti-diagonal, C at a stripe top (B is in the stripe above: coded
    # already, C joins) and D below it (C's column comes later: D waits for
    # cleanup).  Groups at every other stripe boundary, row 31/32 included.
    a = np.zeros((N, N), np.int32)
    for k in range(1, 15, 2):
        for x in range(4 + (k % 4) // 2 * 3, N, 6):
            y = 4 * k + 2
            a[y, x], a[y + 1, x - 1], a[y + 2, x - 2], a[y + 3, x - 3] = 1 << 7, 1 << 6, 1 << 6, 1 << 6
    out.append(("chain_ur_steps", a, 6))
    # steps by the lower-left neighbour, up an anti-diagonal: inside a stripe
    # the lower-left sample is in the column before (coded: the chain runs to
    # the stripe top); at a stripe bottom it is in the stripe below (not yet).
    a = np.zeros((N, N), np.int32)
    for k in range(0, 16, 2):
        for x in range((k % 4) // 2 * 3, N - 3, 6):  # inside stripe k
            y = 4 * k + 3
            a[y, x], a[y - 1, x + 1], a[y - 2, x + 2], a[y - 3, x + 3] = 1 << 9, 1 << 8, 1 << 8, 1 << 8
    out.append(("chain_dl_inside", a, 8))
    a = np.zeros((N, N), np.int32)
    for k in range(0, 15):
        for x in range((k % 2) * 2, N - 2, 5):      # across the bottom of stripe k
            y = 4 * k + 5
            a[y, x], a[y - 1, x + 1], a[y - 2, x + 2] = 1 << 9, 1 << 8, 1 << 8
    out.append(("chain_dl_bottom", a, 8))
    # lanes 0 and 63: rows that run the whole width from either end, and
    # samples that would join only if column 63 and column 0 were neighbours
    a = np.zeros((N, N), np.int32)
    a[1, :] = 1 << 3
    a[1, 0] = 1 << 4
    a[9, :] = 1 << 3
    a[9, N - 1] = 1 << 4
    a[20, N - 1] = 1 << 4
    a[19:22, 0] = 1 << 3
    a[40, 0] = 1 << 4
    a[39:42, N - 1] = 1 << 3
    out.append(("chain_lanes", a, 3))
    # rows 31/32: diagonals through the boundary of the two halves, down-right
    # from a seed above it (every step sees a coded sample) and up-right from
    # a seed below it (the step from row 32 to row 31 leaves its stripe)
    a = np.zeros((N, N), np.int32)
    for x in range(0, 24, 9):
        for i in range(8):
            a[28 + i, x + i] = 1 << 5
            a[35 - i, 32 + x + i] = 1 << 5
        a[28, x] = a[35, 32 + x] = 1 << 6
    out.append(("chain_halves", a, 5))
    return out


CHAIN_PLANE = {n: p for n, _, p in chain_blocks()}
DENSITIES = ((1, 64), (1, 8), (1, 2), (7, 8), (63, 64))


def _signs_correlated(r, mode):
    """Sign field that follows the left neighbour (mode "left"), the upper one
    ("up") or opposes both ("anti"), nine times out of ten."""
    s = np.zeros((N, N), bool)
    flip = r.random((N, N)) < 0.1
    first = r.random((N, N)) < 0.5
    for y in range(N):
        for x in range(N):
            if mode == "left" and x:
                s[y, x] = s[y, x - 1] ^ flip[y, x]
            elif mode == "up" and y:
                s[y, x] = s[y - 1, x] ^ flip[y, x]
            elif mode == "anti" and (x or y):
                s[y, x] = (not s[y, x - 1] if x else not s[y - 1, x]) ^ flip[y, x]
            else:
                s[y, x] = first[y, x]
    return s


def bernoulli_blocks(planes: int = 15):
    out = []
    for i, (a, b) in enumerate(DENSITIES):
        for mode in ("indep", ("left", "up", "anti", "left", "up")[i]):
            r = _rng(f"bern{a}/{b}{mode}")
            mag = np.zeros((N, N), np.int64)
            for p in range(planes):
                mag |= (r.random((N, N)) < a / b).astype(np.int64) << p
            neg = r.random((N, N)) < 0.5 if mode == "indep" else _signs_correlated(r, mode)
            out.append((f"bern_{a}of{b}_{mode}", np.where(neg, -mag, mag).astype(np.int32)))
    return out


def mps_run_blocks(top: int = 32767):
    out = []
    z = np.zeros((N, N), np.int32)
    out.append(("mps_zero", z.copy()))
    for name, (x, y) in (("mps_last", (N - 1, N - 1)), ("mps_first", (0, 0)), ("mps_middle", (31, 33))):
        a = z.copy()
        a[y, x] = -top if name == "mps_middle" else top
        out.append((name, a))
    for name, y0 in (("mps_stripe0", 0), ("mps_stripe9", 36)):
        a = z.copy()
        a[y0:y0 + 4, :] = top
        out.append((name, a))
    r = _rng("mps")
    out.append(("mps_const_top", np.full((N, N), (top + 1) >> 1, np.int32)))           # one bit, then zeros
    out.append(("mps_const_alt", np.where(r.random((N, N)) < 0.5, -1, 1).astype(np.int32) * (0x5555 & top)))
    out.append(("mps_const_one", np.full((N, N), -1, np.int32)))
    return out


def byteout_block(seed: int, top: int = 32767) -> np.ndarray:
    """The search space of the byteout family: a few dozen random samples in
    an empty block (short streams: one flush per few hundred bytes)."""
    r = np.random.default_rng([SEED, 7, seed])
    a = np.zeros((N, N), np.int32)
    n = int(r.integers(8, 96))
    ys, xs = r.integers(0, N, n), r.integers(0, N, n)
    a[ys, xs] = r.integers(-top, top + 1, n)
    return a


def search_byteout_seeds(hi: int = 6000, want: int = 8):
    """How BYTEOUT_SEEDS was found (CPU, seconds): first the seeds whose
    stream carries into a byte that becomes 0xFF (one block in forty), then
    more until every mq_byteout and mq_flush branch is taken `want` times."""
    import oracle_lib as ol
    seeds, by, fl = [], np.zeros(4, np.int64), np.zeros(4, np.int64)
    for rare_only in (True, False):
        for s in range(hi):
            if s in seeds or (by.min() >= want and fl.min() >= want):
                continue
            ol.census_reset()
            ol.t1_encode(to_sm(byteout_block(s)), 0, True)
            c = ol.census_read()
            if rare_only:
                take = c["byteout"][ol.BO_CARRY_TO_FF] > 0 and by[ol.BO_CARRY_TO_FF] < want
            else:
                take = bool(((c["flush"] > 0) & (fl < want)).any())
            if take:
                seeds.append(s)
                by += c["byteout"]
                fl += c["flush"]
    return tuple(seeds)


BYTEOUT_SEEDS = (7, 84, 88, 102, 122, 171, 260, 312, 0, 1, 2, 3, 4, 5, 6, 9, 19, 20, 21, 23, 24)


def byteout_blocks(top: int = 32767):
    return [(f"byteout_{s}", byteout_block(s, top)) for s in BYTEOUT_SEEDS]


def hvd_block(seed: int) -> np.ndarray:
    """The search space of the hvd family: a sparse top plane under a dense
    second one.  The samples the top plane leaves without a significant
    neighbour wait for the second plane's cleanup pass, by which time their
    neighbours have become significant around them."""
    r = np.random.default_rng([SEED, 11, seed])
    d1 = (1 / 32, 1 / 16, 1 / 8, 1 / 5)[seed % 4]
    d2 = (0.6, 0.8, 0.9, 0.97)[(seed // 4) % 4]
    top = r.random((N, N)) < d1
    low = r.random((N, N)) < d2
    mag = (top.astype(np.int64) << 1) | low
    neg = r.random((N, N)) < 0.5
    return np.where(neg, -mag, mag).astype(np.int32)


def search_hvd_seeds(hi: int = 3000):
    """How HVD_SEEDS was found (CPU, seconds): a greedy cover of every
    zero-coding neighbourhood (h, v, d) x pass x decision."""
    import oracle_lib as ol
    rows = []
    for s in range(hi):
        ol.census_reset()
        ol.t1_encode(to_sm(hvd_block(s)), 0, True)
        rows.append(ol.census_read()["zc"][0] > 0)
    need = np.ones(rows[0].shape, bool)
    need[0, 0, 0, 0, :] = False  # no significance pass without a significant neighbour
    seeds = []
    while need.any():
        gains = [int((r & need).sum()) for r in rows]
        b = int(np.argmax(gains))
        assert gains[b], "widen the search"
        seeds.append(b)
        need &= ~rows[b]
    return tuple(seeds)


HVD_SEEDS = (337, 896, 1043, 400, 1024, 208, 17)


def hvd_blocks():
    return [(f"hvd_{s}", hvd_block(s)) for s in HVD_SEEDS]


def to_sm(block: np.ndarray) -> np.ndarray:
    """Signed coefficients -> the oracle's sign-magnitude int32 (bit 31 = sign)."""
    b = block.astype(np.int64)
    return (np.abs(b) | np.where(b < 0, 1 << 31, 0)).astype(np.uint32).view(np.int32)


# --------------------------------------------------------------------------
# images
# --------------------------------------------------------------------------
def blocks16():
    """Every 64x64 block of the 16-bit image, in tile order."""
    out = full_blocks() + [(n, a) for n, a, _ in chain_blocks()] + bernoulli_blocks() + mps_run_blocks() \
        + byteout_blocks() + hvd_blocks()
    assert len(out) <= 64 and len({n for n, _ in out}) == len(out)
    return out


def _twin8(a: np.ndarray) -> np.ndarray:
    """8-bit twin of a 16-bit block: its magnitudes shifted down until the
    largest has 7 bits (32768, sample 0, becomes 128)."""
    m = np.abs(a.astype(np.int64))
    if m.max() == 32768:
        m = m >> 8
    else:
        m = m >> max(0, int(m.max()).bit_length() - 7)
    return (np.sign(a) * m).astype(np.int32)


TWINS8 = ("full_pos", "full_checker", "full_random", "full_min", "chain_serp_fwd", "chain_stair_fwd",
          "chain_ur_steps", "chain_dl_bottom", "bern_1of64_indep", "bern_1of2_indep", "bern_1of2_anti",
          "bern_63of64_indep", "mps_zero", "mps_last", "mps_stripe9", "mps_const_alt")


def blocks8():
    """The 8-bit twins (QuantTab::q16 is off: another index-plane width)."""
    d = dict(blocks16())
    out = [(n + "_8", _twin8(d[n])) for n in TWINS8]
    out += [(f"byteout_{s}_8", byteout_block(s, 127)) for s in BYTEOUT_SEEDS[:8]]
    out += [(n + "_8", a) for n, a in hvd_blocks()[:4]]
    return out


def assemble(blocks, bits: int, per_row: int = 8) -> np.ndarray:
    """One block per 64x64 tile, row-major; the last row is padded with empty
    blocks.  Samples are coefficient + 2^(bits-1)."""
    rows = -(-len(blocks) // per_row)
    img = np.zeros((rows * N, per_row * N), np.int64)
    for i, (_, a) in enumerate(blocks):
        y, x = divmod(i, per_row)
        img[y * N:(y + 1) * N, x * N:(x + 1) * N] = a
    img += 1 << (bits - 1)
    assert img.min() >= 0 and img.max() < (1 << bits)
    return img.astype(np.uint16 if bits == 16 else np.uint8)


# inverse integer 5/3 (F.3.8.2, one level, even lengths) of a Mallat-layout
# array: rows first, undoing a forward transform that ends with them
def _inv53_1d(a, axis):
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    n = a.shape[0] // 2
    s, d = a[:n], a[n:]
    dm1 = np.concatenate([d[:1], d[:-1]])
    even = s - ((dm1 + d + 2) >> 2)
    enext = np.concatenate([even[1:], even[-1:]])
    odd = d + ((even + enext) >> 1)
    x = np.empty_like(a)
    x[0::2], x[1::2] = even, odd
    return np.moveaxis(x, 0, axis)


def inverse_53(bands: np.ndarray) -> np.ndarray:
    """Samples whose one-level reversible transform is `bands` (LL top left,
    HL top right, LH bottom left, HH bottom right)."""
    return _inv53_1d(_inv53_1d(bands, 1), 0)


BAND_NAMES = ("LL", "HL", "LH", "HH")


def band_tiles():
    """Sixteen 128x128 tiles: [(name, [LL, HL, LH, HH])], each band one 64x64
    block from the families at an amplitude that keeps the samples in range."""
    d = dict(blocks16())
    bern = [a for n, a in bernoulli_blocks(planes=11)]
    full = {n: (np.sign(a) * 2047).astype(np.int32) for n, a in full_blocks()}
    chains = [d[n] for n in ("chain_serp_fwd", "chain_stair_fwd", "chain_ur_steps", "chain_dl_inside",
                             "chain_dl_bottom", "chain_halves", "chain_lanes", "chain_down")]
    hvd = [a for _, a in hvd_blocks()]
    out = []
    # every hvd block once as HL and once as HH: their zero-coding tables
    for i in range(7):
        out.append((f"bands_hvd_rot{i}", [hvd[(i + 2) % 7], hvd[i], hvd[(i + 3) % 7], hvd[(i + 1) % 7]]))
    for i in range(3):                                # rotations of densities / chains / full
        out.append((f"bands_bern_rot{i}", [bern[(2 * (b + i) + i // 2) % 10] for b in range(4)]))
    for i in range(4):
        out.append((f"bands_chain_rot{i}", [chains[(b + 2 * i + i // 2) % 8] for b in range(4)]))
    names = list(full)
    for i in range(2):
        out.append((f"bands_full_rot{i}", [full[names[(b + 2 * i) % 5]] for b in range(4)]))
    return out


def bands_image() -> np.ndarray:
    tiles = band_tiles()
    img = np.zeros((4 * 2 * N, 4 * 2 * N), np.int64)
    for i, (_, t) in enumerate(tiles):
        y, x = divmod(i, 4)
        m = np.zeros((2 * N, 2 * N), np.int64)
        m[:N, :N], m[:N, N:], m[N:, :N], m[N:, N:] = t
        img[y * 2 * N:(y + 1) * 2 * N, x * 2 * N:(x + 1) * 2 * N] = inverse_53(m)
    img += 32768
    assert img.min() >= 0 and img.max() < 65536, (img.min(), img.max())
    return img.astype(np.uint16)


GEOMETRY_W = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64)
GEOMETRY_H = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 35, 36, 61, 62, 63, 64)
# (first, second) tile sizes: code-blocks are anchored on the canvas, so the
# second tile is one block only where it ends by sample 64 (or starts there)
_W_PAIRS = ((64, 63), (33, 31), (32, 5), (4, 3), (2, 1))
_H_PAIRS = ((64, 63), (62, 2), (61, 3), (36, 9), (35, 8), (33, 31), (32, 7), (5, 4), (1, 1))


def geometry_cases():
    """Every w x h of GEOMETRY_W x GEOMETRY_H: an image of tile_w + w2 by
    tile_h + h2 samples has one tile of each of four sizes."""
    out = []
    for i, (w1, w2) in enumerate(_W_PAIRS):
        for j, (h1, h2) in enumerate(_H_PAIRS):
            hh = h1 + (h2 if h2 != h1 else 0)
            sizes = [(w, h) for h in dict.fromkeys((h1, h2)) for w in (w1, w2)]
            out.append(dict(name=f"geometry_{w1}+{w2}x{h1}+{h2}", w=w1 + w2, h=hh, tile_w=w1, tile_h=h1,
                            sizes=sizes, bits=16 if (i + j) % 3 else 8, kind=KINDS[(i + 2 * j) % 4],
                            seed=SEED + 100 * i + j))
    assert all(a == N or a + b <= N for a, b in _W_PAIRS + _H_PAIRS)
    assert {s for c in out for s in c["sizes"]} == {(w, h) for w in GEOMETRY_W for h in GEOMETRY_H}
    return out


def geometry_image(c) -> np.ndarray:
    r = np.random.default_rng(c["seed"])
    top = 1 << c["bits"]
    return r.integers(0, top, (c["h"], c["w"])).astype(np.uint16 if c["bits"] == 16 else np.uint8)


# Tiles that do not divide 64: code-blocks are anchored on the canvas, so a
# tile that crosses a multiple of 64 is cut there into blocks narrower or
# shorter than any tile above -- (tile_w, tile_h, image w, image h, bits, kind)
STRADDLE = ((33, 36, 100, 110, 16, "a"), (48, 40, 130, 90, 8, "b"), (63, 61, 200, 130, 16, "c"),
            (5, 7, 70, 70, 8, "d"))


def straddle_cases():
    out = []
    for i, (tw, th, w, h, bits, kind) in enumerate(STRADDLE):
        out.append(dict(name=f"straddle_T{tw}x{th}_{w}x{h}", w=w, h=h, tile_w=tw, tile_h=th, bits=bits, kind=kind,
                        seed=SEED + 5000 + i,
                        sizes=[(min(tw, w - x), min(th, h - y)) for y in range(0, h, th) for x in range(0, w, tw)]))
    return out


# rate_bpp of the rate-driven recipes: about half of recipe (a)'s file, in
# bits per sample (tests/test_t1_blocks.py checks the "about")
RATES = {"blocks16": 0.86, "blocks8": 0.55, "bands": 1.14}
GEOMETRY_RATE = {16: 8.0, 8: 4.0}  # noise does not compress: half the depth


def cases():
    """Every encode of the corpus: dicts of name, group, kind, bits, lossless,
    recipe overrides and `tiles` (tile index -> pattern name and w x h)."""
    out = []
    groups = (("blocks16", 16, blocks16), ("blocks8", 8, blocks8))
    for g, bits, blocks in groups:
        names = [(n, N, N) for n, _ in blocks()]
        for k in KINDS:
            lossless, rc = recipe_for(k, bits, RATES[g])
            out.append(dict(name=f"{g}_{k}", group=g, kind=k, bits=bits, lossless=lossless, recipe=rc, tiles=names))
    names = [(n, 2 * N, 2 * N) for n, _ in band_tiles()]
    for k in KINDS:
        lossless, rc = recipe_for(k, 16, RATES["bands"], levels=1, tile_w=2 * N, tile_h=2 * N)
        out.append(dict(name=f"bands_{k}", group="bands", kind=k, bits=16, lossless=lossless, recipe=rc, tiles=names))
    for c in geometry_cases():
        lossless, rc = recipe_for(c["kind"], c["bits"], GEOMETRY_RATE[c["bits"]], tile_w=c["tile_w"],
                                  tile_h=c["tile_h"])
        out.append(dict(name=f"{c['name']}_{c['bits']}b_{c['kind']}", group="geometry", kind=c["kind"],
                        bits=c["bits"], lossless=lossless, recipe=rc, geometry=c,
                        tiles=[("noise", w, h) for w, h in c["sizes"]]))
    for c in straddle_cases():
        lossless, rc = recipe_for(c["kind"], c["bits"], GEOMETRY_RATE[c["bits"]], tile_w=c["tile_w"],
                                  tile_h=c["tile_h"])
        out.append(dict(name=f"{c['name']}_{c['bits']}b_{c['kind']}", group="straddle", kind=c["kind"],
                        bits=c["bits"], lossless=lossless, recipe=rc, geometry=c,
                        tiles=[("noise, cut at the 64 grid", w, h) for w, h in c["sizes"]]))
    return out


_IMAGES = {}


def image(c) -> np.ndarray:
    """The case's source image (built once per group)."""
    g = c["group"]
    if g in ("geometry", "straddle"):
        return geometry_image(c["geometry"])
    if g not in _IMAGES:
        _IMAGES[g] = {"blocks16": lambda: assemble(blocks16(), 16), "blocks8": lambda: assemble(blocks8(), 8),
                      "bands": bands_image}[g]()
    return _IMAGES[g]


# --------------------------------------------------------------------------
# reading a file back by tile: what a failure is reported with
# --------------------------------------------------------------------------
def _first_sot(cs: bytes) -> int:
    p = 2
    while cs[p:p + 2] != b"\xff\x90":  # main header, segment by segment
        p += 2 + struct.unpack(">H", cs[p + 2:p + 4])[0]
    return p


def tile_part_packets(data: bytes):
    """Per tile-part of a code-stream written with SOP, EPH and PLT:
    (tile index, tile-part bytes, [(packet header, packet body)]), the header
    being what lies between the SOP segment and the EPH marker.  (A packet
    header holds no 0xFF followed by a byte above 0x8F, B.10.1, so the first
    FF92 ends it.)"""
    cs = im.codestream(data)
    walk = im.tile_part_walk(cs, 1)
    p = _first_sot(cs)
    out = []
    for isot, _, _, _, lens in walk:
        assert cs[p:p + 2] == b"\xff\x90"
        psot = struct.unpack(">I", cs[p + 6:p + 10])[0]
        assert struct.unpack(">H", cs[p + 4:p + 6])[0] == isot
        q = p + 12
        while cs[q:q + 2] != b"\xff\x93":
            q += 2 + struct.unpack(">H", cs[q + 2:q + 4])[0]
        q += 2
        pk = []
        for n in lens:
            e = cs.index(b"\xff\x92", q + 6, q + n)
            pk.append((cs[q + 6:e], cs[e + 2:q + n]))
            q += n
        assert q == p + psot
        out.append((isot, cs[p:p + psot], pk))
        p += psot
    return out


def describe_mismatch(case, got: bytes, want: bytes) -> str:
    """Where two files of `case` part: the first tile whose tile-part differs,
    by pattern name and block size, and whether its packet headers or bodies
    differ first."""
    n = min(len(got), len(want))
    d = next((i for i in range(n) if got[i] != want[i]), n)
    msg = f"{case['name']}: {len(got)} vs {len(want)} bytes, first difference at byte {d}"
    try:
        a, b = tile_part_packets(got), tile_part_packets(want)
    except Exception as e:  # the file under test may not even parse
        return f"{msg}; no tile-part walk of the file under test: {e!r}"
    ga, wa = im.codestream(got), im.codestream(want)
    if ga[:_first_sot(ga)] != wa[:_first_sot(wa)]:
        return msg + "; the main headers differ"
    for (ta, ba, pa), (tb, bb, pb) in zip(a, b):
        if ta != tb:
            return msg + f"; tile-part order differs (tile {ta} vs {tb})"
        if ba == bb:
            continue
        name, w, h = case["tiles"][ta] if ta < len(case["tiles"]) else ("padding", N, N)
        msg += f"; first differing tile {ta}: {name}, {w}x{h}"
        for k, ((ha, da), (hb, db)) in enumerate(zip(pa, pb)):
            if ha != hb:
                return msg + (f"; packet {k}: the packet header differs first ({len(ha)} vs {len(hb)} bytes), "
                              f"bodies {len(da)} vs {len(db)} bytes")
            if da != db:
                at = next((i for i in range(min(len(da), len(db))) if da[i] != db[i]), min(len(da), len(db)))
                return msg + (f"; packet {k}: headers agree, the body differs first at its byte {at}; "
                              f"lengths {len(da)} vs {len(db)}" + (" (equal)" if len(da) == len(db) else ""))
        return msg + f"; packets agree, tile-part lengths {len(ba)} vs {len(bb)}"
    return msg + f"; {len(a)} vs {len(b)} tile-parts"
