"""A corpus of steps for one long-lived context (no GPU in this module).

Every other corpus compares one encode with the oracle.  This one is about
what a context carries from one encode to the next: the plan cache (keyed on
width, height, components, bits and the resolved recipe), the tables the
device keeps resident per plan generation, the strip-offset cache, buffers
that only grow, counters left zero by convention, the tier-2 route flags,
the rate state and slope prediction's pmin, the memory policy and the
failure exits.  The steps are chosen so that every piece of that state has a
neighbour that leaves it as it was and one that changes it, and a cache-hit
neighbour always has the buffer sizes and block counts of the step before it
(a missed invalidation would then write a wrong file, never index out of
range).

An encode step is a source (TIFF bytes), a conversion, recipe overrides, a
route and the expected file.  The expected file is the oracle's encode of
the step's pixels (progression_cases.expected for the orders the oracle does
not write); where the source carries metadata the header is
jp2hip.file_header of the TIFF's layout, as in test_gpu_source_metadata.py.
Every step has pixels of its own: two steps of one (w, h, nc, bits) never
expect the same file, so a stale result cannot pass (tests/test_history.py
checks it).  "The same strips, another layout" therefore means the same
geometry and recipe with another layout, not the same pixels.

Routes: "tiff" (encode_tiff), "device" (encode_device on the TIFF in device
memory, `pad` bytes in front of it: every strip offset shifted), "split1"
(encode_split with SingleGroup: the sub-plan has generation 0 and overwrites
the resident tables while the plan cache stays valid), "split2" (the context
under test is rank 1 of a two-rank ThreadGroup: tile0, block0 != 0).

tests/test_gpu_history.py walks the steps; the walks themselves are made
here so that tests/test_history.py can check what they cover.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np

import imaging as im
import ingest_stream_cases as ic
import jp2hip
import metadata_fixtures as mf
import oracle_lib as ol
import pcrd_cases as pc
import pixel_format_cases as pf
import progression_cases as pg
import recipe_axes_cases as rac
import sweep_cases as sc

SEED = 20261022
H, W = 136, 200   # the largest geometry: 3 x 4 tiles of 64^2, the last row and column 8 wide
# every step of the base geometry varies this recipe: four precincts at the
# top resolution, one flush stripe per tile row (so a two-rank split has rows
# for rank 1), one tile-part per tile (every progression order allows that)
BASE = dict(levels=3, layers=6, tile_w=64, tile_h=64, nprecincts=1, prec_w_log2=[5], prec_h_log2=[5], tparts_r=0,
            flush_period=64)


class Step(NamedTuple):
    name: str
    route: str            # "tiff", "device", "split1", "split2"
    lossless: bool
    recipe: dict          # overrides of the conversion's default recipe
    source: object        # () -> (TIFF bytes, the pixels the code-stream holds)
    meta: bool = False    # the source carries metadata: the header is jp2hip.file_header's
    pad: int = 0          # route "device": bytes in front of the TIFF in device memory

    @property
    def conversion(self):
        return jp2hip.LOSSLESS if self.lossless else jp2hip.LOSSY

    @property
    def split(self):
        return self.route in ("split1", "split2")


def _seed(name: str) -> int:
    return SEED + zlib.crc32(name.encode()) % 100000


def _rgb(name, h=H, w=W):
    return sc._content("synth", h, w, 3, 8, _seed(name))


def _strips(name, h=H, w=W, **kw):
    kw.setdefault("rows_per_strip", 16)

    def src():
        px = _rgb(name, h, w)
        return im.tiff_bytes(px, **kw), px
    return src


def _tagged(name):
    def src():
        tif, px = _strips(name)()
        return mf.tag_source(tif, icc=mf.icc_profile(), xres=(300, 1), yres=(300, 1), unit=2), px
    return src


def _gray16be(name):
    def src():
        px = im.synth_u16(H, W, comps=1, seed=_seed(name))
        return im.tiff_bytes(px, rows_per_strip=16, big_endian=True), px
    return src


def _rgba8(name):
    def src():
        px = sc._content("synth", H, W, 4, 8, _seed(name))
        return im.tiff_bytes(px, rows_per_strip=16, alpha=1), px
    return src


def _bilevel(name):
    def src():
        idx = pf.indices(H, W, 1, _seed(name))
        return (pf.make_tiff(idx, 1, pf.WHITE_IS_ZERO, fill_order=2, rows_per_strip=16),
                pf.expand(idx, 1, pf.WHITE_IS_ZERO))
    return src


def _packbits_tiles(name):
    def src():
        px = _rgb(name)
        return im.tiled_tiff_bytes(px, tile=(48, 32), packbits=True), px
    return src


def _pcrd(case):
    def src():
        px = pc.image(case)
        return im.tiff_bytes(px, rows_per_strip=16), px
    return src


def _pcrd_step(name, route, case):
    return Step(name, route, case["lossless"], dict(case["recipe"]), _pcrd(case))


def _base(name, route, lossless=True, source=None, **ov):
    return Step(name, route, lossless, dict(BASE, **ov), source or _strips(name))


def _steps():
    s = [
        # ---- one key: a hit on everything, then the same key with other strip layouts
        _base("base", "tiff"),
        _base("base_px2", "tiff"),
        _base("base_dev", "device"),
        _base("base_rps40", "tiff", source=_strips("base_rps40", rows_per_strip=40)),
        _base("base_shift", "device")._replace(pad=96),   # base_dev's strip count, every offset 96 further
        _base("base_planar", "device", source=_strips("base_planar", planar=True)),
        _base("base_meta", "tiff", source=_tagged("base_meta"))._replace(meta=True),
        # ---- the base geometry, one recipe field away: other tables, the same sizes
        _base("order_cprl", "tiff", progression=pg.CPRL),
        _base("order_lrcp", "device", progression=pg.LRCP),
        _base("prec64", "tiff", prec_w_log2=[6], prec_h_log2=[6]),
        _base("layers1", "tiff", layers=1),
        _base("layers32", "device", layers=32),
        _base("cblk64x16", "tiff", nprecincts=0, cblk_w_log2=6, cblk_h_log2=4),
        _base("cblk16x64", "device", nprecincts=0, cblk_w_log2=4, cblk_h_log2=6),
        _base("no_sop_eph", "tiff", sop=0, eph=0),
        _base("no_plt", "tiff", plt=0),
        _base("mct0", "device", mct=0),
        _base("tparts_r1", "tiff", tparts_r=1),
        # ---- lossy on the same geometry; slope prediction on (pmin written) and off.  8 bits per pixel: the
        # packet headers of these small tiles alone take more than the default 3 would give the whole file
        _base("lossy_skip1", "tiff", lossless=False, rate_bpp=8.0, slope_skip=1),
        _base("lossy_skip0", "device", lossless=False, rate_bpp=8.0, slope_skip=0),
        # ---- other pipelines: no decomposition (k_ingest, no llbuf) and five levels
        _base("levels0", "tiff", levels=0),
        _base("levels5", "tiff", levels=5),
        # ---- the rate loop's rarer doors and the tier-2 routes (pcrd_cases: 256^2 grey, 16^2 blocks, no
        # decomposition): the prediction's safety-net rerun on precincts of one block (k_t2_wave), three
        # iterations on precincts of 128 blocks and a lossless tile of one 256-block precinct (the serial route)
        _pcrd_step("pcrd_safety_p1", "tiff", pc.by_name("extremes_skip_safety_net_p1")),
        _pcrd_step("pcrd_iter3_p128", "device", pc.by_name("iterations_it3_fits_nearties_ly32_b19220_p128")),
        _pcrd_step("serial256", "tiff", pc.make_case("history", "serial256", "hull", "p128", True, layers=6,
                                                     tile_w=pc.SIDE, tile_h=pc.SIDE, flush_period=1024)),
        # ---- sizes: after the largest, buffers keep a dirty tail
        _base("tiny17x9", "tiff", source=_strips("tiny17x9", 9, 17)),
        _base("one1x1", "device", source=_strips("one1x1", 1, 1)),
        # ---- pixel formats
        _base("gray16be", "tiff", source=_gray16be("gray16be")),
        _base("rgba8", "tiff", source=_rgba8("rgba8"))._replace(meta=True),
        _base("bilevel", "tiff", source=_bilevel("bilevel")),
        # ---- compressed sources (the unpack buffers and their error word)
        _base("lzw_pred2", "tiff", source=_strips("lzw_pred2", strip_codec=im.lzw_encode, compression=5, predictor=2)),
        _base("deflate", "device", source=_strips("deflate", strip_codec=zlib.compress, compression=8)),
        _base("packbits_tiles", "tiff", source=_packbits_tiles("packbits_tiles")),
        # ---- splits on the base key
        _base("split_single", "split1"),
        _base("split_rank1", "split2"),
    ]
    assert len({x.name for x in s}) == len(s)
    return s


STEPS = _steps()
N = len(STEPS)
NAMES = [s.name for s in STEPS]


def index(name: str) -> int:
    return NAMES.index(name)


@functools.lru_cache(maxsize=None)
def source(i: int):
    """(TIFF bytes, pixels) of step i."""
    return STEPS[i].source()


def recipe(step):
    return jp2hip.recipe(step.conversion, **step.recipe)


@functools.lru_cache(maxsize=None)
def expected(i: int) -> bytes:
    """The file step i must produce, whatever its context encoded before."""
    step = STEPS[i]
    tif, px = source(i)
    rc = recipe(step)
    want = pg.expected(px, rc) if rc.progression != pg.RPCL else ol.encode(px, ol.copy_recipe(rc))
    if step.meta:
        cs = im.codestream(want)
        want = jp2hip.file_header(jp2hip.tiff_layout(tif)[0], rc.format, len(cs)) + cs
    return want


@functools.lru_cache(maxsize=None)
def geometry(i: int):
    """(w, h, components, bits) of the code-stream: the plan cache's key
    beside the recipe."""
    lay = jp2hip.tiff_layout(source(i)[0])[0]
    return (lay.width, lay.height) + jp2hip.encoded_format(lay)


@functools.lru_cache(maxsize=None)
def key(i: int):
    """What the plan cache compares: geometry and every recipe field."""
    rc = recipe(STEPS[i])
    vals = []
    for name, _ in jp2hip._lib.Recipe._fields_:
        v = getattr(rc, name)
        vals.append(tuple(v) if hasattr(v, "__len__") else v)
    return geometry(i) + tuple(vals)


def cache_hit_pairs():
    """(a, b): b right after a finds the plan, the front's tables and the
    tier-2 tables in place (one key, neither a split)."""
    return [(a, b) for a in range(N) for b in range(N)
            if key(a) == key(b) and not STEPS[a].split and not STEPS[b].split]


# ---- failure steps: only failures the suite provokes elsewhere, all of which return an error ----
class Failure(NamedTuple):
    name: str
    match: str            # what the message says
    tiff: object = None   # () -> TIFF bytes; None: the encode step `of`
    lossless: bool = True
    recipe: object = None  # overrides; None: the default recipe (or `of`'s)
    of: str = ""          # hard limit: the encode step that runs under the cap
    frac: float = 0.0     # ... at this fraction of what that step needs on a fresh context


def _corrupt_deflate():
    img = im.synth_rgb8(64, 64, seed=1)
    data = bytearray(im.tiff_bytes(img, rows_per_strip=32, strip_codec=zlib.compress, compression=8))
    lay, _ = jp2hip.tiff_layout(bytes(data))
    data[lay.strip_offsets[1] + 2] = 0x07  # BFINAL 1, BTYPE 3 (reserved): test_gpu_parity's "bad_block"
    return bytes(data)


FAILURES = [
    Failure("deflate_corrupt", "corrupt", _corrupt_deflate),
    Failure("lzw_invalid_mid_segment", "corrupt", lambda: ic.lzw_error_pair("invalid_mid_segment", "parallel")[0].tiff()),
    Failure("bad_recipe", rac.BAD[0][0], lambda: source(index("base"))[0], lossless=False, recipe=rac.BAD[0][1]),
    Failure("hard_0.3", "device memory limit", of="gray16be", frac=0.3),
    Failure("hard_0.9", "device memory limit", of="gray16be", frac=0.9),
]
FAILURE_NAMES = [f.name for f in FAILURES]
# the steps encoded after a failure: base, lossy, no decomposition, a compressed source, a split
AFTER_FAILURE = ("base", "lossy_skip1", "levels0", "lzw_pred2", "split_single")
# the context is small when a hard-limit step begins (so the cap holds from its first allocation)
BEFORE_FAILURE = {"hard_0.3": "tiny17x9", "hard_0.9": "tiny17x9"}
# pair walks repeated with a trim after every encode
TRIM_ROWS = ("base", "lossy_skip1", "pcrd_iter3_p128")


# ---- walks ----
def pair_walk(a: int, n: int = N) -> list:
    """A, B0, A, B1, ..., A, A: every ordered pair with A in it."""
    out = []
    for b in range(n):
        if b != a:
            out += [a, b]
    return out + [a, a]


def pairs_of(walk) -> set:
    return set(zip(walk, walk[1:]))


WALK_SEEDS = (1, 2, 3, 4)
WALK_LENGTH = 60


def random_walk(seed: int, length: int = WALK_LENGTH) -> list:
    """`length` tokens: ("encode", step index), ("fail", failure index) or
    ("trim",) -- the next encode runs with the soft limit at 1 byte, so it
    ends by releasing the context's buffers."""
    rng = np.random.default_rng([SEED, seed])
    out = []
    for _ in range(length):
        r = rng.random()
        if r < 0.12:
            out.append(("fail", int(rng.integers(len(FAILURES)))))
        elif r < 0.22:
            out.append(("trim",))
        else:
            out.append(("encode", int(rng.integers(N))))
    return out
