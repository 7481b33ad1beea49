"""The crafted PCRD / rate-loop corpus (tests/pcrd_cases.py) on the CPU: that
between them the cases reach every cell of the oracle's PCRD census and of the
device's path determinants except those in an explicit, reasoned list; that
the oracle's selection is the documented rule, checked against a plain model
that shares no code with it (sort, group equal keys, take whole groups while
they fit; the hull in exact fractions); that the committed budgets are what
the committed searches find; and that every case still sits on the path it
was built for (pcrd_cases.PINS).
"""
import math
import struct
from fractions import Fraction

import pytest

import imaging as im
import oracle_lib as ol
import pcrd_cases as pc

CASES = pc.cases()
IDS = [c["name"] for c in CASES]
K = pc.library_constants()


# ---- the constants are read, not restated ---------------------------------
def test_constants_are_read_from_the_library_sources():
    assert set(K) == {"kPcrdBins", "kPcrdBinBase", "kSelBrute", "kResLog2"}
    assert all(isinstance(v, int) and v > 0 for v in K.values())
    # what the construction relies on: a bin is 2^47 keys, narrowed 2^kResLog2 ways a round
    assert K["kPcrdBins"] % 256 == 0 and 47 > K["kResLog2"]


def test_images_are_small_and_blocks_are_tiles():
    for c in CASES:
        img = pc.image(c)
        assert img.shape == (pc.SIDE, pc.SIDE) and pc.SIDE <= 512
        r = c["recipe"]
        assert r["levels"] == 0 and r["mct"] == 0 and r["cblk_w_log2"] == 4 and r["cblk_h_log2"] == 4
        assert pc.blocks_per_precinct(c) in (1, 128)
        assert len(pc.measure(c)["export"]["blocks"]) == pc.NB


def test_counting_and_exporting_change_no_byte():
    for name in ("ties_tie65_exact_p128", "extremes_skip_safety_net_p1", "nearties_lossless_ly12_p1"):
        c = pc.by_name(name)
        ol.pcrd_export_enable(False)
        plain = ol.encode(pc.image(c), ol.recipe(c["lossless"], **c["recipe"]))
        assert ol.pcrd_export()["segments"] == [] and plain == pc.measure(c)["file"]


# ---- census completeness ---------------------------------------------------
def unreachable_cells() -> dict:
    """{cell: reason}: the only way to leave a cell of the oracle's PCRD census
    or of pcrd_cases.PATH_CELLS out of the corpus."""
    return {
        "hull_np_gt88": "a block of Mb magnitude bit-planes has at most 3 Mb - 2 passes and build_plan refuses "
                        "Mb > 30 (plan.cpp: 'band needs more than 30 magnitude bit-planes'): 88 passes at the most; "
                        "the deep cases reach 88",
        "sel_tie_one_block": "a block's hull slopes strictly decrease (build_hull pops on s >= top), so two "
                             "segments with one key never belong to one block",
        "bin_top": "a hull slope is squared error in sample units per byte: at most the whole energy of a block, "
                   "64*64 samples * (2^16)^2 * the largest synthesis gain * component weight (< 2^4) = 2^48 over "
                   "one byte, far below the top bin's lower edge 2^(64 - 1/32)",
        "bin_bin0": "slope >= 1 * weight / dR with weight = Delta^2 G compw / 4, Delta >= 2^(8 - 31) (eps <= 31), "
                    "dR < 2^15.02 (64*64*8 + 256): in this corpus (LL of level 0, one component, G = compw = 1) "
                    "slope >= 2^-63.02, above bin 0's upper edge 2^-63.96.  Other recipes: a search of 8-bit noise, "
                    "smooth, sparse and near-constant 128x128 images, 1 and 3 components, levels 0..2, qstep 2^-31, "
                    "guard_bits 0 found no segment below bin 671 (2^-43)",
    }


def corpus_totals():
    cen, paths = None, dict.fromkeys(pc.PATH_CELLS, 0)
    for c in CASES:
        m = pc.measure(c)
        cen = ol.pcrd_census_add(cen, m["census"])
        for k in pc.PATH_CELLS:
            paths[k] += m["paths"][k]
    return dict(cen, **paths)


def test_corpus_reaches_every_cell_but_the_listed_ones():
    tot = corpus_totals()
    assert set(tot) == set(ol.PCRD_CELLS) | set(pc.PATH_CELLS)
    unreachable = unreachable_cells()
    assert set(unreachable) <= set(tot)
    assert all(len(r) > 40 for r in unreachable.values())
    for cell in ("rate_iterations_1", "rate_iterations_2", "rate_iterations_3", "rate_iterations_8"):
        assert cell not in unreachable          # measured in the suite's own sweeps
    missed = [k for k, v in tot.items() if not v and k not in unreachable]
    assert not missed, missed
    reached = [k for k in unreachable if tot[k]]
    assert not reached, f"listed as unreachable, yet reached: {reached}"


def test_every_family_is_given_on_both_tier2_routes():
    for fam in ("ties", "extremes", "nearties", "hull", "iterations"):
        routes = {c["route"] for c in CASES if c["family"] == fam}
        assert routes == {"p1", "p128"}, (fam, routes)
    for c in CASES:
        p = pc.measure(c)["paths"]
        assert p["t2_precincts_gt_64"] == (c["route"] == "p128") and p["t2_precincts_le_64"] == (c["route"] == "p1")


def test_every_iteration_count_is_in_the_corpus():
    seen = {(pc.measure(c)["export"]["iterations"], bool(pc.measure(c)["census"]["rate_stopped_under_target"]))
            for c in CASES if c["rate_driven"]}
    assert {n for n, _ in seen} == set(range(1, 9))
    assert (8, True) in seen and (8, False) in seen   # the eighth iteration fits / stops over the target


# ---- the committed budgets are what the searches find ---------------------
def test_committed_budgets_are_what_the_searches_find():
    assert pc.search_tie_budgets() == pc.TIE_BUDGETS
    assert pc.search_safety_net() == pc.SAFETY_NET_BUDGETS
    assert pc.search_iterations() == pc.ITERATION_PAIRS


# ---- a plain model of the rule ---------------------------------------------
def model_select(segs, budget):
    """The documented rule, by sorting: walk the segments by decreasing key,
    equal keys together, take whole groups while they fit.  -> (bytes taken,
    Kc = first key not taken + 1 or 0, bytes of the first group not taken,
    its size)."""
    order = sorted(segs, key=lambda s: -s[0])
    taken, i = 0, 0
    while i < len(order):
        j = i
        while j < len(order) and order[j][0] == order[i][0]:
            j += 1
        grp = sum(n for _, n in order[i:j])
        if taken + grp > budget:
            return taken, order[i][0] + 1, grp, j - i
        taken += grp
        i = j
    return taken, 0, 0, 0


def layer_info(data: bytes):
    """[(slope text, bytes text)] of the Kdu-Layer-Info comment."""
    cs = im.codestream(data)
    at = cs.index(b"Kdu-Layer-Info")
    n = struct.unpack(">H", cs[at - 4:at - 2])[0]
    text = cs[at:at + n - 4].decode("latin-1")   # (Lcom counts itself and Rcom)
    return [tuple(x.strip() for x in line.split(",")) for line in text.split("\n")[1:] if line.strip()]


def log_slope_text(Kc: int, bits: int) -> str:
    """oracle layer_log_slope, restated: what Kdu-Layer-Info prints for Kc."""
    if Kc == 0:
        v = -192.0
    elif Kc >= 0x7FF0000000000000:
        v = 192.0
    else:
        v = math.log2(struct.unpack("<d", struct.pack("<Q", Kc))[0]) - 2.0 * bits
        v = min(192.0, max(-192.0, v))
    return ("%6.1f" % v).strip()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_selection_is_the_rule(case):
    m = pc.measure(case)
    exp, L = m["export"], case["recipe"]["layers"]
    groups = sorted({s[3] for s in exp["segments"]} | {l["group"] for l in exp["layers"]})
    Kc_file = [0] * L
    for g in groups:
        segs = [(k, n) for k, n, _, gg in exp["segments"] if gg == g]
        assert [k for k, _ in segs] == sorted((k for k, _ in segs), reverse=True)
        assert all(n > 0 for _, n in segs)
        lay = sorted((l for l in exp["layers"] if l["group"] == g), key=lambda l: l["layer"])
        assert [l["layer"] for l in lay] == list(range(L))
        for l in lay:
            last_lossless = not case["rate_driven"] and l["layer"] == L - 1
            budget = max(l["budget"], 0)
            taken, Kc, grp, _ = model_select(segs, budget)
            if last_lossless:  # every pass, by rule; its budget (all tier-1 bytes) says the same
                assert l["Kc"] == 0 and Kc == 0
            assert l["Kc"] == Kc, (g, l, Kc)
            assert taken <= budget                       # fits
            assert Kc == 0 or taken + grp > budget       # and the next tie group would not (maximality)
            assert taken == sum(n for k, n in segs if k >= Kc) if Kc else taken == sum(n for _, n in segs)
            Kc_file[l["layer"]] = max(Kc_file[l["layer"]], Kc)
    # the device's rule (histogram, narrowing rounds) arrives at the same keys
    for p in m["paths"]["layers"]:
        assert p["Kc"] == p["oracle_Kc"], p
    # the file says so: Kdu-Layer-Info holds the strictest group's key
    info = layer_info(m["file"])
    assert [s for s, _ in info] == [log_slope_text(k, case["bits"]) for k in Kc_file]
    # and every block's layer table is its hull cut at the group's threshold
    first = {}
    for i, (_, _, b, g) in enumerate(exp["segments"]):
        first.setdefault(b, g)
    thr = {(l["group"], l["layer"]): l["K"] for l in exp["layers"]}
    for b, blk in enumerate(exp["blocks"]):
        g = first.get(b)
        for l in range(L):
            if not case["rate_driven"] and l == L - 1:
                want = len(blk["rates"])
            elif g is None:
                want = 0
            else:
                keys = [struct.unpack("<Q", struct.pack("<d", s))[0] for s in blk["hslope"]]
                want = max([blk["hull"][i] for i in range(1, len(keys)) if keys[i] >= thr[(g, l)]], default=0)
            assert blk["nl"][l] == want, (b, l)


TIE_CASES = [c for c in CASES if c["family"] == "ties" and c["rate_driven"] and c["recipe"]["layers"] == 1]


@pytest.mark.parametrize("case", TIE_CASES, ids=[c["name"] for c in TIE_CASES])
def test_tie_budgets_sit_where_the_names_say(case):
    """exact: the first iteration's budget is used to the byte and ends on a
    whole tie group of N; short: that group is the first not taken and misses
    by one byte; over: one byte of the budget is left."""
    n = pc.TIE_IMAGES[case["image"]]
    segs = [(k, b) for k, b, _, _ in pc.measure(case)["export"]["segments"]]
    tag = case["name"].split("_")[2]
    budget = pc.TIE_BUDGETS[case["image"]] + {"exact": 0, "short": -1, "over": 1}[tag]
    taken, Kc, grp, size = model_select(segs, budget)
    by_key = {}
    for k, _ in segs:
        by_key[k] = by_key.get(k, 0) + 1
    last_taken = min(k for k, _ in segs if k >= Kc)
    if tag == "short":
        assert size >= n and taken + grp == budget + 1
    else:
        assert by_key[last_taken] >= n and taken == pc.TIE_BUDGETS[case["image"]]
    assert (n > K["kSelBrute"]) == (case["image"] != "tie60")


# ---- the hull in exact arithmetic -------------------------------------------
def _i64(v: int) -> int:
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def exact_hull(rates, dd, wrap):
    """Upper convex hull of (bytes, distortion decrease) over the passes, by
    the definition, slopes compared as fractions: a pass joins while slopes
    strictly decrease; a pass that adds no distortion decrease over the top is
    skipped.  wrap: the sums of distortion in 64-bit two's complement, as
    both implementations keep them."""
    fix = _i64 if wrap else (lambda v: v)
    D, R = [0], [0]
    for r, d in zip(rates, dd):
        D.append(fix(D[-1] + d))
        R.append(r)
    hull, slope = [0], [None]
    for n in range(1, len(R)):
        while True:
            h = hull[-1]
            dD, dR = fix(D[n] - D[h]), R[n] - R[h]
            if dD <= 0:
                break
            if dR <= 0 or (len(hull) >= 2 and Fraction(dD, dR) >= slope[-1]):
                hull.pop()
                slope.pop()
                continue
            hull.append(n)
            slope.append(Fraction(dD, dR))
            break
    return hull, slope, D, R


_HULLS = {}


def hull_report(case):
    """(blocks whose hull in doubles differs from the one in fractions, blocks
    whose distortion sums pass 2^63); computed once per distinct set of blocks
    (the routes and rates share their hulls)."""
    blocks = pc.measure(case)["export"]["blocks"]
    key = hash(tuple((tuple(b["rates"]), tuple(b["dd"]), b["weight"]) for b in blocks))
    if key not in _HULLS:
        rounding, overflow = [], []
        for i, b in enumerate(blocks):
            hull, slope, D, R = exact_hull(b["rates"], b["dd"], wrap=False)
            # the exact hull is one: slopes strictly decrease, no pass lies above it
            assert all(slope[j] > slope[j + 1] for j in range(1, len(slope) - 1))
            for n in range(1, len(R)):
                j = max(j for j in range(len(hull)) if R[hull[j]] <= R[n] or j == 0)
                if j + 1 < len(hull):
                    a, z = hull[j], hull[j + 1]
                    top = D[a] + Fraction((D[z] - D[a]) * (R[n] - R[a]), R[z] - R[a])
                else:
                    top = D[hull[-1]]
                assert D[n] <= top, (i, n)
            # the oracle's: strictly decreasing doubles; the same points unless a sum wrapped
            hs = b["hslope"]
            assert all(hs[j] > hs[j + 1] for j in range(1, len(hs) - 1)), i
            # (a pass may raise the distortion a little; one below -2^62 is a sum that wrapped in tier-1)
            wrapped = max(abs(d) for d in D) >= 1 << 63 or min(b["dd"], default=0) < -(1 << 62)
            if wrapped:
                overflow.append(i)
            elif b["hull"] != hull:
                rounding.append(i)
            if wrapped and b["hull"] != exact_hull(b["rates"], b["dd"], wrap=True)[0]:
                rounding.append(i)
        _HULLS[key] = (rounding, overflow)
    return _HULLS[key]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hull_is_the_exact_hull(case):
    """Recorded, not hidden: PINS holds the number of blocks where rounding
    the slopes to doubles moves a hull point (none in this corpus), and the
    number of blocks whose distortion sums do not fit 64 bits.  The latter is
    a defect both implementations share: with 30 magnitude bit-planes (the
    deep and finest-step cases) one sample's squared error reaches 2^62, a
    pass's sum and the running total wrap, and the hull is that of the wrapped
    numbers -- byte-identical on both sides, but not the convex hull of the
    block's true rate-distortion points."""
    rounding, overflow = hull_report(case)
    pin = pc.PINS[case["name"]]
    assert (len(rounding), len(overflow)) == (pin["hull_rounding_blocks"], pin["hull_overflow_blocks"]), \
        (rounding, overflow)


# ---- pins --------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_stays_on_its_path(case):
    pc.check_pins(case)


def test_pins_name_every_case_and_nothing_else():
    assert set(pc.PINS) == {c["name"] for c in CASES}
