"""One context, many encodes: its output must not depend on what it encoded
before (tests/history_cases.py has the steps and why each is there).

Every context here is fresh -- never the session's `encoder` -- and every
output is compared byte for byte with the step's expected file, which comes
from the oracle alone.  jp2hip_stats.reused says which caches an encode hit,
so the walks do not merely hope to pass through the reuse paths: each encode's
plan-cache and resident-table bits are compared with a small model of the
context (Walker), and test_census asserts that every bit was seen set and
seen clear where the library can set it.

Nothing here breaks an invalidation to see a test fail: stale tables of
another size could index out of range.  The census is the evidence that both
sides of each branch were taken.
"""
import os
import re
import threading

import pytest

import history_cases as hc
import jp2hip
import progression_cases as pg
from jp2hip import split as js

pytestmark = pytest.mark.gpu

PLAN, FRONT, T2, STRIPS, TRIM, FAILED = (jp2hip._lib.REUSED_PLAN, jp2hip._lib.REUSED_FRONT_TABLES,
                                         jp2hip._lib.REUSED_T2_TABLES, jp2hip._lib.REUSED_STRIPS,
                                         jp2hip._lib.AFTER_TRIM, jp2hip._lib.AFTER_FAILURE)
UNKNOWN = object()

# (test, route, what ran before on the context: a route, "failure" or None, reused) of every encode
CENSUS = []
_ROWS_DONE = set()   # pair walks of test a that ran to their end
_DEV = {}            # device copies of the sources, freed when the module is done
_NEED = {}


@pytest.fixture(scope="module", autouse=True)
def _device_sources():
    yield
    for d in _DEV.values():
        d[0].free()
    _DEV.clear()


def _device(i, rank=None):
    """(DeviceBytes, layout, its offsets array) of step i's source: the whole
    TIFF behind `pad` bytes, or rank `rank`'s band of a two-rank split."""
    if (i, rank) not in _DEV:
        from devmem import DeviceBytes
        step = hc.STEPS[i]
        tif = hc.source(i)[0]
        lay, keep = jp2hip.tiff_layout(tif)
        if rank is None:
            for k in range(lay.nstrips):
                keep[k] += step.pad
            buf = b"\xa5" * step.pad + tif
        else:
            rc = hc.recipe(step)
            r0, r1 = js.split_rows(lay.height, rc.tile_h, rank, 2, rc.flush_period)
            assert r1 > r0
            buf, lay, keep = js.band_strips(tif, lay, keep, r0, r1)
        _DEV[(i, rank)] = (DeviceBytes(buf), lay, keep)
    return _DEV[(i, rank)]


def run_step(enc, i, helper=None):
    """Step i on `enc` by the step's route: (the whole file, enc's Stats)."""
    step = hc.STEPS[i]
    rc, conv = hc.recipe(step), step.conversion
    if step.route == "tiff":
        return enc.encode_tiff(hc.source(i)[0], conv, rc)
    if step.route == "device":
        d, lay, _ = _device(i)
        return enc.encode_device(d.ptr, d.nbytes, lay, conv, rc)
    if step.route == "split1":
        d, lay, _ = _device(i)
        part, off, flen, st = js.encode_split(enc, d.ptr, d.nbytes, lay, conv, js.SingleGroup(), rc)
        assert off == 0 and flen == len(part)
        return part, st
    # two ranks as threads; `enc` is rank 1, `helper` encodes the rows above
    g = js.ThreadGroup(2)
    members = [g.member(0), g.member(1)]
    parts, errs = [None, None], []

    def work(r, e):
        try:
            d, blay, _ = _device(i, r)
            parts[r] = e.encode_device_split(d.ptr, d.nbytes, blay, conv, members[r].split(), rc)
        except Exception as ex:  # keep the other rank from waiting for ever
            errs.append(ex)
            g.abort()

    t = threading.Thread(target=work, args=(0, helper))
    t.start()
    work(1, enc)
    t.join(timeout=60)
    assert not t.is_alive(), "rank 0 of the split did not return"
    if errs:
        raise errs[0]
    assert parts[0][1] == 0 and parts[1][1] == len(parts[0][0]) > 0
    assert parts[0][2] == parts[1][2] == len(parts[0][0]) + len(parts[1][0])
    return parts[0][0] + parts[1][0], parts[1][3]


def need_of(i):
    """Device bytes a fresh context holds after step i: the step's own need."""
    if i not in _NEED:
        enc, helper = jp2hip.Encoder(0), jp2hip.Encoder(0)
        try:
            run_step(enc, i, helper)
            _NEED[i] = enc.device_bytes()
        finally:
            enc.close()
            helper.close()
    return _NEED[i]


class Walker:
    """A fresh context, what it has done so far, and what its next encode
    must therefore report: the plan cache holds the key of the last encode
    that was not a split; the tables of that plan are resident until a split
    (generation 0 tables), a trim or another plan replaces them; bits 16 and
    32 tell how the call before ended."""

    def __init__(self, test):
        self.test = test
        self.enc = jp2hip.Encoder(0)
        self.helper = None
        self.history = []
        self.pc_key = None      # the cached plan's key (None: no valid plan)
        self.tables = False     # that plan's tables are on the device
        self.after = 0          # TRIM | FAILED of the call before (None: not predicted)
        self.prev = None
        self.pool_grows = 0     # encodes repeated because the decision-stream pool was short

    def close(self):
        self.enc.close()
        if self.helper is not None:
            self.helper.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _where(self, label):
        return f"{label} after {self.history[-3:]} (encode {len(self.history)} of the context)"

    def _run(self, i):
        if hc.STEPS[i].route == "split2" and self.helper is None:
            self.helper = jp2hip.Encoder(0)
        return run_step(self.enc, i, self.helper)

    def _limits(self, trim, hard=0):
        self.enc.set_memory_limits(soft=1 if trim else 0, hard=hard)

    def _encoded(self, i, label, got, st, trim):
        step = hc.STEPS[i]
        diff = pg.first_difference(bytes(got), hc.expected(i))
        assert diff is None, f"{self._where(label)}: not the oracle's file: {diff} (reused {st.reused})"
        r = st.reused
        if self.after is not None:
            assert r & (TRIM | FAILED) == self.after, f"{self._where(label)}: reused {r}, the call before ended {self.after}"
        if step.split:
            assert r & (PLAN | FRONT | T2) == 0, f"{self._where(label)}: a split reports reused {r}"
        elif self.pc_key is not UNKNOWN:
            hit = self.pc_key == hc.key(i)
            assert bool(r & PLAN) == hit, f"{self._where(label)}: reused {r}, plan cache hit expected: {hit}"
            if self.tables is not UNKNOWN:
                want = (FRONT | T2) if hit and self.tables else 0
                assert r & (FRONT | T2) == want, f"{self._where(label)}: reused {r}, resident tables expected: {want}"
        CENSUS.append((self.test, step.route, self.prev, r))
        self.pool_grows += st.pool_grows
        if step.split:
            self.tables = False
        else:
            self.pc_key, self.tables = hc.key(i), True
        if trim:
            self.tables = False
        self.after = TRIM if trim else 0
        self.prev = step.route
        self.history.append(label)
        return r

    def encode(self, i, trim=False):
        """Step i; trim: under a soft limit of one byte, so it ends by
        releasing every buffer."""
        label = hc.NAMES[i] + ("+trim" if trim else "")
        self._limits(trim)
        try:
            got, st = self._run(i)
        except Exception as e:
            raise AssertionError(f"{self._where(label)}: {e}") from e
        finally:
            self._limits(False)
        assert self.enc.device_bytes() == 0 if trim else self.enc.device_bytes() > 0, self._where(label)
        return self._encoded(i, label, got, st, trim)

    def fail(self, j, trim=False, strict=True):
        """Failure step j.  A hard-limit step fails for certain only while the
        context holds less than the cap (strict); in a random walk the
        context may hold the step's buffers already, and the step then either
        fails with the limit's message or encodes the oracle's file."""
        f = hc.FAILURES[j]
        label = f.name + ("+trim" if trim else "")
        if f.of:
            i = hc.index(f.of)
            cap = int(need_of(i) * f.frac)
            below = self.enc.device_bytes() <= cap
            assert below or not strict, f"{self._where(label)}: the context holds more than the cap already"
            self._limits(trim, hard=cap)
            try:
                got, st = self._run(i)
            except jp2hip.Jp2hipError as e:
                assert re.search(f.match, str(e)), f"{self._where(label)}: {e}"
                if below:
                    assert self.enc.device_bytes() <= cap, self._where(label)
            else:
                assert not strict, f"{self._where(label)}: encoded under a cap of {cap} bytes"
                self._limits(False)
                return self._encoded(i, label, got, st, trim)
            finally:
                self._limits(False)
            self.pc_key = self.tables = UNKNOWN   # wherever the limit caught it
            self.after = (FAILED | (TRIM if trim else 0)) if strict else None
        else:
            conv = jp2hip.LOSSLESS if f.lossless else jp2hip.LOSSY
            rc = jp2hip.recipe(conv, **f.recipe) if f.recipe else None
            self._limits(trim)
            try:
                with pytest.raises(jp2hip.Jp2hipError, match=f.match):
                    self.enc.encode_tiff(f.tiff(), conv, rc)
            finally:
                self._limits(False)
            if f.recipe:          # refused by the plan: the cache holds no plan now
                self.pc_key, self.tables = None, False
            elif trim:            # a corrupt source fails before the plan is looked at
                self.tables = False
            self.after = FAILED | (TRIM if trim else 0)
        self.prev = "failure"
        self.history.append(label)
        return None


# ---- a. every ordered pair ----
def _pair_row(a):
    with Walker("a") as w:
        for i in hc.pair_walk(a):
            w.encode(i)
    _ROWS_DONE.add(a)


@pytest.mark.parametrize("a", range(hc.N), ids=hc.NAMES)
def test_every_ordered_pair(a):
    """A, B0, A, B1, ..., A, A on one context: with the other rows, every
    ordered pair of steps, every single output checked."""
    _pair_row(a)


# ---- b. after a failure ----
@pytest.mark.parametrize("b", hc.AFTER_FAILURE)
@pytest.mark.parametrize("j", range(len(hc.FAILURES)), ids=hc.FAILURE_NAMES)
def test_after_a_failure(j, b):
    """A, F, B and, on a context of its own, F, B: B is the oracle's file and
    reports that the call before it failed."""
    f = hc.FAILURES[j]
    a = hc.index(hc.BEFORE_FAILURE.get(f.name, "base"))
    for first in ([a], []):
        with Walker("b") as w:
            for i in first:
                w.encode(i)
            w.fail(j)
            r = w.encode(hc.index(b))
            assert r & FAILED


# ---- c. a trim between every pair ----
@pytest.mark.parametrize("name", hc.TRIM_ROWS)
def test_pair_walk_with_a_trim_after_every_encode(name):
    """Every encode starts from no buffers at all while the plan cache holds."""
    with Walker("c") as w:
        for k, i in enumerate(hc.pair_walk(hc.index(name))):
            r = w.encode(i, trim=True)
            assert r & (FRONT | T2 | STRIPS) == 0 and bool(r & TRIM) == (k > 0)


# ---- d. seeded random walks ----
@pytest.mark.parametrize("seed", hc.WALK_SEEDS)
def test_random_walk(monkeypatch, seed):
    """Encode steps, failure steps and trims in a seeded order; the first
    walk on a context whose decision-stream pool starts at 2 % of the bound,
    so pool_hint and the grow path take part."""
    short_pool = seed == hc.WALK_SEEDS[0]
    if short_pool:
        monkeypatch.setenv("JP2HIP_TEST_POOL_FRAC", "0.02")
    w = Walker("d")
    if short_pool:
        monkeypatch.delenv("JP2HIP_TEST_POOL_FRAC")
    with w:
        trim = False
        for tok in hc.random_walk(seed):
            if tok[0] == "trim":
                trim = True
                continue
            if tok[0] == "encode":
                w.encode(tok[1], trim=trim)
            else:
                w.fail(tok[1], trim=trim, strict=False)
            trim = False
        assert w.pool_grows > 0 or not short_pool


# ---- e. two contexts of one device, one thread ----
def test_two_contexts_alternating():
    """They share only what the process shares: plan generations, the pinned
    output pool, the registry reclaim walks."""
    rows = [hc.pair_walk(hc.index("base")), hc.pair_walk(hc.index("lossy_skip1"))]
    with Walker("e") as w0, Walker("e") as w1:
        for i0, i1 in zip(*rows):
            w0.encode(i0)
            w1.encode(i1)


# ---- f. the census ----
def _seen(records, bit):
    return (sum(1 for r in records if r[3] & bit), sum(1 for r in records if not r[3] & bit))


def census_table():
    """{row: {bit: (times set, times clear)}} over the encodes so far."""
    rows = {"pair walks": [r for r in CENSUS if r[0] == "a"]}
    for route, label in ((("tiff",), "route encode_tiff"), (("device",), "route encode_device"),
                         (("split1", "split2"), "route split")):
        rows[label] = [r for r in CENSUS if r[0] == "a" and r[1] in route]
    rows["right after a split"] = [r for r in CENSUS if r[0] == "a" and r[2] in ("split1", "split2")]
    for test, label in (("b", "after a failure"), ("c", "trim walks"), ("d", "random walks"), ("e", "two contexts")):
        rows[label] = [r for r in CENSUS if r[0] == test]
    return {k: {bit: _seen(v, bit) for bit in (PLAN, FRONT, T2, STRIPS, TRIM, FAILED)} | {"encodes": len(v)}
            for k, v in rows.items()}


def test_census():
    """Every reuse branch was taken on both sides, on every route that has
    the branch.  A tile-split encode builds its own plan and loads tables of
    generation 0 each time (encode_split_core), so it can never report the
    plan or the tables as reused, and what follows it never finds tables: those
    cells are asserted to be empty instead."""
    for a in range(hc.N):   # (a run that selected only this test walks the rows itself)
        if a not in _ROWS_DONE:
            _pair_row(a)
    t = census_table()
    print("\ncontext history census (times set / times clear):")
    for row, cells in t.items():
        print(f"  {row:22s} {cells['encodes']:5d} encodes  " +
              "  ".join(f"{bit}: {cells[bit][0]}/{cells[bit][1]}" for bit in (PLAN, FRONT, T2, STRIPS, TRIM, FAILED)))
    both = lambda c: c[0] > 0 and c[1] > 0  # noqa: E731
    for row in ("pair walks", "route encode_tiff", "route encode_device"):
        for bit in (PLAN, FRONT, T2, STRIPS):
            assert both(t[row][bit]), (row, bit, t[row][bit])
    assert both(t["route split"][STRIPS])
    for bit in (PLAN, FRONT, T2):
        assert t["route split"][bit][0] == 0
    for bit in (PLAN, STRIPS):
        assert both(t["right after a split"][bit]), (bit, t["right after a split"][bit])
    for bit in (FRONT, T2):
        assert t["right after a split"][bit][0] == 0
    # the pairs meant as cache hits, and the step after a split on its key
    # (each asserted where it ran, by Walker; counted here)
    hits = [r for r in CENSUS if r[0] == "a" and r[3] & (PLAN | FRONT | T2) == (PLAN | FRONT | T2)]
    after_split = [r for r in CENSUS if r[0] == "a" and r[2] in ("split1", "split2") and r[3] & PLAN]
    assert len(hits) >= len(hc.cache_hit_pairs())
    assert after_split and all(r[3] & (FRONT | T2) == 0 for r in after_split)
    if any(r[0] == "c" for r in CENSUS):
        assert t["trim walks"][TRIM][0] > 0
    if any(r[0] == "b" for r in CENSUS):
        assert t["after a failure"][FAILED][0] > 0
    out = os.environ.get("JP2HIP_HISTORY_CENSUS")
    if out:
        import json
        with open(out, "w") as fh:
            json.dump({k: {str(b): v for b, v in c.items()} for k, c in t.items()}, fh, indent=1)
