"""Explicit per-layer rates on the CPU: every refusal of
jp2hip_check_layer_rates by message, one step of the loop through the
host-only entry jp2hip_layer_rate_step (the text the device and the tile-split
run), the Python restatement of the rule (tests/layer_rate_cases.py) against
that entry on random sizes, the targets and first budgets of every case, and
the iteration counts the one-layer cases of the GPU suite reach on the oracle.
"""
import random

import pytest

import jp2hip
import layer_rate_cases as lr

LL, LY = jp2hip.LOSSLESS, jp2hip.LOSSY
NAN, INF = float("nan"), float("inf")
step = jp2hip._lib.layer_rate_step


# ---- refusals ------------------------------------------------------------------------

@pytest.mark.parametrize("rates,recipe,match", [
    ([0.5, NAN, 2.0], None, r"rates\[1\].*NaN"),
    ([NAN], None, r"rates\[0\].*NaN"),
    ([0.5, INF], None, r"rates\[1\].*infinite"),
    ([0.5, 1.0, -1.0], None, r"rates\[2\].*negative"),
    ([-0.0, 1.0], None, r"rates\[0\].*negative"),
    ([0.5, 2.0, 1.0, 3.0], None, r"rates\[2\] decreases from rates\[1\]"),
    ([1.0, 0.0, 2.0], None, r"rates\[1\] decreases from rates\[0\]"),   # a 0 that is not the last
    ([0.5, 1.0, 0.0], dict(conv=LL, layers=6), r"n = 3.*layers = 6"),
    ([0.5] * 7, dict(conv=LY, layers=6), r"n = 7.*layers = 6"),
    ([0.5, 1.0, 2.0], dict(conv=LL, layers=3), r"rates\[2\], the last, must be 0"),
    ([0.5, 1.0, 2.0], dict(conv=LY, layers=3, rate_bpp=0.0), r"rates\[2\], the last, must be 0"),
    ([0.5, 1.0, 0.0], dict(conv=LY, layers=3), r"rates\[2\] is 0 with rate_bpp > 0"),
    ([0.0, 0.0, 1.0], dict(conv=LY, layers=3), r"rates\[0\] is 0 with rate_bpp > 0"),
    ([1.0] * 33, None, r"n = 33"),
])
def test_check_refuses_by_name(rates, recipe, match):
    rc = None if recipe is None else jp2hip.recipe(recipe.pop("conv"), **recipe)
    with pytest.raises(jp2hip.Jp2hipError, match=match):
        jp2hip.check_layer_rates(rates, rc)


@pytest.mark.parametrize("rates,recipe", [
    ([], None), (None, None), ([0.5, 0.5, 1.0, 1.0], None), ([0.0], None), ([1.0, 2.0, 0.0], None),
    ([0.5, 1.0, 0.0], dict(conv=LL, layers=3)), ([0.5, 1.0, 2.0], dict(conv=LY, layers=3)),
    ([0.0], dict(conv=LL, layers=1)), ([0.0, 0.0], dict(conv=LL, layers=2)),
    ([], dict(conv=LL, layers=3)), ([0.25] * 32, dict(conv=LY, layers=32)),
])
def test_check_accepts(rates, recipe):
    jp2hip.check_layer_rates(rates, None if recipe is None else jp2hip.recipe(recipe.pop("conv"), **recipe))


def test_the_setters_need_a_context():
    """Without a GPU no context exists; the setters refuse a null one by name
    after the checks passed, and the checks come first."""
    L = jp2hip._lib.lib()
    arr, n = jp2hip._lib.slopes_array([0.5, 1.0])
    assert L.jp2hip_set_layer_rates(None, arr, n) != 0 and "null context" in jp2hip._lib.last_error()
    arr, n = jp2hip._lib.slopes_array([1.0, 0.5])
    assert L.jp2hip_set_layer_rates(None, arr, n) != 0 and "rates[1] decreases" in jp2hip._lib.last_error()
    assert L.jp2hip_batch_set_layer_rates(None, arr, n) != 0


# ---- one step ------------------------------------------------------------------------
# sizes as the entry takes them: fixed, part_bytes and packet bytes per layer;
# S[l] = fixed + part - sum(layer_bytes[l + 1:])

def test_step_halts_when_every_layer_fits():
    lb = [100, 200, 300]
    S = lr.through_layers(50, 650, lb)
    assert S == [200, 400, 700]
    halt, b = step(0, 50, 650, lb, [200, 400, 700], [90, 190, 290])
    assert halt and b == [90, 190, 290]
    halt, b = step(0, 50, 650, lb, [200, 399, 700], [90, 190, 290])
    assert not halt


def test_step_halts_at_the_eighth_iteration_with_the_budgets_untouched():
    for it in range(7):
        assert not step(it, 0, 1000, [1000], [10], [500])[0]
    halt, b = step(7, 0, 1000, [1000], [10], [500])
    assert halt and b == [500]


def test_step_lowers_only_the_layers_that_are_over():
    lb = [1000, 1000, 1000]
    # S = [1100, 2100, 3100]; layer 1 is over by 100, the others fit
    halt, b = step(2, 100, 3000, lb, [1100, 2000, 3100], [900, 1900, 2900])
    assert not halt
    assert b == [900, 1900 - ((100 << 2) + (100 >> 4) + 64), 2900]
    # layer 0 alone
    halt, b = step(0, 100, 3000, lb, [1000, 2100, 3100], [900, 1900, 2900])
    assert b == [900 - (100 + 6 + 64), 1900, 2900]


def test_step_floors_at_zero():
    halt, b = step(3, 0, 5000, [5000], [100], [300])
    assert not halt and b == [0]
    halt, b = step(0, 0, 5000, [2000, 3000], [100, 100], [0, 300])
    assert b == [0, 0]


def test_step_clamps_a_lower_budget_that_passes_an_upper_one():
    """Equal rates: layer 2 is over and falls below layer 1's budget, which
    fits; the clamp brings layers 1 and 0 down with it."""
    lb = [500, 500, 500]
    # S = [600, 1100, 1600], targets [1000, 1200, 1200]: only layer 2 is over, by 400
    halt, b = step(1, 100, 1500, lb, [1000, 1200, 1200], [800, 1000, 1000])
    down = 1000 - ((400 << 1) + (400 >> 4) + 64)
    assert not halt and b == [min(800, down), down, down] and down < 800


def test_step_leaves_a_lossless_top_layer_alone():
    lb = [500, 500, 10 ** 6]
    t = [400, 2000, lr.NO_TARGET]
    halt, b = step(0, 100, sum(lb), lb, t, [300, 900, lr.NO_BUDGET])
    assert not halt and b[2] == lr.NO_BUDGET and b[1] == 900 and b[0] < 300
    # it fits below: halt, whatever the top layer's size is
    halt, b = step(0, 100, sum(lb), lb, [600, 2000, lr.NO_TARGET], [300, 900, lr.NO_BUDGET])
    assert halt and b == [300, 900, lr.NO_BUDGET]


def existing_step(it, budget, target, cs_bytes):
    """rate_step of device_common.h, the single rate's: (halt, budget)."""
    if cs_bytes <= target or it == 7:
        return True, budget
    over = cs_bytes - target
    return False, max(0, budget - ((over << it) + (over >> 4) + 64))


@pytest.mark.parametrize("it", range(8))
def test_one_layer_is_the_existing_step(it):
    rnd = random.Random(20261021 + it)
    table = [(0, 0, 0), (1000, 900, 1001), (1000, 900, 1000), (10 ** 9, 10 ** 9, 2 * 10 ** 9), (50, 0, 10 ** 7)]
    table += [(rnd.randrange(0, 10 ** 7), rnd.randrange(0, 10 ** 7), rnd.randrange(0, 10 ** 7)) for _ in range(200)]
    for target, budget, cs in table:
        fixed = min(cs, 117)
        got = step(it, fixed, cs - fixed, [cs - fixed], [target], [budget])
        want = existing_step(it, budget, target, cs)
        assert (got[0], got[1][0]) == want, (it, target, budget, cs)


def test_step_refuses_bad_arguments():
    with pytest.raises(jp2hip.Jp2hipError):
        step(8, 0, 0, [0], [0], [0])
    with pytest.raises(jp2hip.Jp2hipError):
        step(0, 0, 0, [0] * 33, [0] * 33, [0] * 33)


# ---- the model against the entry ---------------------------------------------------------

@pytest.mark.parametrize("seed", range(40))
def test_model_agrees_with_the_entry_on_random_sizes(seed):
    """run_model over a synthetic encoder -- a layer's bytes are its budget's
    share of a random size plus random header bytes, so layers overshoot and
    undershoot in turn -- against a loop over jp2hip_layer_rate_step fed the
    same sizes: the same budgets at every selection, the same halt."""
    rnd = random.Random(seed)
    L = rnd.choice([1, 2, 3, 6, 12, 32])
    lossless_top = seed % 3 == 0
    t = sorted(rnd.randrange(0, 200000) for _ in range(L))
    if seed % 5 == 0 and L > 2:
        t[1] = t[2]   # equal targets
    if lossless_top:
        t[-1] = lr.NO_TARGET
    b0 = [lr.NO_BUDGET if x == lr.NO_TARGET else max(0, x - rnd.randrange(0, 5000) * (l + 1))
          for l, x in enumerate(t)]
    fixed = rnd.randrange(50, 400)
    noise = [[rnd.randrange(0, 6000) for _ in range(L)] for _ in range(8)]
    sizes = []   # (part_bytes, layer_bytes) of every sizing pass, for the entry's loop

    def size(budgets):
        it = len(sizes)
        cum = [min(b, 150000) + noise[it][l] * (3 if it < 3 else 0) // 3 for l, b in enumerate(budgets)]
        cum = [max(cum[:l + 1]) for l in range(L)]
        lb = [cum[0]] + [cum[l] - cum[l - 1] for l in range(1, L)]
        hdr = rnd.randrange(0, 3000)
        sizes.append((hdr + sum(lb), lb))
        return lr.through_layers(fixed, hdr + sum(lb), lb)

    m = lr.run_model(t, b0, select=lambda b: list(b), size=size)
    b = lr.clamp(b0)
    for it, (part, lb) in enumerate(sizes):
        assert m["trace"][it]["budgets"] == b, (seed, it)
        halt, b = step(it, fixed, part, lb, t, b)
        assert halt == (it == len(sizes) - 1), (seed, it)
    assert m["iterations"] == len(sizes) <= 8
    if lossless_top:
        assert all(x["budgets"][-1] == lr.NO_BUDGET for x in m["trace"])


# ---- the cases ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(lr.ALL))
def test_case_rates_pass_the_check_and_match_the_rule(name):
    conv, rc = lr.recipe(name)
    jp2hip.check_layer_rates(lr.rates(name), rc)
    for letters, tlm in ((0, 0), ("LC", 1)):
        t, b, info = lr.plan_numbers(name, letters, tlm)
        assert (info["T"] > 0) == bool(tlm) and (info["E"] > 0) == bool(letters)
        assert b == lr.clamp(b) and all(x >= 0 for x in b)
        assert (t[-1] == lr.NO_TARGET and b[-1] == lr.NO_BUDGET) == (conv == LL)


def test_targets_with_one_layer_are_the_single_rate_s():
    """L = 1: the target and first budget of rate_target_of / first_budget_of
    (what pcrd_cases.first_budget_rate inverts)."""
    for c in lr.one_layer_cases():
        rc = jp2hip.recipe(LY, **c["recipe"])
        t, b, info = jp2hip._lib.layer_rate_targets(256, 256, 1, c["bits"], rc, [rc.rate_bpp])
        assert t == [int(rc.rate_bpp * 256 * 256 / 8)]
        assert b == [max(0, t[0] - 16 * info["npackets"] - 16 * info["ntileparts"] - 256)]
        assert info["T"] == info["E"] == 0


def test_one_layer_cases_reach_every_door_of_the_loop():
    """The GPU suite's one-layer cases: between them 1 iteration, one of
    2 .. 7, and 8 (counted by the oracle), on both tier-2 routes."""
    cases = lr.one_layer_cases()
    assert {c["route"] for c in cases} == set(lr.pc.ROUTES)
    assert any("tie" in c["name"] for c in cases) and any("_ly1" in c["name"] for c in cases)
    counts = {c["name"]: lr.oracle_iterations(c) for c in cases}
    print(counts)
    got = set(counts.values())
    assert 1 in got and 8 in got and got & set(range(2, 8)), counts
