"""The numpy model of the rolling Max / Min (tests/rolling_minmax_model.py)
against its O(n^2) restatement and the hand-derived cases of
tests/golden/rolling_minmax.json.  No GPU."""
import numpy as np
import pytest

from helpers import load_golden
from rolling_minmax_model import (AGGS, apply_delta, brute_output,
                                  expected_delta, full_output, rows_minmax,
                                  zset_diff)

TMAX = (1 << 32) - 1
RANGES = [(1000, 0), (5, 5), (0, 0), (3, 7), (1 << 33, 0)]


def golden_cases():
    return load_golden("rolling_minmax.json")["cases"]


def golden_expected(rows):
    return {((p << 32) | ts, m): w for p, ts, m, w in rows}


def random_integral(rng, n):
    """5 partitions, times below 200, values below 50, weights in -2..3: rows
    cancel, several values share a time, some times hold negative rows only."""
    integral = {}
    for _ in range(n):
        row = (int(rng.integers(0, 5)), int(rng.integers(0, 200)),
               int(rng.integers(0, 50)), int(rng.integers(-2, 4)))
        integral = apply_delta(integral, [row])
    return integral


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("before,after", RANGES)
def test_model_equals_brute_force(before, after, agg):
    rng = np.random.default_rng(before % 1013 + 7 * after + len(agg))
    negative_only = 0
    for n in (0, 1, 30, 400, 1200):
        integral = random_integral(rng, n)
        assert full_output(integral, before, after, agg) == \
            brute_output(integral, before, after, agg)
        times = {}
        for (p, ts, _), w in integral.items():
            times.setdefault((p, ts), []).append(w)
        negative_only += sum(all(w < 0 for w in ws) for ws in times.values())
    assert negative_only > 0, "no time of negative rows only was drawn"


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_golden_cases(case):
    integral, acc = {}, {}
    for step, exp in zip(case["steps"], case["expected"]):
        delta = [tuple(r) for r in step]
        got = expected_delta(integral, delta, case["before"], case["after"],
                             case["agg"])
        assert got == golden_expected(exp)
        integral = apply_delta(integral, delta)
        acc = zset_diff(acc, {k: -w for k, w in got.items()})
    for f in (full_output, brute_output):
        assert acc == f(integral, case["before"], case["after"], case["agg"])


@pytest.mark.parametrize("agg,far,near", [("max", 90, 40), ("min", 2, 40)])
def test_negative_only_time_moves_its_neighbours(agg, far, near):
    """A time whose rows are all negative never emits, yet its value counts
    in the extreme of every time whose range holds it."""
    integral = apply_delta({}, [(2, 100, 20, 1), (2, 103, 30, 2)])
    calm = full_output(integral, 5, 5, agg)
    pick = max if agg == "max" else min
    assert calm == {((2 << 32) | 100, pick(20, 30)): 1,
                    ((2 << 32) | 103, pick(20, 30)): 1}
    for w in (-1, -3):
        moved = apply_delta(integral, [(2, 101, far, w), (2, 101, near, w)])
        out = full_output(moved, 5, 5, agg)
        assert out == {((2 << 32) | 100, far): 1, ((2 << 32) | 103, far): 1}
        assert out == brute_output(moved, 5, 5, agg)
    # one positive row among the negative ones and the time emits, once
    mixed = apply_delta(integral, [(2, 101, far, -1), (2, 101, near, 1)])
    out = full_output(mixed, 5, 5, agg)
    assert out == {((2 << 32) | t, far): 1 for t in (100, 101, 103)}


@pytest.mark.parametrize("agg", AGGS)
def test_values_at_both_ends(agg):
    """0 and 2^32-1 are the tree's identities and also legal values."""
    rows = [(7, 1, 0, 1), (7, 2, TMAX, 1), (7, 2, 0, 1), (7, 9, TMAX, 1),
            (7, 20, 0, 1), (7, TMAX, TMAX, 1), (7, 0, 0, 1)]
    integral = apply_delta({}, rows)
    out = full_output(integral, 1, 0, agg)
    assert out == brute_output(integral, 1, 0, agg)
    m = {k & TMAX: v for (k, v) in out}
    if agg == "max":
        assert m == {0: 0, 1: 0, 2: TMAX, 9: TMAX, 20: 0, TMAX: TMAX}
    else:
        assert m == {0: 0, 1: 0, 2: 0, 9: TMAX, 20: 0, TMAX: TMAX}
    # retracting the extreme uncovers the other end
    d = expected_delta(integral, [(7, 2, TMAX if agg == "max" else 0, -1)],
                       1, 0, agg)
    other = 0 if agg == "max" else TMAX
    if agg == "max":
        assert d == {((7 << 32) | 2, TMAX): -1, ((7 << 32) | 2, other): 1}
    else:
        # time 1 (value 0) is still inside time 2's range [1, 2]
        assert d == {}
        d = expected_delta(integral, [(7, 2, 0, -1), (7, 1, 0, -1)], 1, 0, agg)
        assert d == {((7 << 32) | 1, 0): -1, ((7 << 32) | 2, 0): -1,
                     ((7 << 32) | 2, TMAX): 1}


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("before,after", [(10, 3), (0, 0), (1 << 32, 1 << 32)])
def test_rows_minmax_equals_brute_force(before, after, agg):
    """The batch primitive's model: with every weight positive each time
    emits, so brute_output holds the value of every row's time."""
    rng = np.random.default_rng(after + len(agg))
    integral = {k: abs(w) for k, w in random_integral(rng, 600).items()}
    rows = sorted(integral)
    got = rows_minmax([r[0] for r in rows], [r[1] for r in rows],
                      [r[2] for r in rows], before, after, agg)
    brute = {k: m for (k, m) in brute_output(integral, before, after, agg)}
    assert [int(x) for x in got] == [brute[(p << 32) | ts] for p, ts, _ in rows]
