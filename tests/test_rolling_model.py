"""The numpy rolling-aggregate model (tests/rolling_model.py) against an
O(n^2) brute force, the CPU oracle's batch rolling aggregate, and the
reference's own test vectors (tests/golden/rolling_over_range.json)."""
import numpy as np
import pytest

from dbsp_amd import oracle
from helpers import load_golden, rows_of
from rolling_model import (apply_delta, brute_output, expected_delta,
                           full_output, zset_diff)

RANGES = [(1000, 0), (500, 500), (0, 0), (3, 7), (1 << 33, 0), (0, 1 << 63)]


def _random_delta(rng, n, parts, tmax):
    return [(int(rng.integers(0, parts)), int(rng.integers(0, tmax)),
             int(rng.integers(-2, 4))) for _ in range(n)]


@pytest.mark.parametrize("before,after", RANGES)
def test_model_matches_brute_force(before, after):
    rng = np.random.default_rng(before % 1000 + after % 1000 + 1)
    for tmax in (30, 1000, 10 ** 6, 1 << 32):
        integral = {}
        for _ in range(6):
            delta = _random_delta(rng, int(rng.integers(0, 25)), 4, tmax)
            nxt = apply_delta(integral, delta)
            assert full_output(nxt, before, after) == \
                brute_output(nxt, before, after)
            assert expected_delta(integral, delta, before, after) == \
                zset_diff(brute_output(nxt, before, after),
                          brute_output(integral, before, after))
            integral = nxt
        assert all(w != 0 for w in integral.values())


def test_model_saturates_at_both_ends():
    tmax = (1 << 32) - 1
    integral = {(7, 0): 2, (7, tmax): 3, (8, 0): 5}
    assert full_output(integral, tmax, tmax) == {
        ((7 << 32) | 0, 5): 1, ((7 << 32) | tmax, 5): 1, ((8 << 32), 5): 1}
    assert full_output(integral, 0, 0) == {
        ((7 << 32) | 0, 2): 1, ((7 << 32) | tmax, 3): 1, ((8 << 32), 5): 1}


def test_non_positive_rows_count_but_do_not_emit():
    integral = {(1, 10): -4, (1, 12): 3}
    # (1, 10) has weight <= 0: no output row, but it is inside 12's range
    assert full_output(integral, 5, 0) == {((1 << 32) | 12, (-1) & (2 ** 64 - 1)): 1}


@pytest.mark.parametrize("width", [0, 1, 10, 1000, 1 << 40])
def test_model_matches_oracle_rolling_agg(width):
    """after = 0: the model's sums equal the batch primitive's on the rows
    of positive weight (the rows the operator emits)."""
    rng = np.random.default_rng(width % 97)
    integral = apply_delta({}, _random_delta(rng, 400, 5, 2000))
    rows = rows_of(sorted((p, ts, w) for (p, ts), w in integral.items()))
    got = oracle.rolling_agg(rows, width)
    assert len(got) == len(rows)
    exp = {}
    for r, src in zip(got, rows):
        assert (r["k"], r["v"]) == (src["k"], src["v"])
        if src["w"] > 0:
            exp[((int(r["k"]) << 32) | int(r["v"]),
                 int(r["w"]) & (2 ** 64 - 1))] = 1
    assert full_output(integral, width, 0) == exp


def test_model_reproduces_golden():
    g = load_golden("rolling_over_range.json")
    assert "rolling_aggregate.rs:811-862" in g["source"]
    for case in g["cases"]:
        for rng_key, rows in case["expected"].items():
            before, after = (int(x) for x in rng_key.split(","))
            integral, acc = {}, {}
            for step in case["steps"]:
                d = expected_delta(integral, step, before, after)
                acc = zset_diff(acc, {k: -w for k, w in d.items()})
                integral = apply_delta(integral, step)
            exp = {((p << 32) | ts, s): 1 for p, ts, s in rows}
            assert acc == exp, (case["name"], rng_key)
            assert full_output(integral, before, after) == exp
