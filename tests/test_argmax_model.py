"""The arg-max model (tests/argmax_model.py) against an O(n^2) brute-force
restatement on random streams with retractions, and its Python q7 against
the reference's own q7 test cases (tests/golden/q7_highest_bid.json).  CPU
only."""
import random

import pytest

import argmax_model as am
from helpers import load_golden

GOLD = load_golden("q7_highest_bid.json")

CASE_NAMES = ["latest_bid_determines_window", "window_boundary_below",
              "window_boundary_lower", "window_boundary_upper",
              "window_boundary_above", "tumble_into_new_window",
              "multiple_max_bids"]


def golden_bids(tick):
    d = GOLD["defaults"]
    return [(d["auction"], d["bidder"], b["price"], b["date_time"], 1)
            for b in tick]


def golden_zset(rows):
    return {am.q7_pack(r["auction"], r["bidder"], r["price"],
                       r["date_time"]): r["weight"] for r in rows}


def test_golden_file_holds_the_seven_cases():
    assert [c["name"] for c in GOLD["cases"]] == CASE_NAMES
    assert GOLD["defaults"] == {"auction": 1, "bidder": 1}
    assert GOLD["watermark_lag_ms"] == am.Q7_WATERMARK_LAG_MS
    assert GOLD["tumble_ms"] == am.Q7_TUMBLE_MS


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_golden_cases(case):
    q = am.Q7()
    assert len(case["ticks"]) == len(case["expected"])
    for tick, expected in zip(case["ticks"], case["expected"]):
        assert q.step(golden_bids(tick)) == golden_zset(expected)


def test_q7_pack_roundtrip_and_order():
    a = am.q7_pack(5, 7, 300, 11)
    assert am.q7_unpack(*a) == (5, 7, 300, 11)
    assert a[0] >> am.Q7_GROUP_SHIFT == 0 and a[0] >> am.Q7_RANK_SHIFT == 300
    # the widest fields stay inside one group
    k, _ = am.q7_pack((1 << 32) - 1, (1 << 32) - 1, (1 << 27) - 1,
                      (1 << 32) - 1)
    assert k >> am.Q7_GROUP_SHIFT == 0


def test_q7_retraction_inside_the_window():
    q = am.Q7()
    out = q.step([(1, 1, 50, 11_000, 1), (2, 2, 90, 12_000, 1),
                  (3, 3, 10, 32_000, 1)])
    assert out == {am.q7_pack(2, 2, 90, 12_000): 1}
    out = q.step([(2, 2, 90, 12_000, -1)])
    assert out == {am.q7_pack(2, 2, 90, 12_000): -1,
                   am.q7_pack(1, 1, 50, 11_000): 1}
    assert q.refills == 1 and q.tumbles == 0


def test_relation_and_weights():
    gs, rs = 8, 4
    I, out, r, _ = am.step({}, [(0x110, 0, 1), (0x125, 1, 3), (0x12F, 0, -1),
                                (0x210, 0, 1)], gs, rs)
    # group 1: rank 0x12 holds two rows, each at its own weight
    assert out == {(0x125, 1): 3, (0x12F, 0): -1, (0x210, 0): 1} and r == 0
    I, out, r, _ = am.step(I, [(0x125, 1, -1)], gs, rs)     # 3 -> 2
    assert out == {(0x125, 1): -1} and r == 0
    I, out, r, _ = am.step(I, [(0x130, 0, 1)], gs, rs)      # the maximum rises
    assert out == {(0x130, 0): 1, (0x125, 1): -2, (0x12F, 0): 1} and r == 0


def test_divergence_mixed_sign_ties_keep_their_rank():
    """Two different rows at the top rank with weights +1 and -1: the
    reference's Min sums them to zero and skips the price
    (aggregate/min.rs:38-57); here both rows are present and stay the tie
    set."""
    gs, rs = 8, 4
    I, out, r, _ = am.step({}, [(0x100, 0, 1), (0x120, 0, 1), (0x121, 0, -1)],
                           gs, rs)
    assert out == {(0x120, 0): 1, (0x121, 0): -1}
    assert am.brute_output(I, gs, rs) == out
    m = am.Model(gs, rs)
    assert m.step([(0x100, 0, 1), (0x120, 0, 1), (0x121, 0, -1)])[0] == out


def test_refill_rule():
    gs, rs = 8, 4
    I = am.apply_delta({}, [(0x100, 0, 1), (0x120, 0, 1), (0x121, 5, 1),
                            (0x200, 0, 1)])
    # a tie vanishes while another stays: no refill
    assert am.refills(I, [(0x120, 0, -1)], gs, rs) == (0, 1)
    # all ties vanish: refill
    assert am.refills(I, [(0x120, 0, -1), (0x121, 5, -1)], gs, rs) == (1, 1)
    # ... unless a row of at least that rank appears in the same tick
    assert am.refills(I, [(0x120, 0, -1), (0x121, 5, -1), (0x12F, 9, 1)],
                      gs, rs) == (0, 1)
    assert am.refills(I, [(0x120, 0, -1), (0x121, 5, -1), (0x1F0, 0, 1)],
                      gs, rs) == (0, 1)
    # a lower row appearing does not help
    assert am.refills(I, [(0x120, 0, -1), (0x121, 5, -1), (0x110, 0, 1)],
                      gs, rs) == (1, 1)
    # the group empties: refill; a new group: none
    assert am.refills(I, [(0x200, 0, -1), (0x300, 0, 1)], gs, rs) == (1, 2)
    # a weight change that keeps presence, and a row below the maximum
    assert am.refills(I, [(0x120, 0, 1), (0x100, 0, -1)], gs, rs) == (0, 1)


def _random_delta(rng, live, gs, rs, n):
    delta = []
    for _ in range(n):
        if live and rng.random() < 0.45:
            k, v = rng.choice(live)
            delta.append((k, v, rng.choice([-1, -1, 1, -2])))
        else:
            g = rng.randrange(2 if gs == 63 else 4)
            low = rng.randrange(1 << min(gs, 4))
            k = (g << gs) | low
            v = rng.randrange(3)
            delta.append((k, v, rng.choice([1, 1, 2, -1])))
            live.append((k, v))
    return delta


@pytest.mark.parametrize("gs,rs", [(0, 0), (4, 4), (4, 2), (27, 0), (63, 0),
                                   (63, 2)])
def test_model_against_brute_force(gs, rs):
    rng = random.Random(1000 * gs + rs)
    integral, live, acc = {}, [], {}
    inc = am.Model(gs, rs)
    for _ in range(40):
        delta = _random_delta(rng, live, gs, rs, rng.randrange(1, 25))
        integral, out, n_refill, n_groups = am.step(integral, delta, gs, rs)
        acc = am.zset_add(acc, out)
        assert acc == am.brute_output(integral, gs, rs)
        assert acc == am.full_output(integral, gs, rs)
        assert inc.step(delta) == (out, n_refill, n_groups)
        assert inc.integral == integral and inc.acc == acc


def test_random_stream_seed_makes_both_verdicts_occur():
    """The stream tests/test_gpu_argmax.py asserts groups_refilled on: at
    least 20 refilled group-ticks and at least 20 touched groups that already
    had a maximum and kept it."""
    gs, rs = am.RANDOM_SHIFTS
    m = am.Model(gs, rs)
    refilled = kept = 0
    for delta in am.random_stream(am.RANDOM_SEED):
        had = {g for g, rows in m.groups.items() if rows}
        touched = {k >> gs for k, _ in am.apply_delta({}, delta)}
        _, n_refill, n_groups = m.step(delta)
        assert n_groups == len(touched)
        refilled += n_refill
        kept += len(touched & had) - n_refill
    assert refilled >= 20 and kept >= 20, (refilled, kept)
    assert m.acc == am.full_output(m.integral, gs, rs)
