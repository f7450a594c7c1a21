"""The top-K model (tests/topk_model.py) against the reference's own q19 test
cases (tests/golden/q19_top_bids.json) and against an O(n^2) brute-force
restatement on random streams with retractions.  CPU only."""
import random

import pytest

import topk_model as tm
from helpers import load_golden

GOLD = load_golden("q19_top_bids.json")


def _golden_delta(tick):
    return [tm.q19_pack(b["auction"], b["bidder"], b["price"],
                        GOLD["defaults"]["date_time"]) + (1,) for b in tick]


def _golden_zset(rows):
    return {tm.q19_pack(r["auction"], r["bidder"], r["price"],
                        r["date_time"]): r["weight"] for r in rows}


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_golden_cases(case):
    integral = {}
    inc = tm.Model(GOLD["k"], tm.Q19_SHIFT)
    for tick, expected in zip(case["ticks"], case["expected"]):
        delta = _golden_delta(tick)
        integral, out, _, _ = tm.step(integral, delta, GOLD["k"],
                                      tm.Q19_SHIFT)
        assert out == _golden_zset(expected)
        assert inc.step(delta)[0] == out


def test_pack_roundtrip_and_order():
    a = tm.q19_pack(5, 7, 300, 11)
    assert tm.q19_unpack(*a) == (5, 7, 300, 11)
    # (auction, price, bidder, date_time) order is (k, v) order
    rows = [(1, 9, 100, 5), (1, 2, 101, 0), (1, 2, 100, 7), (2, 0, 0, 0),
            (1, 9, 100, 4)]
    packed = sorted(tm.q19_pack(*r) for r in rows)
    assert [tm.q19_unpack(*p) for p in packed] == sorted(
        rows, key=lambda r: (r[0], r[2], r[1], r[3]))


def test_presence_rules():
    K, s = 2, 4
    I, out, _, _ = tm.step({}, [(0x10, 1, 1), (0x11, 0, 1), (0x12, 0, 1)], K, s)
    assert out == {(0x11, 0): 1, (0x12, 0): 1}
    I, out, _, _ = tm.step(I, [(0x12, 0, 1)], K, s)        # 1 -> 2: nothing
    assert out == {}
    I, out, _, _ = tm.step(I, [(0x12, 0, -2)], K, s)       # net 0: vanishes
    assert out == {(0x12, 0): -1, (0x10, 1): 1}
    I, out, _, _ = tm.step(I, [(0x13, 5, -1)], K, s)       # net -1: present
    assert out == {(0x13, 5): 1, (0x10, 1): -1}
    I, out, _, _ = tm.step(I, [(0x13, 5, 1)], K, s)        # -1 then +1
    assert out == {(0x13, 5): -1, (0x10, 1): 1}


def test_verdict_rule():
    K, s = 2, 8
    I = tm.apply_delta({}, [(0x100 | i, 0, 1) for i in range(4)] +
                       [(0x200, 0, 1)])
    # a member of a full top-K vanishes: refill
    assert tm.refills(I, [(0x103, 0, -1)], K, s) == (1, 1)
    # a row below the threshold of a full group vanishes: no refill
    assert tm.refills(I, [(0x100, 0, -1)], K, s) == (0, 1)
    # a member of a short group vanishes: no refill
    assert tm.refills(I, [(0x200, 0, -1)], K, s) == (0, 1)
    # a weight change that keeps presence is no vanish
    assert tm.refills(I, [(0x103, 0, 1)], K, s) == (0, 1)
    # the first member itself counts (r >= first)
    assert tm.refills(I, [(0x102, 0, -1), (0x200, 0, -1)], K, s) == (1, 2)


def _random_delta(rng, live, shift, n):
    delta = []
    for _ in range(n):
        if live and rng.random() < 0.4:
            k, v = rng.choice(live)
            delta.append((k, v, rng.choice([-1, -1, 1, -2])))
        else:
            g = rng.randrange(2 if shift == 63 else 5)
            k = (g << shift) | rng.randrange(1 << min(shift, 3))
            v = rng.randrange(3)
            delta.append((k, v, rng.choice([1, 1, 2, -1])))
            live.append((k, v))
    return delta


@pytest.mark.parametrize("K,shift", [(1, 0), (3, 4), (10, 27), (2, 63)])
def test_model_against_brute_force(K, shift):
    rng = random.Random(1000 * K + shift)
    integral, live, acc = {}, [], {}
    inc = tm.Model(K, shift)
    for _ in range(40):
        delta = _random_delta(rng, live, shift, rng.randrange(1, 25))
        integral, out, n_refill, n_groups = tm.step(integral, delta, K, shift)
        acc = tm.zset_add(acc, out)
        assert acc == tm.brute_output(integral, K, shift)
        assert all(w in (1, -1) for w in out.values())
        assert inc.step(delta) == (out, n_refill, n_groups)
        assert inc.integral == integral and inc.acc == acc


def test_random_stream_seed_makes_both_verdicts_occur():
    """The stream tests/test_gpu_topk.py asserts groups_refilled on: at least
    20 refilled and 20 non-refilled group-ticks."""
    m = tm.Model(10, 20)
    refilled = kept = 0
    for delta in tm.random_stream(tm.RANDOM_SEED):
        _, n_refill, n_groups = m.step(delta)
        refilled += n_refill
        kept += n_groups - n_refill
    assert refilled >= 20 and kept >= 20, (refilled, kept)
    assert m.acc == tm.full_output(m.integral, 10, 20)
