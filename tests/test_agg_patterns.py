"""The aggregate patterns are what they claim, their references agree with
the C++ oracle where it has the operation, and the last-10 patterns tell the
right fold from subtly wrong ones.  CPU only."""
import numpy as np
import pytest

from agg_patterns import (AUCTION_MAX, EMPTY, LAST_N, M64, MAX_TRACE_BATCHES,
                          MODES, PRICE_BITS, PRICE_MAX, SIZES, consolidated,
                          distinct_cases, key_cases, key_run, last10_cases,
                          linear_cases, max_cases, new_value, ref_distinct,
                          ref_sum_spine, ref_upsert, size_case, sorted_rows,
                          sum_cases)
from dbsp_amd import oracle
from helpers import np_consolidate


def _upsert_cases(sizes=SIZES):
    return (last10_cases() + max_cases() + linear_cases() + key_cases()
            + [size_case(n) for n in sizes])


def _by(cases):
    return {c["name"]: c for c in cases}


def _val(mode, case, key, variant=None):
    return new_value(mode, key_run(case["in_rows"], key), variant)


# ---- the patterns are what they claim ----

def test_last10_patterns():
    by = _by(last10_cases())
    c = by["last10-run-lengths"]
    assert sorted(c["meta"]["lengths"].values()) == [1, 9, 10, 11, 12, 100]
    for key, n in c["meta"]["lengths"].items():
        run = key_run(c["in_rows"], key)
        assert len(run) == n
        prices = [int(v) % (1 << PRICE_BITS) for v in run["v"]]
        assert _val("last10", c, key) == sum(prices[-LAST_N:]) // min(n, LAST_N)
    c = by["last10-price-edges"]
    assert _val("last10", c, 1) == 0
    assert _val("last10", c, 2) == PRICE_MAX
    run = key_run(c["in_rows"], 3)
    assert len(run) == 12 and np.all(run["v"] // np.uint64(1 << PRICE_BITS)
                                     == np.uint64(AUCTION_MAX))
    assert run["v"][-1] == np.uint64(M64)
    # the last ten prices are PRICE_MAX-9 .. PRICE_MAX: 4.5 below, floored
    assert _val("last10", c, 3) == PRICE_MAX - 5
    assert _val("last10", c, 4) == 1 and (1 + 2) % 2 == 1
    assert _val("last10", c, 5) == (1 << 20) + 5
    c = by["last10-negative-weights"]
    w = key_run(c["in_rows"], 7)["w"]
    assert (w < 0).any() and (w > 0).any() and w[-1] > 0 and len(w) > LAST_N
    for key in c["meta"]["negative_keys"]:
        assert np.all(key_run(c["in_rows"], key)["w"] < 0)
        assert _val("last10", c, key) is not None  # fold.rs:87: still emits
    assert _val("last10", c, 9) == 40


def test_max_and_linear_patterns():
    c = max_cases()[0]
    for key, n in c["meta"]["lengths"].items():
        run = key_run(c["in_rows"], key)
        assert len(run) == n
        assert _val("max", c, key) == int(run["v"][-1]) == int(run["v"].max())
    assert key_run(c["in_rows"], c["meta"]["negative_last"])["w"][-1] < 0
    assert _val("max", c, 13) == M64
    c = linear_cases()[0]
    assert _val("linear", c, 20) is None
    got = ref_upsert("linear", [20], c["in_rows"], c["out_rows"])
    assert got.tolist() == [(20, 6, -1)]  # the retraction alone
    assert _val("linear", c, 21) == M64 - 6  # -7 as its bits
    assert len(key_run(c["in_rows"], 22)) == 1000
    assert _val("linear", c, 23) == (1 << 64) - (1 << 62)


def test_key_patterns():
    by = _by(key_cases())
    full = by["keys-all"]
    ik, ok = full["in_rows"]["k"], full["out_rows"]["k"]
    assert ik[0] == 0 and ik[-1] == np.uint64(M64) and ok[0] == 0
    c = by["keys-same-val"]
    for mode in MODES:
        assert _val(mode, c, 20) == 7
        raw = ref_upsert(mode, c["keys"], c["in_rows"], c["out_rows"])
        assert raw.tolist() == [(20, 7, 1), (20, 7, -1)], mode
        assert len(np_consolidate(raw)) == 0
    assert len(key_run(full["in_rows"], 10)) and not len(
        key_run(full["out_rows"], 10))
    assert len(key_run(full["out_rows"], 30)) == 3 and not len(
        key_run(full["in_rows"], 30))
    assert (key_run(full["out_rows"], 30)["w"] < 0).any()
    c = by["keys-absent"]
    k = c["in_rows"]["k"]
    a = c["meta"]["absent"]
    assert a[0] < k[0] and k[0] < a[1] < k[-1] and a[2] > k[-1]
    for mode in MODES:
        assert len(ref_upsert(mode, c["keys"], c["in_rows"],
                              c["out_rows"])) == 0
        assert len(ref_upsert(mode, by["keys-none"]["keys"], full["in_rows"],
                              full["out_rows"])) == 0
    assert len(by["keys-empty-in"]["in_rows"]) == 0
    assert len(by["keys-empty-out"]["out_rows"]) == 0


def test_size_patterns():
    assert SIZES == (1, 255, 256, 257, 2048, 2049, 65537)
    for nd in SIZES:
        c = size_case(nd)
        assert len(c["keys"]) == nd
        assert consolidated(c["in_rows"]) and consolidated(c["out_rows"])
        if nd >= 255:
            # keys with and without rows on either side, and trace keys that
            # no delta key names
            for t in (c["in_rows"], c["out_rows"]):
                present = np.isin(c["keys"], t["k"])
                assert present.any() and not present.all()
                assert not np.isin(t["k"], c["keys"]).all()


def test_sum_patterns():
    by = {c[0]: c for c in sum_cases()}
    for nb in (1, 2, MAX_TRACE_BATCHES):
        _, delta, batches, meta = by[f"sum-nb{nb}"]
        assert len(batches) == nb == meta["nb"]
        assert consolidated(delta) and all(consolidated(b) for b in batches)
        if nb > 1:
            assert any(len(b) == 0 for b in batches)
        keys, rows = ref_sum_spine(delta, batches)
        assert 0 < len(rows) < len(keys)
    _, delta, batches, meta = by["sum-cancel-across-batches"]
    keys, rows = ref_sum_spine(delta, batches)
    for key in meta["zero_keys"]:
        assert key not in rows["k"]
        assert any(len(key_run(b, key)) for b in batches)
    for key in (4, 5):  # no single batch cancels them
        assert all(int(key_run(b, key)["w"].sum()) != 0 for b in batches
                   if len(key_run(b, key)))
    assert rows["k"].tolist() == [6, 7, M64]
    for name, delta, batches, meta in sum_cases():
        if not name.startswith("uniq-"):
            continue
        keys, _ = ref_sum_spine(delta, batches)
        assert len(keys) == meta["nkeys"], name
        if "heads" in meta:
            k = delta["k"]
            heads = [0] + (np.flatnonzero(k[1:] != k[:-1]) + 1).tolist()
            assert tuple(heads) == meta["heads"]
    k = by["uniq-run-across-256"][1]["k"]
    assert k[250] == k[260] and k[249] < k[250] and k[261] > k[260]


def test_distinct_patterns():
    by = {c[0]: c for c in distinct_cases()}
    _, delta, (t,), _ = by["distinct-val-absent"]
    for k, v in zip(delta["k"], delta["v"]):
        run = key_run(t, k)
        assert len(run) and v not in run["v"]
    _, delta, (t,), _ = by["distinct-val-above-run-next-key-equal"]
    assert delta["v"][0] > key_run(t, 5)["v"].max()
    assert key_run(t, 6)["v"][0] == delta["v"][0]
    _, delta, (t,), _ = by["distinct-run-ends-batch"]
    assert t["k"][-1] == 8 and delta["v"][1] > t["v"][-1]
    _, delta, batches, _ = by["distinct-cross-zero-over-batches"]
    got = ref_distinct(delta, batches)
    assert got.tolist() == [(1, 1, 1), (2, 1, -1), (3, 1, -1), (4, 1, 1),
                            (4, 2, 1)]
    # no single batch gives those verdicts
    assert any(ref_distinct(delta, [b]).tolist() != got.tolist()
               for b in batches)
    assert len(by["distinct-nb24"][2]) == MAX_TRACE_BATCHES
    exp = ref_distinct(*by["distinct-nb24"][1:3])
    assert (exp["w"] > 0).any() and (exp["w"] < 0).any()


# ---- the references agree with the oracle ----

@pytest.mark.parametrize("mode", ["linear", "max"])
def test_ref_upsert_agrees_with_the_oracle(mode):
    fn = {"linear": oracle.agg_linear_upsert, "max": oracle.agg_max_upsert}
    for c in _upsert_cases():
        raw = ref_upsert(mode, c["keys"], c["in_rows"], c["out_rows"])
        exp = fn[mode](c["keys"], c["in_rows"], c["out_rows"],
                       cap=len(raw) + 16)
        # the oracle consolidates each key's updates (upsert.rs:198)
        assert np.array_equal(np_consolidate(raw), np_consolidate(exp)), (
            c["name"])


def test_ref_sum_and_distinct_agree_with_the_oracle():
    for name, delta, batches, _ in sum_cases():
        keys, rows = ref_sum_spine(delta, batches)
        trace = EMPTY
        for b in batches:
            trace = oracle.merge(trace, b)
        exp = oracle.agg_linear_upsert(keys, trace, EMPTY)
        assert np.array_equal(sorted_rows(rows), sorted_rows(exp)), name
    for name, delta, batches, _ in distinct_cases():
        trace = EMPTY
        for b in batches:
            trace = oracle.merge(trace, b)
        exp = oracle.distinct_inc(delta, trace)
        assert np.array_equal(ref_distinct(delta, batches), exp), name


# ---- wrong variants ----

@pytest.mark.parametrize("variant", ["first", "positive", "mask20"])
def test_last10_patterns_expose_a_wrong_fold(variant):
    exposed = []
    for c in last10_cases():
        good = ref_upsert("last10", c["keys"], c["in_rows"], c["out_rows"])
        bad = ref_upsert("last10", c["keys"], c["in_rows"], c["out_rows"],
                         variant)
        if len(good) != len(bad) or not np.array_equal(good, bad):
            exposed.append(c["name"])
    want = {"first": "last10-run-lengths", "positive": "last10-negative-weights",
            "mask20": "last10-price-edges"}[variant]
    assert want in exposed, exposed


def test_the_right_fold_differs_on_none():
    for c in _upsert_cases(sizes=(257,)):
        for mode in MODES:
            a = ref_upsert(mode, c["keys"], c["in_rows"], c["out_rows"])
            b = ref_upsert(mode, c["keys"], c["in_rows"], c["out_rows"], None)
            assert np.array_equal(a, b)
