"""The window patterns are what they claim, their references agree with the
C++ oracle and the reference's own test vectors, and each pattern family
tells the right ranges / emit / watermark from a subtly wrong one.  CPU only."""
import numpy as np
import pytest

from dbsp_amd import oracle
from helpers import load_golden, rows_of
from window_patterns import (BASE, BLK, BOUND_NAMES, EMPTY, GRID_CAP,
                             GRID_TOTAL, M64, MAX_TRACE_BATCHES, RUN_LENGTHS,
                             SHAPES, WM_PARAMS, chain_cases, chain_for,
                             emit_cases, grid_case, model_emit_regions,
                             model_wm, ref_chain, ref_window_spine, ref_wm,
                             run_cases, run_lengths, shape_cases, spine_cases,
                             table_diff, wm_sequences, zset_rows)

FAMILIES = {"runs": run_cases, "shapes": shape_cases, "spines": spine_cases,
            "emit": emit_cases, "grid": lambda: [grid_case()]}


def _all_cases():
    return [c for f in FAMILIES.values() for c in f()]


def _ref(case, **kw):
    s0, e0, s1, e1, hp = case["bounds"]
    return ref_window_spine(case["batches"], case["tick"], hp, s0, e0, s1, e1,
                            **kw)


def _nonempty(table):
    return {r for r in range(len(table)) if table[r, 2] > 0}


# ---- the patterns are what they claim ----

def test_run_patterns_put_each_bound_on_each_run():
    cases = run_cases()
    assert len(cases) == 4 * len(RUN_LENGTHS) * 3 * 3
    seen = set()
    for c in cases:
        m = c["meta"]
        bounds = dict(zip(BOUND_NAMES, c["bounds"][:4]))
        assert bounds[m["which"]] == BASE[m["which"]] + m["off"]
        assert all(bounds[n] == BASE[n] for n in BOUND_NAMES
                   if n != m["which"])
        for batch in (c["batches"][0], c["batches"][2], c["tick"]):
            assert run_lengths(batch, m["key"]) == m["length"]
        for batch in (c["batches"][0], c["tick"]):
            k = batch["k"]
            if m["place"] == "start":
                assert k[0] == m["key"] and k[-1] > m["key"]
            elif m["place"] == "end":
                assert k[-1] == m["key"] and k[0] < m["key"]
            else:
                assert k[0] < m["key"] < k[-1]
                assert run_lengths(batch, m["key"] - 1) == 1
                assert run_lengths(batch, m["key"] + 1) == 1
        assert c["bounds"][4] == 1
        seen.add((m["which"], m["length"], m["place"], m["off"]))
    assert len(seen) == len(cases)


def test_shape_patterns():
    s = SHAPES
    assert s["slide"][2] < s["slide"][1]
    assert s["jump"][2] > s["jump"][1]
    assert s["jump-exact"][2] == s["jump-exact"][1]
    assert s["shrink"][3] < s["shrink"][1]
    assert s["unchanged"][:2] == s["unchanged"][2:4]
    assert s["empty-new"][2] == s["empty-new"][3]
    assert s["empty-old"][0] == s["empty-old"][1]
    assert s["first"][4] == 0 and s["start-0"][2] == 0
    assert s["end-max"][3] == M64
    by = {c["meta"]["shape"]: c for c in shape_cases()}
    assert set(by) == set(s)
    # no previous window: the trace regions are empty though the trace is not
    table, rows = _ref(by["first"])
    assert sum(len(b) for b in by["first"]["batches"]) > 0
    assert _nonempty(table) == {len(table) - 1}
    # key 0 is inside a window that starts at 0
    # key 0 is inside a window that starts at 0: the tick's row when the old
    # window held it already, the trace's rows too when it was empty
    table, rows = _ref(by["start-0"])
    assert np.count_nonzero(rows["k"] == 0) == 1
    table, rows = _ref(by["first-saturated"])
    assert np.count_nonzero(rows["k"] == 0) == 4
    # 2^64-2 is inside [s1, 2^64-1), 2^64-1 is not, though both are stored
    table, rows = _ref(by["end-max"])
    stored = np.concatenate(by["end-max"]["batches"] + [by["end-max"]["tick"]])
    assert np.count_nonzero(stored["k"] == np.uint64(M64)) >= 4
    assert np.count_nonzero(rows["k"] == np.uint64(M64)) == 0
    assert np.count_nonzero(rows["k"] == np.uint64(M64 - 1)) >= 4
    # a shrink fills the shrink regions and leaves the insert regions empty
    table, _ = _ref(by["shrink"])
    assert {r % 3 for r in _nonempty(table) if r < len(table) - 1} == {0, 1}
    table, _ = _ref(by["unchanged"])
    assert _nonempty(table) == {len(table) - 1}


def test_spine_patterns():
    by = {c["name"]: c for c in spine_cases()}
    assert {c["meta"]["nb"] for c in by.values()} >= {1, 2, 3, 24}
    for c in by.values():
        assert len(c["batches"]) == c["meta"]["nb"]
    s0, e0, s1, e1, _ = SHAPES["slide"]
    below, inside, above = by["spine-nb3-below-inside-above"]["batches"]
    assert below["k"].max() < s0 and above["k"].min() >= e1
    assert inside["k"].min() >= s1 and inside["k"].max() < e0
    table, _ = _ref(by["spine-nb3-below-inside-above"])
    assert _nonempty(table) == {len(table) - 1}
    assert [len(b) for b in by["spine-one-empty"]["batches"]].count(0) == 1
    assert all(len(b) == 0 for b in by["spine-all-empty"]["batches"])
    assert sum(len(b) == 0 for b in
               by["spine-nb24-some-empty"]["batches"]) == 5
    a, b = by["spine-opposite-weights"]["batches"]
    assert np.array_equal(a["k"], b["k"]) and np.array_equal(a["w"], -b["w"])
    # linear operator: the rows come out per batch, though their sum is the
    # tick region alone
    table, rows = _ref(by["spine-opposite-weights"])
    assert len(_nonempty(table)) == 5
    assert len(zset_rows(rows)) == table[-1, 2]


def test_emit_patterns():
    by = {c["name"]: c for c in emit_cases()}
    nb = MAX_TRACE_BATCHES
    for c in by.values():
        table, rows = _ref(c)
        nbat = len(c["batches"])
        want = {3 * nbat if r == "tick" else 3 * r[0] + r[1]
                for r in c["meta"]["regions"]
                if c["meta"]["lengths"].get(r, 3) > 0}
        assert _nonempty(table) == want, c["name"]
        for r in c["meta"]["regions"]:
            idx = 3 * nbat if r == "tick" else 3 * r[0] + r[1]
            assert table[idx, 2] == c["meta"]["lengths"].get(r, 3), c["name"]
    # tie positions: every offset before the only occupied region is 0, every
    # one after it is the total
    t, _ = _ref(by["emit-only-last-trace-region"])
    assert len(t) == 3 * nb + 1 and np.all(t[:3 * nb, 4] == 0)
    assert t[3 * nb, 4] == 3
    t, _ = _ref(by["emit-only-region-0"])
    assert t[0, 4] == 0 and np.all(t[1:, 4] == 3)
    t, _ = _ref(by["emit-only-tick"])
    assert np.all(t[:, 4] == 0)
    t, _ = _ref(by["emit-len1-retract-insert"])
    assert np.all(t[_nonempty_idx(t), 2] == 1) and len(_nonempty(t)) == 49
    t, _ = _ref(by["emit-len1-retract-shrink"])
    assert np.all(t[_nonempty_idx(t), 2] == 1) and len(_nonempty(t)) == 49
    for total in (1, 255, 256, 257):
        assert len(_ref(by[f"emit-total-{total}"])[1]) == total
    g = grid_case()
    assert len(g["batches"]) == 2
    table, rows = _ref(g)
    assert len(rows) == GRID_TOTAL == GRID_CAP * BLK + 257
    assert len(_nonempty(table)) == 4


def _nonempty_idx(table):
    return np.flatnonzero(table[:, 2] > 0)


def test_chain_patterns():
    by = {c["name"]: c for c in chain_cases()}
    s0, e0, s1, e1, _ = SHAPES["slide"]
    exp = {n: ref_chain(c["batches"], c["tick"], c["chain"])
           for n, c in by.items()}
    for n in ("equal", "shorter", "one", "zero"):
        e = exp[f"chain-len-{n}"]
        # the chained form publishes the host-bounds case's window
        assert e["bounds"] == [s0, e0, s1, e1, 1, 0], n
    c = by["chain-len-shorter"]
    bn, tick = c["chain"]["bn"], c["tick"]
    assert 0 < bn < len(tick)
    assert np.all((tick["k"][bn:] >= s1) & (tick["k"][bn:] < e1))
    assert (exp["chain-len-equal"]["total"] - exp["chain-len-shorter"]["total"]
            == len(tick) - bn)
    assert exp["chain-len-zero"]["table"][-1, 2] == 0
    assert exp["chain-len-zero"]["total"] > 0  # the trace regions remain
    assert exp["chain-len-negative"]["total"] == -1
    # a negative batch length does not stop the watermark
    assert exp["chain-len-negative"]["state"] == exp["chain-len-equal"]["state"]
    e = exp["chain-err-watermark"]
    assert e["total"] == -1 and e["bounds"][5] == 1
    assert e["state"] == list(by["chain-err-watermark"]["chain"]["state"])
    for p in WM_PARAMS:
        c, e = by[f"chain-{p}-advance"], exp[f"chain-{p}-advance"]
        assert e["state"][0] > c["chain"]["state"][0] and e["total"] > 0


def test_watermark_sequences_reach_their_edges():
    for name, (width, tumble, lag), ticks in wm_sequences():
        if not name.endswith("-walk"):
            assert ticks[0] is not None
            continue
        assert ticks[0] is None and None in ticks[1:] and M64 in ticks
        assert lag == 0 or lag in ticks
        state, seen = (0, 0, 0, 0), set()
        for g in ticks:
            before = state
            state, bounds = ref_wm(state, g, width, tumble, lag)
            wm, s1, e1, _ = state
            assert wm >= before[0] and s1 >= before[1], "monotone"
            assert bounds[:2] == list(before[1:3]) and bounds[4] == before[3]
            if not g:
                assert wm == before[0] and state[3] == 1
                seen.add("empty")
            elif g - lag < before[0]:
                assert wm == before[0]
                seen.add("late")
            for d in (-1, 0, 1):
                if wm > 1 and (wm - d) % tumble == 0:
                    seen.add(f"multiple{d:+d}")
            seen.add("below" if e1 < width else
                     "equal" if e1 == width else "above")
            if e1 < width:
                assert s1 == 0
        want = {"empty", "late", "multiple+0", "multiple+1", "below", "equal",
                "above"} | ({"multiple-1"} if tumble > 2 else set())
        assert want <= seen, (name, want - seen)


# ---- the references agree with the oracle and the reference's vectors ----

@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_ref_window_is_the_oracle_window_of_the_merged_spine(family):
    for c in FAMILIES[family]():
        s0, e0, s1, e1, hp = c["bounds"]
        trace = EMPTY
        for b in c["batches"]:
            trace = oracle.merge(trace, b)
        exp = oracle.window(trace, c["tick"], hp, s0, e0, s1, e1)
        table, rows = _ref(c)
        assert table[-1, 4] + table[-1, 2] == len(rows)
        assert np.array_equal(zset_rows(rows), zset_rows(exp)), c["name"]


def test_ref_chain_is_the_oracle_window_too():
    for c in chain_cases():
        e = ref_chain(c["batches"], c["tick"], c["chain"])
        if e["total"] < 0:
            continue
        s0, e0, s1, e1, hp, _ = e["bounds"]
        trace = EMPTY
        for b in c["batches"]:
            trace = oracle.merge(trace, b)
        bn = c["chain"].get("bn", len(c["tick"]))
        exp = oracle.window(trace, c["tick"][:bn], hp, s0, e0, s1, e1)
        assert np.array_equal(zset_rows(e["rows"]), zset_rows(exp)), c["name"]


def test_refs_replay_the_reference_window_vectors():
    """tests/golden/window_ops.json tick by tick, the trace kept as a spine
    of the earlier ticks' batches.  Bounds a watermark can give (the end does
    not move back) come from ref_wm with tumble 1, lag 0 and the window's own
    width; the vectors' shrinking windows are set directly."""
    g = load_golden("window_ops.json")
    stepped = 0
    for case in g["cases"]:
        spine, state = [], (0, 0, 0, 0)
        for tick, (b, inp, exp) in enumerate(
                zip(case["bounds"], case["inputs"], case["expected"])):
            s1, e1 = b
            batch = oracle.consolidate(rows_of([tuple(r) for r in inp]))
            if e1 >= state[0] and e1 > 0 and s1 <= e1:
                state, bounds = ref_wm(state, e1, e1 - s1, 1, 0)
                stepped += 1
            else:
                bounds = [state[1], state[2], s1, e1, state[3], 0]
                state = (state[0], s1, e1, 1)
            assert bounds[2:4] == [s1, e1], (case["name"], tick)
            s0, e0, _, _, hp, _ = bounds
            assert len(spine) <= MAX_TRACE_BATCHES
            _, rows = ref_window_spine(spine, batch, hp, s0, e0, s1, e1)
            want = zset_rows(rows_of([tuple(r) for r in exp]))
            assert np.array_equal(zset_rows(rows), want), (case["name"], tick)
            spine.append(batch)
    assert stepped >= 6


# ---- wrong variants ----

def _differs(case, **kw):
    t0, r0 = _ref(case)
    t1, r1 = _ref(case, **kw)
    return table_diff(t1, t0) is not None or not np.array_equal(r0, r1)


@pytest.mark.parametrize("which", BOUND_NAMES)
def test_run_patterns_expose_an_upper_bound_at_each_bound(which):
    """A ranges kernel that seeks one bound with upper_bound differs from
    the reference on the patterns that put that bound on a run, at every run
    length, and on none that put it beside the run's key."""
    hit = set()
    for c in run_cases():
        m = c["meta"]
        if m["which"] != which:
            continue
        if m["off"] == 0:
            assert _differs(c, upper=(which,)), c["name"]
            hit.add((m["length"], m["place"]))
    assert len(hit) == len(RUN_LENGTHS) * 3
    for c in run_cases() + shape_cases():
        assert not _differs(c, upper=()), c["name"]


def test_emit_patterns_expose_a_strict_region_search():
    """`<` for `<=` in the emit's search sends the first row of every region
    to the region before it (or off the table)."""
    exposed = 0
    for c in emit_cases() + spine_cases():
        table, rows = _ref(c)
        total = len(rows)
        owner = np.repeat(np.arange(len(table)), table[:, 2])
        assert np.array_equal(model_emit_regions(table, total), owner)
        if total:
            wrong = model_emit_regions(table, total, strict=True)
            assert not np.array_equal(wrong, owner), c["name"]
            exposed += 1
    assert exposed >= len(emit_cases())


@pytest.mark.parametrize("variant", ["round_first", "no_saturate"])
def test_watermark_sequences_expose_wrong_watermarks(variant):
    exposed = []
    for name, (width, tumble, lag), ticks in wm_sequences():
        good = bad = (0, 0, 0, 0)
        differ = False
        for g in ticks:
            good, gb = ref_wm(good, g, width, tumble, lag)
            bad, bb = model_wm(bad, g, width, tumble, lag, variant)
            differ |= (good, gb) != (bad, bb)
        if differ:
            exposed.append(name)
    assert any(n.endswith("-walk") for n in exposed), exposed


def test_model_wm_without_a_variant_is_the_reference():
    for name, (width, tumble, lag), ticks in wm_sequences():
        a = b = (0, 0, 0, 0)
        for g in ticks:
            a, ab = ref_wm(a, g, width, tumble, lag)
            b, bb = model_wm(b, g, width, tumble, lag, None)
            assert (a, ab) == (b, bb), name


def test_chain_for_publishes_the_case_bounds():
    for c in shape_cases() + spine_cases():
        ch = chain_for(c)
        e = ref_chain(c["batches"], c["tick"], ch)
        assert tuple(e["bounds"][:5]) == c["bounds"], c["name"]
        table, rows = _ref(c)
        assert table_diff(e["table"], table) is None
        assert np.array_equal(e["rows"], rows)
