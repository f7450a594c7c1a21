"""The join pattern grid of tests/join_patterns.py, checked without a GPU:
every pattern has the property its name claims, the numpy reference agrees
with the C++ oracle where the two are independent (projections 0..8), the
q4 / q6 window edges come out as the plain fields say, and the run and
hot-key patterns tell the right gallop and owner search from each classic
wrong variant."""
import numpy as np
import pytest

from dbsp_amd import ROW_DT, oracle
from helpers import np_consolidate
from join_patterns import (FUSE_MAX, FUSE_THREADS, GALLOP_WRONG, HOT1, HOT2,
                           HOT_RUNS, K_ALL, K_ALT, K_FIRST, K_LAST, K_OPP,
                           M64, MAX_TRACE_BATCHES, NB_GRID, OWNER_WRONG,
                           PROBE_BLOCK, PROBE_STRIDE, RUN_LENGTHS, SCAN_BLOCK,
                           SIZES_BIG, SIZES_SMALL, TAIL_CAP, TAIL_TOTALS,
                           _rows, batch_cases, gallop_model, hot_cases,
                           match_ranges, merged_trace, owner_model, plan_view,
                           proj_cases, ref_join, ref_tail, run_cases,
                           size_cases, sorted_kv, spine_cases, tail_cases)

ROW_LIMIT = 1 << 16  # rows of a trace and of an output


def _well_formed(delta, batches):
    assert delta.dtype == ROW_DT and sorted_kv(delta)
    assert 1 <= len(batches) <= MAX_TRACE_BATCHES
    for t in batches:
        assert t.dtype == ROW_DT and sorted_kv(t)
    assert sum(len(t) for t in batches) < ROW_LIMIT
    w = np.concatenate([delta["w"]] + [t["w"] for t in batches])
    assert np.all(w != 0) and np.abs(w).max() <= 5
    assert (w > 0).any() and (w < 0).any()


def _oracle_agrees(delta, batches, proj, param, what):
    ref = ref_join(delta, batches, proj, param)
    assert len(ref) < ROW_LIMIT, what
    exp = oracle.join_raw(delta, merged_trace(batches), proj, param,
                          cap=len(ref) + 16)
    assert len(exp) == len(ref), what
    assert np.array_equal(np_consolidate(ref), np_consolidate(exp)), what
    return ref


def test_sizes_name_the_kernels_blocks():
    assert PROBE_BLOCK == 256 and PROBE_STRIDE == 2048 and SCAN_BLOCK == 2048
    assert FUSE_MAX == 8 * FUSE_THREADS == 8192
    for edge in (PROBE_BLOCK, PROBE_STRIDE, FUSE_MAX):
        assert {edge - 1, edge, edge + 1} <= set(SIZES_SMALL + SIZES_BIG)
    assert {SCAN_BLOCK - 1, SCAN_BLOCK + 1, 20000} <= set(SIZES_BIG)
    assert max(SIZES_SMALL) == FUSE_MAX < min(
        n for n in SIZES_BIG if n > SCAN_BLOCK + 1)
    for n in SIZES_SMALL + SIZES_BIG:  # a neighbour that is no multiple of 8
        assert n % 8 or (n - 1 in SIZES_SMALL + SIZES_BIG)


def test_run_patterns_are_what_they_claim():
    cases = run_cases()
    seen = set()
    for name, delta, batches, m in cases:
        _well_formed(delta, batches)
        (t,) = batches
        tk = t["k"].astype(object)
        key, n, at = m["key"], m["length"], m["run_at"]
        seen.add((n, m["place"], key))
        assert len(t) == m["nt"]
        assert [int(x) for x in np.flatnonzero(t["k"] == np.uint64(key))] == \
            list(range(at, at + n)), name
        if m["place"] in ("start", "whole"):
            assert at == 0, name
        else:
            assert tk[at - 1] == key - 1, name
        if m["place"] in ("end", "whole"):
            assert at + n == len(t), name
        else:
            assert tk[at + n] == key + 1, name
        if m["place"] == "whole":
            assert len(t) == n
        dk = [int(x) for x in delta["k"]]
        assert dk.count(key) == 2
        for nbr in (key - 1, key + 1):
            if 0 <= nbr <= M64:
                assert nbr in dk, name
        lo_k, hi_k = int(tk[0]), int(tk[-1])
        if lo_k > 2:
            assert dk[0] < lo_k, name            # below every trace key
        if hi_k < M64 - 2:
            assert dk[-1] > hi_k, name           # above every trace key
        if m["place"] == "middle":               # in a gap between two keys
            assert key - 6 in dk and key - 6 not in tk
        cnt = match_ranges(delta, batches)[1][:, 0]
        for i, k in enumerate(dk):
            assert cnt[i] == int(np.count_nonzero(t["k"] == np.uint64(k)))
    for n in RUN_LENGTHS:
        for combo in (("start", 0), ("whole", 0), ("end", M64), ("whole", M64)):
            assert (n,) + combo in seen
        assert sum(1 for s in seen if s[0] == n) == 8


def test_batch_patterns_are_what_they_claim():
    cases = batch_cases()
    assert [m["nb"] for _, _, _, m in cases if m["empty_at"] is None] == \
        list(NB_GRID)
    empties = {(m["nb"], m["empty_at"]) for _, _, _, m in cases} - \
        {(nb, None) for nb in NB_GRID}
    assert empties == {(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (24, 0),
                       (24, 12), (24, 23)}
    for name, delta, batches, m in cases:
        _well_formed(delta, batches)
        nb, at = m["nb"], m["empty_at"]
        assert len(batches) == nb
        assert [b for b in range(nb) if len(batches[b]) == 0] == (
            [] if at is None else [at])

        def holders(key):
            return [b for b in range(nb) if np.any(batches[b]["k"] == key)]
        live = [b for b in range(nb) if b != at]
        assert holders(K_FIRST) == [b for b in live if b == 0]
        assert holders(K_LAST) == [b for b in live if b == nb - 1]
        assert holders(K_ALT) == [b for b in live if b % 2 == 0]
        assert holders(K_ALL) == live
        if nb >= 2:
            assert holders(K_OPP) == [b for b in live if b in (0, nb - 1)]
            if at not in (0, nb - 1):
                a = batches[0][batches[0]["k"] == K_OPP]
                z = batches[-1][batches[-1]["k"] == K_OPP]
                assert len(a) == len(z) == 1 and a["v"] == z["v"]
                assert a["w"] == -z["w"]
                raw = ref_join(delta, batches, 8)
                mine = raw[raw["k"] == K_OPP]
                assert len(mine) == 2 and mine["w"].sum() == 0
        for key in (K_FIRST, K_LAST, K_ALT, K_ALL):
            assert np.any(delta["k"] == key)


def test_hot_patterns_are_what_they_claim():
    shapes = set()
    for name, delta, batches, m in hot_cases():
        _well_formed(delta, batches)
        assert len(batches) == 3
        cnt = match_ranges(delta, batches)[1]
        h, z = m["hot_row"], m["zeros"]
        shapes.add(m["shape"])
        assert int(delta["k"][h]) == HOT1
        assert tuple(cnt[h]) == HOT_RUNS and sum(HOT_RUNS) == 5017
        tot = cnt.sum(axis=1)
        before = m["shape"] in ("before", "both", "last")
        after = m["shape"] in ("after", "both", "between")
        if before:
            assert np.all(tot[h - z:h] == 0) and tot[h - z - 1] > 0, name
        if after:
            assert np.all(tot[h + 1:h + 1 + z] == 0) and tot[h + 1 + z] > 0
        if m["shape"] == "between":
            assert int(delta["k"][h + 1 + z]) == HOT2
            assert sorted(cnt[h + 1 + z]) == sorted(HOT_RUNS)
        if m["shape"] == "last":
            assert h == len(delta) - 1
        else:
            assert tot[-1] > 0
    assert shapes == {"before", "after", "between", "both", "last"}


def test_size_patterns_are_what_they_claim():
    cases = size_cases()
    assert [m["nd"] for _, _, _, m in cases] == list(SIZES_SMALL + SIZES_BIG)
    for name, delta, batches, m in cases:
        if m["nd"] > 1:
            _well_formed(delta, batches)
        assert len(delta) == m["nd"]
        tot = match_ranges(delta, batches)[1].sum(axis=1)
        assert tot[0] == 3 and tot[-1] == 3, name  # both ends own slots
        assert tot.sum() < ROW_LIMIT
        if m["nd"] > 8:
            assert np.any(tot == 0) and np.any(tot == 1) and np.any(tot == 2)


def test_ref_join_agrees_with_the_oracle_on_every_spine_pattern():
    for name, delta, batches, _ in spine_cases():
        for proj in (0, 8):
            raw = _oracle_agrees(delta, batches, proj, 0, (name, proj))
            # delta row major, then batch, then trace position: v2 names the
            # batch and the place, v1 the delta row
            if proj == 0 and "batches" not in name:
                order = np.lexsort((raw["k"] & np.uint64((1 << 40) - 1),
                                    raw["k"] >> np.uint64(40), raw["v"]))
                assert np.array_equal(order, np.arange(len(raw))), name


def test_projection_patterns():
    cases = proj_cases()
    assert sorted(m["proj"] for _, _, _, m in cases) == sorted(
        list(range(13)) + [3, 4])
    assert {(m["proj"], m["param"]) for _, _, _, m in cases
            if m["proj"] in (3, 4)} == {(p, q) for p in (3, 4)
                                        for q in (1, 10000)}
    for name, delta, batches, m in cases:
        _well_formed(delta, batches)
        proj, param = m["proj"], m["param"]
        vals = np.concatenate([delta["v"]] + [t["v"] for t in batches])
        ks = np.concatenate([delta["k"]] + [t["k"] for t in batches])
        assert ks.min() == 0 and ks.max() == M64
        raw = ref_join(delta, batches, proj, param)
        assert 0 < len(raw) < ROW_LIMIT
        if proj <= 8:
            assert (vals >> np.uint64(48)).max() > 0     # 64-bit-wide vals
            assert (vals & np.uint64(0xFFFFFFFF)).max() > 1 << 24
            _oracle_agrees(delta, batches, proj, param, name)
            if param:
                low = vals & np.uint64(0xFFFFFFFF)
                assert np.any(low % np.uint64(param) == 0)
                assert param == 1 or np.any(low % np.uint64(param) != 0)
            continue
        # 9..12: weight-0 slots stay in the sequence
        assert np.any(raw["w"] == 0) and np.any(raw["w"] != 0)
        bits = m["tag_bits"]
        edges = {True: 0, False: 0}
        for key, av, bv, tag, price, valid in m["pairs"]:
            d, t = _rows([key], [bv], [1]), _rows([key], [av], [-2])
            if proj in (10, 12):
                d, t = t, d
            (row,) = ref_join(d, [t], proj, param)
            assert int(row["k"]) == (key * (1 << bits) + tag) % (1 << 64)
            assert int(row["v"]) == price
            assert int(row["w"]) == (-2 if valid else 0), (name, key, av, bv)
            edges[valid] += 1
        assert edges[True] >= 40 and edges[False] >= 40
        fields = {(av >> (bits + (24 if bits == 4 else 16)),
                   (av >> bits) % (1 << (24 if bits == 4 else 16)),
                   av % (1 << bits)) for _, av, _, _, _, _ in m["pairs"]}
        dur_max = (1 << (24 if bits == 4 else 16)) - 1
        dt_max = (1 << (36 if bits == 4 else 28)) - 1
        for f, top in enumerate((dt_max, dur_max, (1 << bits) - 1)):
            assert {0, top} <= {x[f] for x in fields}, (name, f)
        bid_v = delta["v"] if proj in (9, 11) else np.concatenate(
            [t["v"] for t in batches])
        prices = {int(x) % (1 << 27) for x in bid_v}
        assert {0, (1 << 27) - 1} <= prices


def test_tail_patterns_are_what_they_claim():
    cases = tail_cases()
    by_name = {name: (plans, cap, m) for name, plans, cap, m in cases}
    assert len(by_name) == len(cases)
    for name, plans, cap, m in cases:
        assert 1 <= len(plans) <= 3 and cap == TAIL_CAP
        for pl in plans:
            view = plan_view(pl)
            assert sorted_kv(pl["delta"]) and len(pl["delta"]) <= FUSE_MAX
            assert all(sorted_kv(t) for t in pl["batches"])
            assert sum(len(t) for t in pl["batches"]) < ROW_LIMIT
            assert pl["proj"] in (0, 1)  # the tail passes param 0
            if view is not None and len(pl["delta"]):
                w = np.concatenate([pl["delta"]["w"]]
                                   + [t["w"] for t in pl["batches"]])
                assert (w > 0).any() and np.abs(w).max() <= 5
        r = ref_tail(plans, cap)
        healthy = [t for t in r["totals"] if t >= 0]
        if "total" in m:
            assert sum(r["totals"]) == m["total"], name
            assert r["d_flag"] == (1 if m["total"] > cap else 0)
            assert r["d_total"] == (m["total"] if m["total"] <= cap else -1)
            assert (r["d_final"] >= 0) == (m["total"] <= FUSE_MAX)
            assert (r["capbuf"] is not None) == (FUSE_MAX < m["total"] <= cap)
        if "stride" in m:
            assert [len(pl["delta"]) for pl in plans] == [8192, 8192,
                                                          m["last"]]
            rows = np.concatenate([match_ranges(*plan_view(pl))[1].sum(axis=1)
                                   for pl in plans])
            for cell in (0, 8191, 8192, 16383, 16384, len(rows) - 1):
                assert rows[cell] > 0, (name, cell)
            assert np.count_nonzero(rows) < len(rows) // 4      # sparse
            assert (rows.sum() <= FUSE_THREADS) == (m["stride"] == 97)
            assert rows.sum() <= FUSE_MAX
        if "empty" in m:
            assert [t == 0 for t in r["totals"]] == [
                p == m["empty"] for p in range(3)]
            assert len(plans[m["empty"]]["delta"]) == 0
        if "left" in m:
            assert r["totals"] == [m["n"], m["n"] - m["left"]]
            assert r["d_final"] == m["left"] == len(r["store"])
        if "kind" in m:
            at, kind = m["at"], m["kind"]
            if kind in ("tn=0", "tn=30"):
                # a short or empty tick-fresh trace is healthy: the plan
                # matches that many trace rows and no more
                assert len(plans[at]["batches"][0]) > 30
                assert r["totals"][at] == int(kind[3:]) and r["d_flag"] == 0
                assert r["d_total"] == sum(r["totals"]) > 0
            else:
                assert r["totals"][at] == -1 and r["offsets"][at] is None
                assert (r["d_flag"], r["d_total"], r["d_final"]) == (1, -1, -1)
                assert r["store"] is None and r["capbuf"] is None
            others = [p for p in range(3) if p != at]
            assert all(r["totals"][p] == len(plans[p]["delta"]) > 0
                       for p in others)
            assert all(np.array_equal(r["offsets"][p],
                                      np.arange(len(plans[p]["delta"])))
                       for p in others)
        if "nb=24" in name:
            assert sorted(len(pl["batches"]) for pl in plans) == [1, 24]
        assert len(healthy) == sum(o is not None for o in r["offsets"])
    totals = [m["total"] for _, _, _, m in cases if "total" in m]
    assert totals == list(TAIL_TOTALS) == [0, 1, 1023, 1024, 1025, 8191, 8192,
                                           8193, 32768, 32769]
    kinds = {(m["kind"], m["at"]) for _, _, _, m in cases if "kind" in m}
    assert kinds == {("nd=-1", 0), ("nd=-1", 1), ("nd=-1", 2), ("nd=8193", 0),
                     ("nd=8193", 1), ("nd=8193", 2), ("tn=-1", 2), ("tn=0", 2),
                     ("tn=30", 2)}
    sized = {m["nd"]: plans for _, plans, _, m in cases if "nd" in m}
    assert sorted(sized) == list(SIZES_SMALL)
    assert all(len(sized[nd][0]["delta"]) == nd for nd in sized)
    assert {m["empty"] for _, _, _, m in cases if "empty" in m} == {0, 1, 2}
    assert {(m["stride"], m["last"]) for _, _, _, m in cases
            if "stride" in m} == {(97, 100), (5, 100), (97, 8192)}
    assert {(m["n"], m["left"]) for _, _, _, m in cases if "left" in m} == {
        (400, 0), (400, 1), (1500, 0), (1500, 1)}


def test_ref_tail_store_is_the_consolidated_concatenation():
    name, plans, cap, _ = next(c for c in tail_cases() if "stride=5" in c[0])
    r = ref_tail(plans, cap)
    cat = np.concatenate([ref_join(*plan_view(pl), pl["proj"]) for pl in plans])
    assert np.array_equal(r["store"], np_consolidate(cat))
    assert r["d_total"] == len(cat) > FUSE_THREADS
    base = 0
    for pl, off, tot in zip(plans, r["offsets"], r["totals"]):
        # a row's offset is where its first output sits in its plan's rows
        per_row = match_ranges(*plan_view(pl))[1].sum(axis=1)
        first = np.flatnonzero(per_row)
        got = cat[base + off[first].astype(np.int64)]
        assert np.array_equal(got["v"] if pl["proj"] == 0 else got["k"],
                              pl["delta"]["v"][first])
        base += tot


def test_patterns_tell_the_right_gallop_from_each_wrong_one():
    """The right model equals the searchsorted counts everywhere; every wrong
    variant miscounts (or reads outside the batch) on some run pattern, and
    each run length catches at least one of them."""
    caught = {v: set() for v in GALLOP_WRONG}
    for name, delta, batches, m in run_cases():
        (t,) = batches
        tk = t["k"]
        lo, cnt = match_ranges(delta, batches)
        for i in range(len(delta)):
            key, at = int(delta["k"][i]), int(lo[i, 0])
            assert gallop_model(tk, key, at) == cnt[i, 0], name
            for v in GALLOP_WRONG:
                try:
                    wrong = gallop_model(tk, key, at, v)
                except IndexError:
                    wrong = "out of range"
                if wrong != cnt[i, 0]:
                    caught[v].add((m["length"], m["place"])
                                  if key == m["key"] else (0, "neighbour"))
    for v in GALLOP_WRONG:
        assert caught[v], v
    # `<` for `<=` and the short window undercount a run of 1 already
    assert {n for n, _ in caught["lt_final"]} - {0} == set(RUN_LENGTHS)
    assert 1 in {n for n, _ in caught["rem_minus_one"]}
    # the loop bounds show only where the run touches the end of its batch
    for v in ("loop_le_nt", "loop_stops_early"):
        assert {p for _, p in caught[v]} - {"neighbour"} == {"end", "whole"}
    assert {2, 4, 8, 16} <= {n for n, _ in caught["loop_stops_early"]}
    # one past a doubling point: key + 1 directly behind the run is counted
    # by no variant that passes the run itself
    hot = hot_cases()[0]
    lo, cnt = match_ranges(hot[1], hot[2])
    h = hot[3]["hot_row"]
    for b in range(3):
        assert gallop_model(hot[2][b]["k"], HOT1, int(lo[h, b])) == HOT_RUNS[b]


def test_patterns_tell_the_right_owner_search_from_each_wrong_one():
    """upper_bound(offsets, o) - 1 lands on the row that owns slot o; `<` for
    `<=`, the first of the equal offsets and a range one row short each land
    elsewhere on the hot-key patterns."""
    caught = {v: set() for v in OWNER_WRONG}
    for name, delta, batches, m in hot_cases() + run_cases()[:8]:
        per_row = match_ranges(delta, batches)[1].sum(axis=1)
        offsets = np.cumsum(per_row) - per_row
        owners = np.flatnonzero(per_row)
        for i in owners:
            for o in {int(offsets[i]), int(offsets[i] + per_row[i] - 1)}:
                assert owner_model(offsets, o) == i, name
                for v in OWNER_WRONG:
                    if owner_model(offsets, o, v) != i:
                        caught[v].add(m.get("shape", "run"))
    hot_shapes = {"before", "after", "between", "both", "last"}
    assert caught["lt"] >= hot_shapes
    # the zero-match run directly before a hot row shares its offset
    assert caught["first_equal"] >= {"before", "both", "last"}
    for name, delta, batches, m in hot_cases():
        if m["shape"] in ("before", "both", "last"):
            per_row = match_ranges(delta, batches)[1].sum(axis=1)
            offsets = np.cumsum(per_row) - per_row
            h = m["hot_row"]
            assert owner_model(offsets, int(offsets[h]), "first_equal") == \
                h - m["zeros"]
    # only a last row that owns slots shows the short range
    assert "last" in caught["short"]
