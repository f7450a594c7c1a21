"""The antijoin model (tests/antijoin_model.py) against hand-derived cases
and against the reference's composition A - A |><| distinct(B)
(join.rs:298-319) computed with the pinned oracle primitives."""
import numpy as np
import pytest

import antijoin_model as am
from dbsp_amd import ROW_DT, gen, oracle
from helpers import load_golden, rows_of, zset

GOLD = load_golden("antijoin.json")
PROJ_HI_K_LO_V2 = 8  # DBSP_PROJ_HI_K_LO_V2


def _zs(triples):
    return {(k, v): w for k, v, w in triples}


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_golden_cases(case):
    model = am.Model(case["mode"])
    totals = [0, 0, 0]
    for tick, expected in zip(case["ticks"], case["expected"]):
        delta, nf, ng, nd = model.step([tuple(r) for r in tick["a"]],
                                       [tuple(r) for r in tick["b"]])
        assert delta == _zs(expected)
        totals = [totals[0] + nf, totals[1] + ng, totals[2] + nd]
    assert totals == case["counters"]
    assert model.acc == am.full_output(model.integral_a, model.integral_b,
                                       case["mode"])


def _neg(rows):
    out = rows.copy()
    out["w"] = -out["w"]
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_delta_equals_the_reference_composition(seed):
    anti, semi = am.Model(am.ANTIJOIN), am.Model(am.SEMIJOIN)
    A = np.empty(0, dtype=ROW_DT)       # integral of A
    BK = np.empty(0, dtype=ROW_DT)      # integral of the key rows (k, 0, w)
    D = np.empty(0, dtype=ROW_DT)       # integral of distinct(B)
    for i, (dA, dB) in enumerate(am.random_stream(seed)):
        got_anti = anti.step(dA, dB)[0]
        got_semi = semi.step(dA, dB)[0]
        da = oracle.consolidate(rows_of(dA))
        db = oracle.consolidate(rows_of([(k, 0, w) for k, w in dB]))
        # distinct(B) incrementally (distinct.rs:273), then the two-sided
        # join A |><| distinct(B): dD against A, and distinct-B' against dA
        dD = oracle.distinct_inc(db, BK)
        D_after = oracle.consolidate(np.concatenate([D, dD]))
        j1 = oracle.join_raw(dD, A, PROJ_HI_K_LO_V2)
        j2 = oracle.join_raw(D_after, da, PROJ_HI_K_LO_V2)
        join = oracle.consolidate(np.concatenate([j1, j2]))
        minus = oracle.consolidate(np.concatenate([da, _neg(join)]))
        assert zset(join) == got_semi, f"tick {i}"
        assert zset(minus) == got_anti, f"tick {i}"
        # semijoin = A - antijoin, tick by tick
        assert am.zset_add(got_anti, got_semi) == zset(da), f"tick {i}"
        A = oracle.consolidate(np.concatenate([A, da]))
        BK = oracle.consolidate(np.concatenate([BK, db]))
        D = D_after
    for m in (anti, semi):
        assert m.acc == am.full_output(m.integral_a, m.integral_b, m.mode)
        assert zset(A) == m.integral_a
    assert set(zset(D)) == {(k, 0) for k, w in anti.integral_b.items()
                            if w > 0}


def test_counters_follow_the_flips():
    m = am.Model(am.ANTIJOIN)
    m.step([(1, v, 1) for v in range(5)] + [(2, 0, 1)], [])
    # a key delta that flips nothing gathers nothing
    assert m.step([], [(1, 1)])[1:] == (1, 5, 0)
    assert m.step([], [(1, 1)])[1:] == (0, 0, 0)
    assert m.step([(1, 9, 1), (2, 9, 1)], [(3, 1)])[1:] == (1, 0, 1)


@pytest.mark.parametrize("tick,n_events,expect", [
    (1000, 20000, (1188, 207, 981, 12)),
    (37, 37 * 40, (81, 62, 19, 9)),
])
def test_query_103_figures(tick, n_events, expect):
    """Flips, rows gathered, rows filtered and the auctions still unbid at
    the end, on the stream tests/test_gpu_query_103.py runs."""
    events = gen.generate(20000, rate=100_000.0)
    model = am.Model(am.ANTIJOIN)
    tot = [0, 0, 0]
    for lo in range(0, n_events, tick):
        _, nf, ng, nd = model.step(*am.q103_deltas(events[lo:lo + tick]))
        tot = [tot[0] + nf, tot[1] + ng, tot[2] + nd]
    assert (*tot, len(model.acc)) == expect
