"""The front of q3's pipelined train: block-level flatmap tickets, the delta
sorts that take the flatmap's counters and hand them back zeroed (so a
train's flatmap runs without a counter fill), and the barrier-free
accumulator fold.  Streams and the train driver are those of
test_gpu_q3_train; every observed output is compared with the CPU oracle,
exactly (Z-set equality, int64 weights)."""
import os

import numpy as np
import pytest

from dbsp_amd import EVENT_DT, gen, oracle
from helpers import bid_event, person_event, zset
from test_gpu_q3_train import CA, ID, OR, _auctions, _run_trains, _tick_of

pytestmark = pytest.mark.gpu

# one row, every lane of a wave, every wave of a 1024-thread block, one past
# each, partial last blocks, more than two blocks
TICKS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_nofold():
    """A context created with the fold knob off: the train keeps the general
    multi-workgroup merge for its accumulators."""
    from dbsp_amd.engine import Ctx
    old = os.environ.get("DBSP_Q3_FOLD")
    os.environ["DBSP_Q3_FOLD"] = "0"
    try:
        c = Ctx(0)
    finally:
        if old is None:
            del os.environ["DBSP_Q3_FOLD"]
        else:
            os.environ["DBSP_Q3_FOLD"] = old
    yield c
    c.close()


def _persons(ids, state=OR, w=1):
    ids = np.asarray(ids, dtype=np.uint64)
    out = np.empty(len(ids), dtype=EVENT_DT)
    out[:] = person_event(0, 0, 2, state, w=w)
    out["f0"] = ids
    out["f1"] = ids % 1000
    return out


# ---- 1. tickets: all lanes / all waves / no wave, per stream ----

def _all_or_nothing_stream(n):
    """Six ticks of n events, each of one kind only: every event a qualifying
    person (tick 0), every event a qualifying auction of one of them (1, 3),
    nothing qualifying (2, 5), every event a retraction of tick 0's persons
    (4).  Ticks 1 and 3 emit n rows each, tick 4 takes 2n back."""
    pid = np.arange(5000, 5000 + n)
    bids = np.empty(n, dtype=EVENT_DT)
    bids[:] = bid_event(1, 0)
    a1 = _auctions(np.arange(100_000, 100_000 + n), 0)
    a1["f1"] = pid
    a3 = _auctions(np.arange(200_000, 200_000 + n), 0)
    a3["f1"] = pid[::-1]
    return np.concatenate([_persons(pid), a1, bids, a3,
                           _persons(pid, w=-1), bids])


@pytest.mark.parametrize("n", TICKS)
def test_front_all_or_nothing_ticks(ctx, n):
    evs = _all_or_nothing_stream(n)
    # first = 1, 2, 3 end calls at ticks {0, 3, 5}, {1, 4, 5}, {2, 5}: every
    # tick is observed, and each is a train commit in at least one run
    seen = {f: _run_trains(ctx, evs, n, first=f, note=f" front n={n}")
            for f in (1, 2, 3)}
    assert len(seen[2][0]) == n            # tick 1: n rows
    assert len(seen[1][1]) == n            # tick 3: n more
    assert len(seen[2][1]) == 2 * n        # tick 4: all retracted
    assert all(w == -1 for _, w in seen[2][1])
    assert seen[3][0] == [] and seen[1][2] == []


# ---- 2. counter hand-back: fill and no-fill fronts interleaved ----

def _run_mixed(ctx, evs, tick, first, note=""):
    """run_staged calls (trains: no counter fill after a taking sort) with a
    single out-of-band step_staged tick (fill, base 0) after each; the oracle
    is compared after every call."""
    from dbsp_amd.engine import Engine
    assert len(evs) % tick == 0
    eng = Engine(ctx, query=3)
    q = oracle.Query(3)
    eng.stage(evs)
    lo, nticks, single = 0, first, False
    try:
        while lo < len(evs):
            hi = min(lo + (1 if single else nticks) * tick, len(evs))
            if single:
                eng.step_staged(lo, hi)
            else:
                eng.run_staged(lo, hi, tick)
            got = eng.output()
            for t in range(lo, hi, tick):
                exp = q.step(evs[t:t + tick], cap=1 << 22)
            assert zset(got) == zset(exp), (
                f"q3 front{note}: [{lo},{hi}) tick {tick} "
                f"{'step' if single else 'run'}: {len(got)} vs {len(exp)} rows")
            lo, nticks, single = hi, 3, not single
    finally:
        eng.close()
        q.close()


@pytest.mark.parametrize("first", [1, 2, 3])
def test_front_counter_handback_interleaved(ctx, first):
    evs = gen.generate(700 * 20, seed=29)
    _run_mixed(ctx, evs, 700, first, note=f" first={first}")


@pytest.mark.parametrize("first", [1, 2, 3])
def test_front_handback_after_lost_speculation(ctx, first):
    """Tick 4 has 8200 qualifying auctions: whichever way it runs, its delta
    sort loses the speculation, and as a train its replay reads the raw
    counts from the slots the taking sort left them in.  The ticks after it
    are trains again (no counter fill) and join against its rows."""
    tick, n_big = 8300, 8200
    base = gen.generate(tick * 10, seed=31)
    ticks = [base[i * tick:(i + 1) * tick].copy() for i in range(10)]
    ids = np.arange(10_000_000, 10_000_000 + n_big)
    big = _tick_of(_auctions(ids, 0), tick)
    big["f1"][:n_big] = 1 + ids % 40
    ticks[4] = big
    sellers = _persons(np.arange(1, 41), state=CA)
    ticks[5][:20] = sellers[:20]
    ticks[7][:20] = sellers[20:]
    evs = np.concatenate(ticks)
    _run_trains(ctx, evs, tick, first=first, note=" lost spec, hand-back")
    _run_mixed(ctx, evs, tick, first, note=" lost spec, mixed")


# ---- 3. accumulators across the spill threshold ----

def _spill_stream():
    """~4000 qualifying auctions per tick for ten ticks (the auction
    accumulator passes the 32768-row spill threshold at tick 8) for sellers
    1..500, of whom 1..250 are known from tick 0 on; tick 10 brings the
    other sellers' persons, tick 11 retracts every tenth auction."""
    tick, per = 4300, 4000
    ticks = []
    for t in range(10):
        ids = np.arange(1_000_000 + t * per, 1_000_000 + (t + 1) * per)
        a = _tick_of(_auctions(ids, 0), tick)
        a["f1"][:per] = 1 + ids % 500
        ticks.append(a)
    ticks[0][per:per + 250] = _persons(np.arange(1, 251), state=ID)
    ticks.append(_tick_of(_persons(np.arange(251, 501), state=ID), tick))
    ids = np.arange(1_000_000, 1_000_000 + 10 * per, 10)
    r = _auctions(ids, 0, w=-1)
    r["f1"] = 1 + ids % 500
    ticks.append(_tick_of(r, tick))
    return np.concatenate(ticks), tick


def test_front_accumulator_across_spill(ctx, ctx_nofold):
    evs, tick = _spill_stream()
    a = _run_trains(ctx, evs, tick, note=" spill, fold")
    b = _run_trains(ctx_nofold, evs, tick, note=" spill, general merge")
    assert a == b
    assert [len(x) for x in a] == [2000, 2000, 2000, 4000]
    assert all(w == -1 for _, w in a[-1])


def test_front_fold_off_is_identical(ctx, ctx_nofold):
    for n in (65, 1025):
        evs = _all_or_nothing_stream(n)
        for f in (2, 3):
            assert _run_trains(ctx, evs, n, first=f) == \
                _run_trains(ctx_nofold, evs, n, first=f)


# ---- 4. q5 and q8 share the flatmap's ticket scheme ----

@pytest.mark.parametrize("query", [5, 8])
def test_front_shared_flatmap_other_queries(ctx, query):
    from dbsp_amd.engine import Engine
    tick = 1025
    evs = gen.generate(tick * 6, seed=37)
    eng = Engine(ctx, query=query)
    q = oracle.Query(query)
    eng.stage(evs)
    try:
        for lo in range(0, len(evs), 2 * tick):
            eng.run_staged(lo, lo + 2 * tick, tick)
            got = eng.output()
            for t in range(lo, lo + 2 * tick, tick):
                exp = q.step(evs[t:t + tick], cap=1 << 22)
            assert zset(got) == zset(exp), (
                f"q{query} tick {tick} [{lo},..): {len(got)} vs {len(exp)}")
    finally:
        eng.close()
        q.close()
