"""q3's re-forked train: the loop stream carries flatmap, delta sorts, fold
and head readback; probe, join tail and tail readback run on the back stream
and are joined only on demand.  These streams put a tick's back-stream work
under exactly the commit paths that free, recycle or overwrite what it uses:
a spill with its deferred resolve and cascade, a short or long next tick in
the other arena half, an emit-overflow replay beside the next train, and a
lost speculation behind the slowest tail.

Every observed output — the output of the last tick of each `run_staged`
call; a middle tick's output cannot be read back — is compared with
`oracle.Query(3)` stepped through the same ticks: Z-set equality, int64
weights, no tolerance.  The oracle runs once per stream."""
import os

import numpy as np
import pytest

from dbsp_amd import EVENT_DT, gen, oracle
from helpers import auction_event, bid_event, events, person_event, zset

pytestmark = pytest.mark.gpu

CA, ID, OR, WA = 1, 2, 3, 4  # helpers.STATE_IDS; q3 keeps CA, ID, OR


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_nofork():
    """A context created with the fork knob off: the whole train stays on
    one stream."""
    from dbsp_amd.engine import Ctx
    old = os.environ.get("DBSP_Q3_FORK")
    os.environ["DBSP_Q3_FORK"] = "0"
    try:
        c = Ctx(0)
    finally:
        if old is None:
            del os.environ["DBSP_Q3_FORK"]
        else:
            os.environ["DBSP_Q3_FORK"] = old
    yield c
    c.close()


def _tick_bounds(lo, hi, tick):
    return [(t, min(t + tick, hi)) for t in range(lo, hi, tick)]


_ORACLE = {}


def _expected(name, evs, calls, tick):
    """Oracle output of every tick of the calls [(lo, hi), ...], keyed by the
    tick's (lo, hi); computed once per (stream name, tick boundaries)."""
    ticks = tuple(b for lo, hi in calls for b in _tick_bounds(lo, hi, tick))
    key = (name, ticks)
    if key not in _ORACLE:
        q = oracle.Query(3)
        try:
            _ORACLE[key] = {b: zset(q.step(evs[b[0]:b[1]], cap=1 << 22))
                            for b in ticks}
        finally:
            q.close()
    return _ORACLE[key]


def _run_calls(ctx, name, evs, calls, tick, note=""):
    """One engine, one run_staged(lo, hi, tick) per entry of calls; after each
    the engine's output is compared with the oracle's for the call's last
    tick.  Returns the observed outputs as sorted row lists."""
    from dbsp_amd.engine import Engine
    exp = _expected(name, evs, calls, tick)
    eng = Engine(ctx, query=3)
    eng.stage(evs)
    seen = []
    try:
        for lo, hi in calls:
            eng.run_staged(lo, hi, tick)
            got = zset(eng.output())
            want = exp[_tick_bounds(lo, hi, tick)[-1]]
            assert got == want, (
                f"q3 refork {name}{note}: call [{lo},{hi}) tick {tick}: last "
                f"tick diverged: {len(got)} vs {len(want)} rows")
            seen.append(sorted(got.items()))
    finally:
        eng.close()
    return seen


def _split(nticks, tick, counts):
    """Call ranges of counts[i] ticks each over nticks ticks."""
    assert sum(counts) == nticks
    out, lo = [], 0
    for c in counts:
        out.append((lo * tick, (lo + c) * tick))
        lo += c
    return out


def _pad(evs, tick):
    """One tick of exactly `tick` events: evs plus bids, which q3 ignores."""
    evs = list(evs)
    assert len(evs) <= tick
    out = np.empty(tick, dtype=EVENT_DT)
    out[:] = bid_event(1, 0)
    if evs:
        out[:len(evs)] = events(*evs)
    return out


def _auctions(ids, seller, category=10, w=1):
    ids = np.asarray(ids, dtype=np.uint64)
    out = np.empty(len(ids), dtype=EVENT_DT)
    out[:] = auction_event(0, seller, category, w=w)
    out["f0"] = ids
    return out


def _persons(ids, state=OR, w=1):
    ids = np.asarray(ids, dtype=np.uint64)
    out = np.empty(len(ids), dtype=EVENT_DT)
    out[:] = person_event(0, 0, 2, state, w=w)
    out["f0"] = ids
    out["f1"] = ids % 1000
    return out


def _tick_of(*parts, tick):
    out = _pad([], tick)
    arr = np.concatenate(parts)
    out[:len(arr)] = arr
    return out


# ---- 1. spill and deferred resolve inside one call ----

SPILL_TICK, SPILL_PER, SPILL_N = 4300, 4000, 20


def _spill_auctions():
    """4000 qualifying auctions with distinct ids per tick for 20 ticks: the
    auction accumulator passes 32768 rows at ticks 8 and 17, each seal's
    round is resolved at the commit after it, and the two sealed batches
    cascade.  Sellers 1..500; persons 1..250 arrive at tick 0 and 251..500
    at tick 12, so every probe has matches (tick 12: 28000 rows)."""
    ticks = []
    for t in range(SPILL_N):
        ids = np.arange(1_000_000 + t * SPILL_PER,
                        1_000_000 + (t + 1) * SPILL_PER)
        a = _auctions(ids, 0)
        a["f1"] = 1 + ids % 500
        parts = [a]
        if t == 0:
            parts.append(_persons(np.arange(1, 251), state=ID))
        if t == 12:
            parts.append(_persons(np.arange(251, 501), state=CA))
        ticks.append(_tick_of(*parts, tick=SPILL_TICK))
    return np.concatenate(ticks)


def _spill_persons():
    """The person side: 4000 qualifying persons with distinct ids per tick.
    Tick t also brings 150 auctions of persons of tick t-1 (tick 0: of its
    own persons, the same-tick join) and 100 auctions of persons who arrive
    at tick t+1, so all three plans match on every tick."""
    def pids(t):
        return np.arange(2_000_000 + t * SPILL_PER,
                         2_000_000 + (t + 1) * SPILL_PER)
    ticks = []
    for t in range(SPILL_N):
        old = pids(max(t - 1, 0))[7::26][:150]
        a = _auctions(np.arange(5_000_000 + t * 300,
                                5_000_000 + t * 300 + 150), 0)
        a["f1"] = old
        parts = [_persons(pids(t), state=(ID, OR, CA)[t % 3]), a]
        if t + 1 < SPILL_N:
            new = pids(t + 1)[11::39][:100]
            b = _auctions(np.arange(5_000_000 + t * 300 + 150,
                                    5_000_000 + t * 300 + 250), 0)
            b["f1"] = new
            parts.append(b)
        ticks.append(_tick_of(*parts, tick=SPILL_TICK))
    return np.concatenate(ticks)


_SPILL = {"auctions": _spill_auctions, "persons": _spill_persons}
_SPILL_EVS = {}


@pytest.mark.parametrize("counts", [(20,), (7, 13), (9, 11)],
                         ids=["one-call", "7+13", "9+11"])
@pytest.mark.parametrize("side", ["auctions", "persons"])
def test_refork_spill_and_deferred_resolve(ctx, ctx_nofork, side, counts):
    """The first seal (tick 8) is a middle tick of the one-call and 7+13
    forms and the last tick of the first call in 9+11; trains are in flight
    through both seals, the deferred resolves and the cascade."""
    if side not in _SPILL_EVS:
        _SPILL_EVS[side] = _SPILL[side]()
    evs = _SPILL_EVS[side]
    calls = _split(SPILL_N, SPILL_TICK, counts)
    name = f"spill-{side}"
    a = _run_calls(ctx, name, evs, calls, SPILL_TICK, note=" fork")
    b = _run_calls(ctx, name, evs, calls, SPILL_TICK, note=" fork, 2nd run")
    c = _run_calls(ctx_nofork, name, evs, calls, SPILL_TICK, note=" no fork")
    assert a == b and a == c
    assert all(len(x) > 0 for x in a)


# ---- 2. short last tick ----

def test_refork_short_last_tick(ctx):
    """The last train is smaller than its predecessor: its front lands in
    the other arena half, below the previous train's live buffers."""
    n = 3 * 1000 + 137
    evs = gen.generate(n, seed=43)
    _run_calls(ctx, "short-last", evs, [(0, n)], 1000)


def test_refork_short_then_long_across_calls(ctx):
    """The reverse across calls on one engine: a 137-event call, a
    1000-event call, then two 1000-event ticks in one call (a train again)."""
    evs = gen.generate(137 + 3 * 1000, seed=47)
    _run_calls(ctx, "short-then-long", evs,
               [(0, 137), (137, 1137), (1137, 3137)], 1000)


# ---- 3. emit overflow on a tick that is not the last of its call ----

def _overflow_stream(n_out=33_000):
    """Seller 7's n_out category-10 auctions arrive over ticks 0..4; tick 5
    brings seller 7's person row: n_out output rows, more than the capacity
    buffer holds, so the tick is replayed from the tail kernel's counts,
    offsets and totals — while the train of tick 6 is already enqueued.
    Tick 6 holds 100 qualifying auctions of seller 9 (known from tick 0), so
    that train's probe and tail write real counts and totals; tick 7 holds
    50 more."""
    per = -(-n_out // 5)
    tick = per + 8
    ids = np.arange(1000, 1000 + n_out)
    ticks = [_tick_of(_auctions(ids[i * per:(i + 1) * per], 7), tick=tick)
             for i in range(5)]
    ticks[0][per] = person_event(9, 23, 4, OR)
    ticks.append(_pad([person_event(7, 21, 4, ID),
                       person_event(8, 22, 4, WA)], tick))
    ticks.append(_tick_of(_auctions(np.arange(90_000, 90_100), 9), tick=tick))
    ticks.append(_tick_of(_auctions(np.arange(91_000, 91_050), 9), tick=tick))
    return np.concatenate(ticks), tick


@pytest.mark.parametrize("counts", [(8,), (3, 3, 2), (7, 1)],
                         ids=["one-call", "3-tick-calls", "7+1"])
def test_refork_emit_overflow_mid_call(ctx, counts):
    """One call: the replay of tick 5 runs beside train 6 and two commits
    follow it.  3-tick calls observe the replayed tick itself.  7+1 observes
    tick 6, whose join tail leaves its totals in the length slots the
    replay's sized ops borrow."""
    evs, tick = _overflow_stream()
    seen = _run_calls(ctx, "overflow", evs, _split(8, tick, counts), tick)
    if counts == (3, 3, 2):
        assert len(seen[1]) == 33_000
    if counts == (7, 1):
        assert len(seen[0]) == 100
    assert len(seen[-1]) == 50


# ---- 4. lost speculation with live back-stream work ----

def _lost_spec_stream():
    """Tick 3's join fans out to 8193 output rows — one past the tail's
    fused output sort, its slowest path — and tick 4, whose train is
    enqueued while that tail runs, has 8200 qualifying auctions: its train
    loses the delta-sort speculation and is replayed.  Ticks 5 and 6 bring
    the persons of tick 4's sellers."""
    tick, n_big, n_fan = 8300, 8200, 8193
    fan = np.arange(40_000_000, 40_000_000 + n_fan)
    ticks = [_tick_of(_auctions(fan[i::3], 1007), tick=tick)
             for i in range(3)]
    ticks.append(_pad([person_event(1007, 50, 1, OR)], tick))
    ids = np.arange(10_000_000, 10_000_000 + n_big)
    big = _tick_of(_auctions(ids, 0), tick=tick)
    big["f1"][:n_big] = 1 + ids % 40
    ticks.append(big)
    later = [person_event(s, 30 + s, 1, CA) for s in range(1, 41)]
    ticks.append(_pad(later[:20], tick))
    ticks.append(_pad(later[20:], tick))
    return np.concatenate(ticks), tick


@pytest.mark.parametrize("counts", [(7,), (4, 3), (5, 2)],
                         ids=["one-call", "4+3", "5+2"])
def test_refork_lost_speculation_behind_slow_tail(ctx, counts):
    """One call runs it whole; 4+3 observes the 8193-row tick, 5+2 the
    replayed one."""
    evs, tick = _lost_spec_stream()
    seen = _run_calls(ctx, "lost-spec", evs, _split(7, tick, counts), tick)
    if counts == (4, 3):
        assert len(seen[0]) == 8193
    assert len(seen[-1]) == 20 * 205
