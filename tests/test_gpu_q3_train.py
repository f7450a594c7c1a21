"""q3's pipelined train (probe with start positions -> single-workgroup join
tail, accumulator merge forked to a side stream) against the CPU oracle.

`step_staged` never runs a train; `run_staged` does: inside one call every
tick after the first is a train commit.  Each case stages one stream, runs it
in consecutive 3-tick `run_staged` calls and compares the engine's output
after each call — the output of that call's last tick, a train commit — with
the oracle stepped through the same ticks.  Z-set equality, int64 weights,
no tolerance."""
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
    the main stream."""
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


def _run_trains(ctx, evs, tick, first=3, note=""):
    """Run evs through run_staged calls of 3 ticks (the first call `first`
    ticks, which shifts which ticks end a call and are observed).  Returns
    the observed outputs as sorted row lists, for run-to-run comparison."""
    from dbsp_amd.engine import Engine
    assert len(evs) % tick == 0
    eng = Engine(ctx, query=3)
    q = oracle.Query(3)
    eng.stage(evs)
    seen = []
    lo, nticks = 0, first
    try:
        while lo < len(evs):
            hi = min(lo + nticks * tick, len(evs))
            eng.run_staged(lo, hi, tick)
            got = eng.output()
            for t in range(lo, hi, tick):
                exp = q.step(evs[t:t + tick], cap=1 << 22)
            assert zset(got) == zset(exp), (
                f"q3 train{note}: call [{lo},{hi}) tick {tick}: last tick "
                f"diverged: {len(got)} vs {len(exp)} rows")
            seen.append(sorted(zset(got).items()))
            lo, nticks = hi, 3
    finally:
        eng.close()
        q.close()
    return seen


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
    """Auction events for many ids at once (auction_event's layout)."""
    ids = np.asarray(ids, dtype=np.uint64)
    out = np.empty(len(ids), dtype=EVENT_DT)
    out[:] = auction_event(0, seller, category, w=w)
    out["f0"] = ids
    return out


def _tick_of(arr, tick):
    out = _pad([], tick)
    out[:len(arr)] = arr
    return out


# ---- 1. empty sides ----

@pytest.mark.parametrize("first", [1, 2, 3])
def test_train_tiny_generated_ticks(ctx, first):
    """137-event ticks: most have an empty side, many are empty altogether."""
    evs = gen.generate(137 * 21, seed=13)
    _run_trains(ctx, evs, 137, first=first)


@pytest.mark.parametrize("first", [1, 2, 3])
def test_train_hand_built_empty_sides(ctx, first):
    tick = 8
    ticks = [
        # a person and an auction that both qualify (same-tick join)
        [person_event(1, 11, 0, OR), auction_event(100, 1, 10)],
        # no qualifying auction (category 9), a qualifying person
        [auction_event(101, 1, 9), person_event(2, 12, 1, CA)],
        # no qualifying person (WA), a qualifying auction of person 2
        [person_event(3, 13, 2, WA), auction_event(102, 2, 10)],
        # neither
        [person_event(4, 14, 3, WA), auction_event(103, 4, 3)],
        # nothing but bids
        [],
        # auctions only, for an old and an unknown seller
        [auction_event(104, 1, 10), auction_event(105, 9, 10)],
        # persons only: the unknown seller arrives, person 1 is retracted
        [person_event(9, 15, 4, ID), person_event(1, 11, 0, OR, w=-1)],
        [],
        [auction_event(106, 9, 10), auction_event(106, 9, 10, w=-1)],
    ]
    evs = np.concatenate([_pad(t, tick) for t in ticks])
    _run_trains(ctx, evs, tick, first=first)


# ---- 2. raw != consolidated inside a train tick ----

def _dups_stream():
    evs = gen.generate(5_000, seed=19)
    dup = evs[:2000].copy()
    neg = evs[:1000].copy()
    neg["w"] = -2
    # interleave so duplicates and their cancellations share ticks
    mixed = np.concatenate([evs[:1000], dup[:1000], neg, evs[1000:],
                            dup[1000:]])
    return mixed[:len(mixed) // 1000 * 1000]


def _retractions_stream():
    evs = gen.generate(30_000, seed=17)
    retract = evs[::3].copy()
    retract["w"] = -1
    mixed = np.concatenate([evs, retract])
    return mixed[:len(mixed) // 4000 * 4000]


@pytest.mark.parametrize("first", [1, 2, 3])
def test_train_duplicates_and_cancellations(ctx, first):
    _run_trains(ctx, _dups_stream(), 1000, first=first, note="+dups")


@pytest.mark.parametrize("first", [2, 3])
def test_train_retractions(ctx, first):
    _run_trains(ctx, _retractions_stream(), 4000, first=first,
                note="+retractions")


# ---- 3. fan-out from a multi-batch spine ----

def _fanout_stream(n_out, retract=True):
    """One seller's n_out category-10 auctions arrive over ticks 0..4, so at
    tick 5 they sit in several spine batches and the accumulator.  Tick 5
    brings the seller's person row (n_out output rows); with retract, tick 8
    takes it back (n_out rows of weight -1).  Both are the last tick of a
    3-tick call."""
    per = -(-n_out // 5)
    tick = per + 8
    ids = np.arange(1000, 1000 + n_out)
    ticks = [_tick_of(_auctions(ids[i * per:(i + 1) * per], 7), tick)
             for i in range(5)]
    ticks.append(_pad([person_event(7, 21, 4, ID),
                       person_event(8, 22, 4, WA)], tick))
    if not retract:
        return np.concatenate(ticks), tick
    ticks.append(_pad([auction_event(5, 8, 10)], tick))
    ticks.append(_pad([], tick))
    ticks.append(_pad([person_event(7, 21, 4, ID, w=-1)], tick))
    return np.concatenate(ticks), tick


FANOUT = [2048, 2049, 8192, 8193]


@pytest.mark.parametrize("n_out", FANOUT)
def test_train_fanout_multi_batch(ctx, n_out):
    """Output sizes at the sort's bitonic/radix cutoff (2048 / 2049) and at
    the tail's capacity (8192) with the first size that takes the sized-sort
    fallback from the capacity buffer (8193)."""
    evs, tick = _fanout_stream(n_out)
    seen = _run_trains(ctx, evs, tick, note=f" fanout {n_out}")
    assert len(seen[1]) == n_out and len(seen[2]) == n_out


# ---- 4. emit overflow ----

def test_train_emit_overflow(ctx):
    """More matches than the capacity buffer holds (32768): the tick is
    replayed from the tail kernel's offsets and totals."""
    n_out = 33_000
    evs, tick = _fanout_stream(n_out, retract=False)
    seen = _run_trains(ctx, evs, tick, note=" emit overflow")
    assert len(seen[1]) == n_out


# ---- 5. lost speculation mid-run ----

@pytest.mark.parametrize("side", ["auctions", "persons"])
def test_train_lost_speculation_mid_run(ctx, side):
    """Tick 4 (the middle of the second call) has more than 8192 qualifying
    rows on one side: its train loses the delta-sort speculation and is
    replayed; ticks 5.. are trains again and must see the replayed tick's
    rows in the spines (their sellers / auctions refer back to it)."""
    tick = 8300
    n_big = 8200
    base = gen.generate(tick * 9, seed=23)
    ticks = [base[i * tick:(i + 1) * tick].copy() for i in range(9)]
    big = _pad([], tick)
    if side == "auctions":
        # sellers 1..40 get 205 auctions each; their persons come later
        ids = np.arange(10_000_000, 10_000_000 + n_big)
        big[:n_big] = _auctions(ids, 0)
        big["f1"][:n_big] = 1 + ids % 40
        later = [person_event(s, 30 + s, 1, CA) for s in range(1, 41)]
    else:
        big[:n_big] = person_event(0, 0, 2, OR)
        big["f0"][:n_big] = np.arange(20_000_000, 20_000_000 + n_big)
        big["f1"][:n_big] = np.arange(n_big) % 1000
        later = [auction_event(30_000_000 + i, 20_000_000 + 37 * i, 10)
                 for i in range(200)]
    ticks[4] = big
    # references back to the big tick, split over the two ticks after it
    half = len(later) // 2
    ticks[5][:half] = events(*later[:half])
    ticks[6][:len(later) - half] = events(*later[half:])
    evs = np.concatenate(ticks)
    for first in (2, 3):  # tick 5 / tick 4.. end a call
        _run_trains(ctx, evs, tick, first=first, note=f" lost spec {side}")


# ---- 6. same-tick join ----

def test_train_same_tick_join_on_empty_spines(ctx):
    """Plan 3 alone: a person and that person's auctions arrive in one tick
    — a train commit — with nothing in either spine."""
    tick = 300
    same = [person_event(5, 40, 3, OR)] + \
           [auction_event(500 + i, 5, 10) for i in range(250)] + \
           [auction_event(900, 5, 11), auction_event(901, 6, 10)]
    evs = np.concatenate([_pad([], tick), _pad([], tick), _pad(same, tick)])
    seen = _run_trains(ctx, evs, tick)
    assert len(seen[0]) == 250


# ---- 7. single-stream equivalence ----

def test_train_fork_off_is_identical(ctx, ctx_nofork):
    streams = [(_dups_stream(), 1000), (_retractions_stream(), 4000)]
    streams += [_fanout_stream(n) for n in FANOUT]
    for evs, tick in streams:
        a = _run_trains(ctx, evs, tick, note=" fork on")
        b = _run_trains(ctx_nofork, evs, tick, note=" fork off")
        assert a == b
