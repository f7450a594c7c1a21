"""q3's join tail around its on-chip cutoff: when the tick's emitted rows fit
one row per thread (total <= 1024) the tail hands them to the sort in
registers and never writes the capacity buffer; one row more takes the
buffer and the LDS bitonic.  Streams and the train driver are those of
test_gpu_q3_train; every observed output is compared with the CPU oracle
there, exactly."""
import os

import numpy as np
import pytest

from helpers import auction_event, person_event
from test_gpu_q3_train import (ID, WA, _auctions, _fanout_stream, _pad,
                               _run_trains, _tick_of)

pytestmark = pytest.mark.gpu

N_OUT = [1, 63, 64, 65, 1023, 1024, 1025]


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


def _cancel_stream():
    """Observed ticks (the last of each 3-tick call):
    tick 2  the same auction inserted and retracted for a known seller: the
            delta cancels, the tail's total is 0;
    tick 5  the seller's person row is retracted in the tick that brings 50
            auctions of theirs: +50 rows against the person spine, -50
            against the person delta — 100 emitted rows, nothing left;
    tick 8  the person comes back: 50 rows."""
    tick = 72
    ticks = [_pad([person_event(7, 21, 4, ID), person_event(8, 22, 4, WA)],
                  tick),
             _pad([], tick),
             _pad([auction_event(500, 7, 10), auction_event(500, 7, 10, w=-1)],
                  tick),
             _pad([], tick), _pad([], tick)]
    t5 = _tick_of(_auctions(np.arange(600, 650), 7), tick)
    t5[50] = person_event(7, 21, 4, ID, w=-1)
    ticks += [t5, _pad([], tick), _pad([], tick),
              _pad([person_event(7, 21, 4, ID)], tick)]
    return np.concatenate(ticks), tick


def _check_fanout(seen, n_out):
    assert len(seen[1]) == n_out and len(seen[2]) == n_out
    assert all(w == 1 for _, w in seen[1])
    assert all(w == -1 for _, w in seen[2])
    assert [kv for kv, _ in seen[1]] == [kv for kv, _ in seen[2]]


@pytest.mark.parametrize("n_out", N_OUT)
def test_tail_small_fanout(ctx, n_out):
    evs, tick = _fanout_stream(n_out)
    seen = _run_trains(ctx, evs, tick, note=f" tail fanout {n_out}")
    _check_fanout(seen, n_out)


def test_tail_small_consolidates_to_nothing(ctx):
    evs, tick = _cancel_stream()
    seen = _run_trains(ctx, evs, tick, note=" tail cancel")
    assert seen[0] == [] and seen[1] == []
    assert len(seen[2]) == 50 and all(w == 1 for _, w in seen[2])


def test_tail_small_fork_off_is_identical(ctx, ctx_nofork):
    streams = [_fanout_stream(n) for n in N_OUT] + [_cancel_stream()]
    for evs, tick in streams:
        a = _run_trains(ctx, evs, tick, note=" fork on")
        b = _run_trains(ctx_nofork, evs, tick, note=" fork off")
        assert a == b
