"""Engine query 102 on the GPU: the per-auction rolling highest (or lowest)
bid, bids.map_index(|b| (b.auction, (b.date_time, b.price)))
.partitioned_rolling_aggregate(Max | Min, range), against the numpy model of
tests/rolling_minmax_model.py fed (auction, date_time, price, w)."""
import numpy as np
import pytest

from dbsp_amd import KIND_BID, gen
from helpers import bid_event, events as make_events, zset
from rolling_minmax_model import (apply_delta, expected_delta, full_output,
                                  zset_diff)

pytestmark = pytest.mark.gpu

BEFORE, AFTER = 50, 0


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def events():
    ev = gen.generate(20000, rate=100_000.0)
    bt = ev["f3"][ev["kind"] == KIND_BID]
    assert int(bt.max()) - int(bt.min()) > BEFORE
    return ev


def _assert_consolidated(rows):
    if len(rows) == 0:
        return
    assert (rows["w"] != 0).all()
    k, v = rows["k"], rows["v"]
    inc = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1]))
    assert inc.all(), "output not sorted by (k, v) / not distinct"


def _bid_delta(ev):
    b = ev[ev["kind"] == KIND_BID]
    return [(int(a), int(t), int(pr), int(w))
            for a, t, pr, w in zip(b["f0"], b["f3"], b["f2"], b["w"])]


def _engine(ctx, agg=None):
    from dbsp_amd.engine import Engine
    eng = Engine(ctx, query=102)
    eng.rolling_init(BEFORE, AFTER)
    if agg is not None:
        eng.rolling_agg(agg)
    return eng


def _run_stepped(ctx, events, n_events, tick, agg=None):
    """Staged ticks next to the model; returns the per-tick outputs."""
    eng = _engine(ctx, agg)
    eng.stage(events)
    model_agg = agg or "max"
    integral, acc, outs = {}, {}, []
    for lo in range(0, n_events, tick):
        hi = min(lo + tick, n_events)
        eng.step_staged(lo, hi)
        rows = eng.output()
        _assert_consolidated(rows)
        got = zset(rows)
        delta = _bid_delta(events[lo:hi])
        assert got == expected_delta(integral, delta, BEFORE, AFTER,
                                     model_agg), f"tick [{lo},{hi})"
        integral = apply_delta(integral, delta)
        acc = zset_diff(acc, {k: -w for k, w in got.items()})
        outs.append(rows)
    assert acc == full_output(integral, BEFORE, AFTER, model_agg)
    for call in (lambda: eng.rolling_init(BEFORE, AFTER),
                 lambda: eng.rolling_agg("max"),
                 lambda: eng.rolling_lateness(5)):
        with pytest.raises(RuntimeError):
            call()                  # rejected after stepping
    eng.close()
    return outs


@pytest.fixture(scope="module")
def stepped_1000(ctx, events):
    return _run_stepped(ctx, events, len(events), 1000)


def test_ticks_of_1000(stepped_1000):
    assert sum(len(o) for o in stepped_1000) > 0


def test_ticks_of_37(ctx, events):
    _run_stepped(ctx, events, 37 * 40, 37)


def test_run_staged_equals_stepped(ctx, events, stepped_1000):
    eng = _engine(ctx)
    eng.stage(events)
    eng.run_staged(0, len(events), 1000)
    assert np.array_equal(eng.output(), stepped_1000[-1])
    eng.close()


def test_unstaged_step_equals_staged(ctx, events, stepped_1000):
    eng = _engine(ctx)
    for i in range(2):
        eng.step(events[i * 1000:(i + 1) * 1000])
        assert np.array_equal(eng.output(), stepped_1000[i])
    eng.close()


def test_min_through_rolling_agg(ctx, events, stepped_1000):
    outs = _run_stepped(ctx, events, 5000, 1000, agg="min")
    assert any(a.tobytes() != b.tobytes()
               for a, b in zip(outs, stepped_1000))


def test_default_range(ctx, events):
    from dbsp_amd.engine import Engine
    eng = Engine(ctx, query=102)    # 10000 ms before, 0 after; Max
    eng.stage(events)
    eng.step_staged(0, 3000)
    assert zset(eng.output()) == expected_delta(
        {}, _bid_delta(events[:3000]), 10000, 0, "max")
    eng.close()


def test_lateness_bounds_the_traces(ctx):
    n_events, tick, lateness = 20000, 1000, 150
    ev = gen.generate(n_events, rate=10_000.0)
    bt = ev["f3"][ev["kind"] == KIND_BID].astype(np.int64)
    assert (np.diff(bt) >= 0).all(), "bid times are not monotone"
    for lo in range(0, n_events, tick):     # nothing can be late
        e = ev[lo:lo + tick]
        t = e["f3"][e["kind"] == KIND_BID].astype(np.int64)
        assert t.max() - t.min() <= lateness
    assert bt.max() - bt.min() > 4 * (lateness + BEFORE)

    def run(with_lateness):
        eng = _engine(ctx)
        if with_lateness:
            eng.rolling_lateness(lateness)
        eng.stage(ev)
        outs = []
        for lo in range(0, n_events, tick):
            eng.step_staged(lo, lo + tick)
            outs.append(eng.output())
        st = eng.rolling_stats()
        eng.close()
        return outs, st

    plain, (p_in, p_out, p_late, p_sweeps) = run(False)
    bounded, (b_in, b_out, b_late, b_sweeps) = run(True)
    assert sum(len(o) for o in plain) > 0
    for i, (a, b) in enumerate(zip(plain, bounded)):
        assert a.tobytes() == b.tobytes(), f"tick {i}"
    assert (p_late, p_sweeps, b_late) == (0, 0, 0)
    assert b_sweeps >= 2
    assert b_in < p_in and b_out < p_out


def test_rejected_on_another_query(ctx):
    from dbsp_amd.engine import Engine
    q3 = Engine(ctx, query=3)
    for call in (lambda: q3.rolling_agg("min"), lambda: q3.rolling_init(1, 1),
                 lambda: q3.rolling_lateness(1)):
        with pytest.raises(RuntimeError):
            call()
    q3.close()
    q101 = Engine(ctx, query=101)   # the sum query has no aggregator to pick
    with pytest.raises(RuntimeError):
        q101.rolling_agg("max")
    q101.close()
    eng = Engine(ctx, query=102)
    with pytest.raises(RuntimeError):
        eng.rolling_agg("sum")      # Max or Min only
    eng.close()


@pytest.mark.parametrize("field", ["price", "date_time"])
def test_field_overflow_is_an_error(ctx, field):
    eng = _engine(ctx)
    eng.step(make_events(bid_event(7, 100, price=5), bid_event(7, 120, price=9),
                         bid_event(8, 110, price=3)))
    assert len(eng.output()) == 3
    stats = eng.rolling_stats()
    bad = (bid_event(7, 130, price=1 << 32) if field == "price"
           else bid_event(7, 1 << 32, price=4))
    with pytest.raises(RuntimeError):
        eng.step(make_events(bid_event(8, 125, price=2), bad,
                             bid_event(9, 126, price=1)))
    assert eng.rolling_stats() == stats
    # the engine goes on as if the tick had not been sent
    eng.step(make_events(bid_event(7, 140, price=(1 << 32) - 1)))
    assert zset(eng.output()) == {
        ((7 << 32) | 140, (1 << 32) - 1): 1}
    eng.close()
