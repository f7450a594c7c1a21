"""Engine query 7 on the GPU: the highest bids of the last tumbled window
(Nexmark q7: bids by time, the monotone watermark, the tumbling window, the
arg-max operator), against the reference's own test cases
(tests/golden/q7_highest_bid.json) and the Python q7 of tests/argmax_model.py.
Output rows are k = price << 32 | date_time, v = auction << 32 | bidder."""
import numpy as np
import pytest

import argmax_model as am
from dbsp_amd import KIND_BID, gen
from helpers import bid_event, events as make_events, load_golden, zset

pytestmark = pytest.mark.gpu

GOLD = load_golden("q7_highest_bid.json")


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def events():
    # 400 events/s: 20000 events span 50 s of event time, five tumbles
    return gen.generate(20000, rate=400.0)


def _assert_consolidated(rows):
    if len(rows) == 0:
        return
    assert (rows["w"] != 0).all()
    k, v = rows["k"], rows["v"]
    inc = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1]))
    assert inc.all(), "output not sorted by (k, v) / not distinct"


def _bids(ev):
    b = ev[ev["kind"] == KIND_BID]
    return list(zip(b["f0"].tolist(), b["f1"].tolist(), b["f2"].tolist(),
                    b["f3"].tolist(), b["w"].tolist()))


def _engine(ctx):
    from dbsp_amd.engine import Engine
    return Engine(ctx, query=7)


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_golden_cases(ctx, case):
    eng = _engine(ctx)
    d = GOLD["defaults"]
    for tick, expected in zip(case["ticks"], case["expected"]):
        eng.step(make_events(*[
            bid_event(d["auction"], b["date_time"], bidder=d["bidder"],
                      price=b["price"]) for b in tick]))
        rows = eng.output()
        _assert_consolidated(rows)
        assert zset(rows) == {
            am.q7_pack(r["auction"], r["bidder"], r["price"],
                       r["date_time"]): r["weight"] for r in expected}
    eng.close()


def _run_stepped(ctx, events, n_events, tick):
    """Staged ticks next to the Python q7; returns the per-tick outputs, the
    stats and the model."""
    eng = _engine(ctx)
    eng.stage(events)
    q = am.Q7()
    outs = []
    for lo in range(0, n_events, tick):
        hi = min(lo + tick, n_events)
        eng.step_staged(lo, hi)
        rows = eng.output()
        _assert_consolidated(rows)
        assert zset(rows) == q.step(_bids(events[lo:hi])), f"tick [{lo},{hi})"
        outs.append(rows)
    st = eng.argmax_stats()
    assert st["groups_refilled"] == q.refills
    assert st["in_rows"] >= len(q.windowed)
    eng.close()
    return outs, st, q


@pytest.fixture(scope="module")
def stepped_1000(ctx, events):
    return _run_stepped(ctx, events, len(events), 1000)


def test_ticks_of_1000(stepped_1000):
    outs, st, q = stepped_1000
    assert q.tumbles >= 3
    assert sum(len(o) for o in outs) > 0
    # an in-order stream changes the window only when it tumbles; a tumble
    # retracts the old maximum and refills unless the new window holds a bid
    # at least as high (_run_stepped holds the count to the model's)
    assert 3 <= st["groups_seen"] <= q.tumbles
    assert st["rows_gathered"] > 0 or st["groups_refilled"] == 0


def test_ticks_of_37(ctx, events):
    # 37 * 300 events span 27 s: the window tumbles here too
    _, _, q = _run_stepped(ctx, events, 37 * 300, 37)
    assert q.tumbles >= 1


def test_run_staged_equals_stepped(ctx, events, stepped_1000):
    eng = _engine(ctx)
    eng.stage(events)
    eng.run_staged(0, len(events), 1000)
    assert np.array_equal(eng.output(), stepped_1000[0][-1])
    assert eng.argmax_stats() == stepped_1000[1]
    eng.close()


def test_unstaged_step_equals_staged(ctx, events, stepped_1000):
    eng = _engine(ctx)
    for i in range(8):
        eng.step(events[i * 1000:(i + 1) * 1000])
        assert np.array_equal(eng.output(), stepped_1000[0][i])
    eng.close()


def test_retractions_through_the_engine(ctx):
    """Event weights reach the operator: the top bid taken back inside the
    window is replaced by the next price."""
    eng = _engine(ctx)
    eng.step(make_events(bid_event(1, 11_000, bidder=1, price=50),
                         bid_event(2, 12_000, bidder=2, price=90),
                         bid_event(4, 12_500, bidder=4, price=50, w=2),
                         bid_event(3, 32_000, bidder=3, price=10)))
    assert zset(eng.output()) == {am.q7_pack(2, 2, 90, 12_000): 1}
    before = eng.argmax_stats()["groups_refilled"]
    eng.step(make_events(bid_event(2, 12_000, bidder=2, price=90, w=-1)))
    assert zset(eng.output()) == {am.q7_pack(2, 2, 90, 12_000): -1,
                                  am.q7_pack(1, 1, 50, 11_000): 1,
                                  am.q7_pack(4, 4, 50, 12_500): 2}
    assert eng.argmax_stats()["groups_refilled"] == before + 1
    eng.close()


def test_a_tick_without_bids_changes_nothing(ctx):
    from helpers import auction_event
    eng = _engine(ctx)
    eng.step(make_events(bid_event(1, 11_000, price=50),
                         bid_event(1, 32_000, price=10)))
    assert len(eng.output()) == 1
    stats = eng.argmax_stats()
    eng.step(make_events(auction_event(5, 6, 7, dt=90_000)))
    assert len(eng.output()) == 0 and eng.argmax_stats() == stats
    eng.close()


def test_world_2_is_rejected(ctx):
    from dbsp_amd.engine import Engine
    with pytest.raises(RuntimeError):
        Engine(ctx, query=7, rank=0, world=2)


def test_argmax_stats_rejected_on_other_queries(ctx):
    from dbsp_amd.engine import Engine
    for q in (3, 19):
        other = Engine(ctx, query=q)
        with pytest.raises(RuntimeError):
            other.argmax_stats()
        other.close()


@pytest.mark.parametrize("field", ["auction", "price", "bidder", "date_time"])
def test_field_overflow_is_an_error(ctx, field):
    eng = _engine(ctx)
    eng.step(make_events(bid_event(7, 11_000, bidder=2, price=5),
                         bid_event(7, 12_000, bidder=3, price=9),
                         bid_event(8, 32_000, bidder=4, price=3)))
    first = eng.output()
    assert zset(first) == {am.q7_pack(7, 3, 9, 12_000): 1}
    stats = eng.argmax_stats()
    good = dict(auction=7, dt=13_000, bidder=1, price=4)
    wide = {"auction": ("auction", 1 << 32), "price": ("price", 1 << 27),
            "bidder": ("bidder", 1 << 32), "date_time": ("dt", 1 << 32)}
    name, value = wide[field]
    bad = dict(good)
    bad[name] = value
    with pytest.raises(RuntimeError):
        eng.step(make_events(bid_event(8, 12_500, price=20), bid_event(**bad),
                             bid_event(9, 12_600, price=1)))
    assert eng.argmax_stats() == stats
    assert np.array_equal(eng.output(), first)
    # the engine goes on as if the tick had not been sent: the watermark
    # stands, so a late bid inside the window still counts; the widest values
    # that fit are accepted
    eng.step(make_events(bid_event((1 << 32) - 1, 19_999,
                                   bidder=(1 << 32) - 1,
                                   price=(1 << 27) - 1)))
    assert zset(eng.output()) == {
        am.q7_pack(7, 3, 9, 12_000): -1,
        am.q7_pack((1 << 32) - 1, (1 << 32) - 1, (1 << 27) - 1, 19_999): 1}
    assert eng.argmax_stats()["in_rows"] == stats["in_rows"] + 1
    # the widest date_time moves the window past everything so far
    eng.step(make_events(bid_event(1, (1 << 32) - 1, price=1)))
    assert len(eng.output()) == 1 and eng.output()["w"][0] == -1
    eng.close()
