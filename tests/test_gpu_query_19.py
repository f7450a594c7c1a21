"""Engine query 19 on the GPU: the top K bids of every auction (Nexmark q19,
bids.flat_map_index(|b| (b.auction, (b.price, b))) into the top-K operator),
against the reference's own test cases (tests/golden/q19_top_bids.json) and
the dict model of tests/topk_model.py fed the packed rows
k = auction << 27 | price, v = bidder << 32 | date_time."""
import numpy as np
import pytest

import topk_model as tm
from dbsp_amd import KIND_BID, gen
from helpers import bid_event, events as make_events, load_golden, zset

pytestmark = pytest.mark.gpu

GOLD = load_golden("q19_top_bids.json")


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def events():
    return gen.generate(20000, rate=100_000.0)


def _assert_consolidated(rows):
    if len(rows) == 0:
        return
    assert (rows["w"] != 0).all()
    k, v = rows["k"], rows["v"]
    inc = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1]))
    assert inc.all(), "output not sorted by (k, v) / not distinct"


def _bid_delta(ev):
    b = ev[ev["kind"] == KIND_BID]
    return [tm.q19_pack(a, bd, pr, t) + (int(w),)
            for a, bd, pr, t, w in zip(b["f0"].tolist(), b["f1"].tolist(),
                                       b["f2"].tolist(), b["f3"].tolist(),
                                       b["w"].tolist())]


def _engine(ctx, k=None):
    from dbsp_amd.engine import Engine
    eng = Engine(ctx, query=19)
    if k is not None:
        eng.topk_init(k)
    return eng


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_golden_cases(ctx, case):
    eng = _engine(ctx)              # the default K is the reference's 10
    assert GOLD["k"] == 10
    for tick, expected in zip(case["ticks"], case["expected"]):
        eng.step(make_events(*[
            bid_event(b["auction"], GOLD["defaults"]["date_time"],
                      bidder=b["bidder"], price=b["price"]) for b in tick]))
        rows = eng.output()
        _assert_consolidated(rows)
        assert zset(rows) == {
            tm.q19_pack(r["auction"], r["bidder"], r["price"],
                        r["date_time"]): r["weight"] for r in expected}
    eng.close()


def _run_stepped(ctx, events, n_events, tick, k=None):
    """Staged ticks next to the model; returns the per-tick outputs."""
    eng = _engine(ctx, k)
    eng.stage(events)
    model = tm.Model(10 if k is None else k, tm.Q19_SHIFT)
    outs, refills = [], 0
    for lo in range(0, n_events, tick):
        hi = min(lo + tick, n_events)
        eng.step_staged(lo, hi)
        rows = eng.output()
        _assert_consolidated(rows)
        exp, n_refill, _ = model.step(_bid_delta(events[lo:hi]))
        assert zset(rows) == exp, f"tick [{lo},{hi})"
        refills += n_refill
        outs.append(rows)
    st = eng.topk_stats()
    assert st["groups_refilled"] == refills
    assert model.acc == tm.full_output(model.integral, model.K, tm.Q19_SHIFT)
    with pytest.raises(RuntimeError):
        eng.topk_init(5)            # rejected after stepping
    eng.close()
    return outs, st


@pytest.fixture(scope="module")
def stepped_1000(ctx, events):
    return _run_stepped(ctx, events, len(events), 1000)


def test_ticks_of_1000(stepped_1000):
    outs, st = stepped_1000
    assert sum(len(o) for o in outs) > 0
    # the generated bids are insert-only
    assert st["groups_refilled"] == 0 and st["rows_gathered"] == 0


def test_ticks_of_37(ctx, events):
    _run_stepped(ctx, events, 37 * 40, 37)


def test_run_staged_equals_stepped(ctx, events, stepped_1000):
    eng = _engine(ctx)
    eng.stage(events)
    eng.run_staged(0, len(events), 1000)
    assert np.array_equal(eng.output(), stepped_1000[0][-1])
    assert eng.topk_stats() == stepped_1000[1]
    eng.close()


def test_unstaged_step_equals_staged(ctx, events, stepped_1000):
    eng = _engine(ctx)
    for i in range(2):
        eng.step(events[i * 1000:(i + 1) * 1000])
        assert np.array_equal(eng.output(), stepped_1000[0][i])
    eng.close()


def test_topk_init_3(ctx, events, stepped_1000):
    outs, _ = _run_stepped(ctx, events, 5000, 1000, k=3)
    assert any(a.tobytes() != b.tobytes()
               for a, b in zip(outs, stepped_1000[0]))


def test_retractions_through_the_engine(ctx):
    """Event weights reach the operator: a top bid taken back is replaced by
    the next one below."""
    eng = _engine(ctx, k=2)
    eng.step(make_events(*[bid_event(7, 10 + p, bidder=p, price=100 * p)
                           for p in range(1, 6)]))
    assert zset(eng.output()) == {tm.q19_pack(7, 4, 400, 14): 1,
                                  tm.q19_pack(7, 5, 500, 15): 1}
    eng.step(make_events(bid_event(7, 15, bidder=5, price=500, w=-1)))
    assert zset(eng.output()) == {tm.q19_pack(7, 5, 500, 15): -1,
                                  tm.q19_pack(7, 3, 300, 13): 1}
    assert eng.topk_stats()["groups_refilled"] == 1
    eng.close()


def test_rejected_on_another_query_and_bad_k(ctx):
    from dbsp_amd.engine import Engine
    for q in (3, 102):
        other = Engine(ctx, query=q)
        with pytest.raises(RuntimeError):
            other.topk_init(5)
        with pytest.raises(RuntimeError):
            other.topk_stats()
        other.close()
    eng = _engine(ctx)
    for k in (0, 65537):
        with pytest.raises(RuntimeError):
            eng.topk_init(k)
    eng.close()


def test_world_2_is_rejected(ctx):
    from dbsp_amd.engine import Engine
    with pytest.raises(RuntimeError):
        Engine(ctx, query=19, rank=0, world=2)


@pytest.mark.parametrize("field", ["auction", "price", "bidder", "date_time"])
def test_field_overflow_is_an_error(ctx, field):
    eng = _engine(ctx)
    eng.step(make_events(bid_event(7, 100, bidder=2, price=5),
                         bid_event(7, 120, bidder=3, price=9),
                         bid_event(8, 110, bidder=4, price=3)))
    assert len(eng.output()) == 3
    stats = eng.topk_stats()
    good = dict(auction=7, dt=130, bidder=1, price=4)
    wide = {"auction": ("auction", 1 << 37), "price": ("price", 1 << 27),
            "bidder": ("bidder", 1 << 32), "date_time": ("dt", 1 << 32)}
    name, value = wide[field]
    bad = dict(good)
    bad[name] = value
    with pytest.raises(RuntimeError):
        eng.step(make_events(bid_event(8, 125, price=2), bid_event(**bad),
                             bid_event(9, 126, price=1)))
    assert eng.topk_stats() == stats
    assert len(eng.output()) == 0
    # the engine goes on as if the tick had not been sent; the widest values
    # that fit are accepted
    eng.step(make_events(bid_event((1 << 37) - 1, (1 << 32) - 1,
                                   bidder=(1 << 32) - 1,
                                   price=(1 << 27) - 1)))
    assert zset(eng.output()) == {((1 << 64) - 1, (1 << 64) - 1): 1}
    assert eng.topk_stats()["in_rows"] == stats["in_rows"] + 1
    eng.close()
