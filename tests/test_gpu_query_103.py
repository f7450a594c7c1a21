"""Engine query 103 on the GPU: auctions nobody has bid on yet,
auctions.map_index(|a| (a.id, a.seller)).antijoin(&bids.map_index(|b|
(b.auction, ()))), against the dict model of tests/antijoin_model.py fed
(f0, f1, w) of the auction events and f0 of the bid events."""
import pytest

import antijoin_model as am
from dbsp_amd import gen
from helpers import auction_event, bid_event, events as make_events, zset

pytestmark = pytest.mark.gpu


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


def _run_stepped(ctx, events, n_events, tick):
    """Staged ticks next to the model; returns (flips, rows gathered, rows
    filtered, auctions still unbid at the end)."""
    from dbsp_amd.engine import Engine
    eng = Engine(ctx, query=103)
    eng.stage(events)
    model = am.Model(am.ANTIJOIN)
    tot = [0, 0, 0]
    for lo in range(0, n_events, tick):
        hi = min(lo + tick, n_events)
        eng.step_staged(lo, hi)
        rows = eng.output()
        _assert_consolidated(rows)
        exp, nf, ng, nd = model.step(*am.q103_deltas(events[lo:hi]))
        assert zset(rows) == exp, f"tick [{lo},{hi})"
        tot = [tot[0] + nf, tot[1] + ng, tot[2] + nd]
    st = eng.antijoin_stats()
    eng.close()
    assert [st["keys_flipped"], st["rows_gathered"],
            st["rows_filtered"]] == tot
    assert st["a_rows"] == len(model.integral_a)
    assert model.acc == am.full_output(model.integral_a, model.integral_b,
                                       am.ANTIJOIN)
    return (*tot, len(model.acc))


def test_ticks_of_1000(ctx, events):
    figures = _run_stepped(ctx, events, len(events), 1000)
    # a build that never gathers or never filters cannot pass
    assert all(f > 0 for f in figures), figures


def test_ticks_of_37(ctx, events):
    figures = _run_stepped(ctx, events, 37 * 40, 37)
    assert all(f > 0 for f in figures), figures


def test_run_staged_counts_as_stepped(ctx, events):
    from dbsp_amd.engine import Engine
    model = am.Model(am.ANTIJOIN)
    tot = [0, 0, 0]
    for lo in range(0, 5000, 1000):
        exp, nf, ng, nd = model.step(*am.q103_deltas(events[lo:lo + 1000]))
        tot = [tot[0] + nf, tot[1] + ng, tot[2] + nd]
    eng = Engine(ctx, query=103)
    eng.stage(events)
    eng.run_staged(0, 5000, 1000)
    assert zset(eng.output()) == exp
    st = eng.antijoin_stats()
    assert [st["keys_flipped"], st["rows_gathered"],
            st["rows_filtered"]] == tot
    eng.close()


def test_unstaged_step_equals_the_model(ctx, events):
    from dbsp_amd.engine import Engine
    eng = Engine(ctx, query=103)
    model = am.Model(am.ANTIJOIN)
    for i in range(2):
        ev = events[i * 1000:(i + 1) * 1000]
        eng.step(ev)
        assert zset(eng.output()) == model.step(*am.q103_deltas(ev))[0]
    eng.close()


def test_two_auctions_a_bid_and_its_retraction(ctx):
    from dbsp_amd.engine import Engine
    eng = Engine(ctx, query=103)
    eng.step(make_events(auction_event(10, 501, 3), auction_event(11, 502, 3)))
    assert zset(eng.output()) == {(10, 501): 1, (11, 502): 1}
    eng.step(make_events(bid_event(10, 5, bidder=9, price=100)))
    assert zset(eng.output()) == {(10, 501): -1}
    eng.step(make_events(bid_event(10, 5, bidder=9, price=100, w=-1)))
    assert zset(eng.output()) == {(10, 501): 1}
    st = eng.antijoin_stats()
    assert (st["keys_flipped"], st["rows_gathered"],
            st["rows_filtered"]) == (2, 2, 0)
    assert st["a_rows"] == 2
    # an auction arriving with its first bid is never shown
    eng.step(make_events(auction_event(12, 503, 1),
                         bid_event(12, 6, bidder=9, price=100)))
    assert len(eng.output()) == 0
    assert eng.antijoin_stats()["rows_filtered"] == 1
    eng.close()


def test_stats_rejected_on_another_query(ctx):
    from dbsp_amd.engine import Engine
    other = Engine(ctx, query=3)
    with pytest.raises(RuntimeError):
        other.antijoin_stats()
    other.close()


def test_world_2_is_rejected(ctx):
    from dbsp_amd.engine import Engine
    with pytest.raises(RuntimeError):
        Engine(ctx, query=103, rank=0, world=2)
