"""Incremental partitioned rolling aggregate on the GPU (dbsp_rolling_*,
engine query 101) against the numpy model of tests/rolling_model.py.

Per tick the operator's output delta must equal R(I_after) - R(I_before)
bit for bit, be consolidated (sorted by (k, v), distinct, no zero weights),
and the accumulated outputs must equal the from-scratch relation R(I)."""
import numpy as np
import pytest

from dbsp_amd import KIND_BID, gen
from helpers import load_golden, rows_of, zset
from rolling_model import apply_delta, expected_delta, full_output, zset_diff

pytestmark = pytest.mark.gpu

TMAX = (1 << 32) - 1


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


def _assert_consolidated(rows):
    if len(rows) == 0:
        return
    assert (rows["w"] != 0).all()
    k, v = rows["k"], rows["v"]
    inc = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1]))
    assert inc.all(), "output not sorted by (k, v) / not distinct"


class Driver:
    """Steps an operator and the model side by side."""

    def __init__(self, ctx, before, after):
        self.op = ctx.rolling_create(before, after)
        self.before, self.after = before, after
        self.integral, self.acc = {}, {}

    def step(self, delta):
        got_rows = self.op.step(rows_of(delta))
        _assert_consolidated(got_rows)
        got = zset(got_rows)
        exp = expected_delta(self.integral, delta, self.before, self.after)
        assert got == exp, (
            f"tick delta of {len(delta)} rows: {len(got)} output rows vs "
            f"{len(exp)} expected")
        self.integral = apply_delta(self.integral, delta)
        self.acc = zset_diff(self.acc, {k: -w for k, w in got.items()})
        return got_rows

    def finish(self):
        assert self.acc == full_output(self.integral, self.before, self.after)
        in_rows, _, out_rows, _ = self.op.stats()
        # spine rows are counted per batch, before cross-batch cancellation
        assert in_rows >= len(self.integral)
        assert out_rows >= len(self.acc)
        self.op.close()


@pytest.mark.parametrize("before,after", [(1000, 0), (500, 500)])
def test_golden_vectors(ctx, before, after):
    g = load_golden("rolling_over_range.json")
    for case in g["cases"]:
        d = Driver(ctx, before, after)
        for step in case["steps"]:
            d.step([tuple(r) for r in step])
        exp = {((p << 32) | ts, s): 1
               for p, ts, s in case["expected"][f"{before},{after}"]}
        assert d.acc == exp, case["name"]
        d.finish()


@pytest.mark.parametrize("tmax", [1000, 10 ** 6])
@pytest.mark.parametrize("before,after", [(1000, 0), (500, 500), (0, 0),
                                          (3, 7), (1 << 33, 0)])
def test_reference_proptest_shapes(ctx, before, after, tmax):
    """The shapes of the reference's proptests (rolling_aggregate.rs
    :864-960): few partitions, small batches, weights that cancel."""
    rng = np.random.default_rng(tmax + before % 1013 + after)
    d = Driver(ctx, before, after)
    for _ in range(20):
        n = int(rng.integers(0, 51))
        d.step([(int(rng.integers(0, 5)), int(rng.integers(0, tmax)),
                 int(rng.integers(-2, 4))) for _ in range(n)])
    d.finish()


def test_late_row_updates_later_aggregates(ctx):
    d = Driver(ctx, 5000, 0)
    first = d.step([(3, t, 1) for t in range(3000)])
    assert len(first) == 3000
    late = d.step([(3, 0, 1)])
    # every output retracts and re-emits with its sum raised by one
    assert len(late) == 6000
    assert int((late["w"] == -1).sum()) == 3000
    d.finish()


@pytest.mark.parametrize("n", [16, 17, 256, 257, 4096, 4097, 8192, 8193])
def test_slice_size_boundaries(ctx, n):
    """One dense partition, deltas touching all of it: the gathered slice
    crosses the radix-16 tree levels and the fused-sort capacity."""
    rng = np.random.default_rng(n)
    d = Driver(ctx, 10, 3)
    w = rng.integers(1, 4, n)
    d.step([(9, t, int(w[t])) for t in range(n)])
    d.step([(9, t, 1) for t in range(0, n, 7)])
    d.finish()


def test_row_life_cycle(ctx):
    d = Driver(ctx, 10, 10)
    d.step([(1, 45, 5), (1, 55, 7), (2, 50, 1)])
    d.step([(1, 50, 1)])
    gone = d.step([(1, 50, -1)])
    assert ((1 << 32) | 50) in set(gone["k"][gone["w"] < 0].tolist())
    assert ((1 << 32) | 50) not in set(gone["k"][gone["w"] > 0].tolist())
    neg = d.step([(1, 50, -1)])     # weight -1: no row of its own ...
    assert ((1 << 32) | 50) not in set(neg["k"].tolist())
    assert len(neg) == 4            # ... but both neighbours' sums drop
    d.step([(1, 50, 2)])
    assert len(d.step([])) == 0
    d.step([(2, 58, 4)])
    d.step([(1, 45, 1), (1, 45, -1)])   # cancels inside the delta
    d.finish()


def test_multi_batch_spines(ctx):
    rng = np.random.default_rng(6)
    d = Driver(ctx, 100, 20)
    split = {0: 1, 2: -1, 4: 1}     # one row's weight across ticks
    max_batches = 0
    for tick, n in enumerate([4000, 1500, 500, 150, 40, 10]):
        delta = [(int(rng.integers(0, 3)), int(rng.integers(0, 5000)),
                  int(rng.integers(1, 4))) for _ in range(n)]
        if tick in split:
            delta.append((0, 7777, split[tick]))
        d.step(delta)
        max_batches = max(max_batches, d.op.stats()[1])
    assert max_batches >= 3, "the cross-batch gather never ran"
    assert d.integral[(0, 7777)] == 1
    d.finish()


def test_partition_edges(ctx):
    p = (1 << 32) - 2
    d = Driver(ctx, TMAX, TMAX)
    d.step([(p, 0, 2), (p, TMAX, 3)])
    d.step([(p + 1, 0, 5), (p + 1, TMAX, 7)])
    assert d.acc == {((p << 32), 5): 1, ((p << 32) | TMAX, 5): 1,
                     (((p + 1) << 32), 12): 1, (((p + 1) << 32) | TMAX, 12): 1}
    before_stats = d.op.stats()
    for bad in ([(1 << 32, 5, 1)], [(p, 1 << 32, 1)],
                [(p, 1, 1), (1 << 40, 0, 1), (p + 1, 3, 1)]):
        with pytest.raises(RuntimeError):
            d.op.step(rows_of(bad))
        assert d.op.stats() == before_stats
    d.step([(p, 17, 1), (p + 1, TMAX, -7)])
    d.finish()
    z = Driver(ctx, 0, 0)               # zero-width range at the clamps
    z.step([(0, 0, 1), (0, TMAX, 1), (p + 1, 0, 1), (p + 1, TMAX, 1)])
    z.step([(0, TMAX, 1), (p + 1, 0, -1)])
    z.finish()


def _bid_delta(events):
    b = events[events["kind"] == KIND_BID]
    return [(int(a), int(t), int(w) * int(pr))
            for a, t, w, pr in zip(b["f0"], b["f3"], b["w"], b["f2"])]


def test_engine_query_101(ctx):
    from dbsp_amd.engine import Engine
    events = gen.generate(20000, rate=100_000.0)
    assert int(events["f3"][events["kind"] == KIND_BID].max()) - \
        int(events["f3"][events["kind"] == KIND_BID].min()) > 50
    before, after = 50, 0

    def run(n_events, tick):
        eng = Engine(ctx, query=101)
        eng.rolling_init(before, after)
        eng.stage(events)
        integral, acc, outs = {}, {}, []
        for lo in range(0, n_events, tick):
            hi = min(lo + tick, n_events)
            eng.step_staged(lo, hi)
            rows = eng.output()
            _assert_consolidated(rows)
            got = zset(rows)
            delta = _bid_delta(events[lo:hi])
            assert got == expected_delta(integral, delta, before, after), \
                f"tick [{lo},{hi})"
            integral = apply_delta(integral, delta)
            acc = zset_diff(acc, {k: -w for k, w in got.items()})
            outs.append(rows)
        assert acc == full_output(integral, before, after)
        with pytest.raises(RuntimeError):
            eng.rolling_init(before, after)     # rejected after stepping
        eng.close()
        return outs

    outs = run(len(events), 1000)
    assert sum(len(o) for o in outs) > 0
    run(37 * 40, 37)

    eng = Engine(ctx, query=101)
    eng.rolling_init(before, after)
    eng.stage(events)
    eng.run_staged(0, len(events), 1000)
    assert np.array_equal(eng.output(), outs[-1])
    eng.close()

    eng = Engine(ctx, query=101)        # unstaged ticks take the same path
    eng.rolling_init(before, after)
    for i in range(2):
        eng.step(events[i * 1000:(i + 1) * 1000])
        assert np.array_equal(eng.output(), outs[i])
    eng.close()

    eng = Engine(ctx, query=101)        # default range: 10000 ms before, 0 after
    eng.stage(events)
    eng.step_staged(0, 3000)
    assert zset(eng.output()) == expected_delta(
        {}, _bid_delta(events[:3000]), 10000, 0)
    eng.close()

    q3 = Engine(ctx, query=3)
    with pytest.raises(RuntimeError):
        q3.rolling_init(1, 1)       # another query
    q3.close()
