"""Rolling Max / Min on the GPU (dbsp_rolling_create_agg, dbsp_rolling_minmax)
against the numpy model of tests/rolling_minmax_model.py.

Per tick the operator's output delta must equal R(I_after) - R(I_before)
bit for bit, be consolidated (sorted by (k, v), distinct, no zero weights),
and the accumulated outputs must equal the from-scratch relation R(I)."""
import numpy as np
import pytest

from dbsp_amd import ROW_DT
from helpers import load_golden, zset
from rolling_minmax_model import (AGGS, apply_delta, expected_delta,
                                  full_output, rows_minmax, zset_diff)

pytestmark = pytest.mark.gpu

TMAX = (1 << 32) - 1
RANGES = [(1000, 0), (5, 5), (0, 0), (3, 7), (1 << 33, 0)]


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


def dev_rows(delta):
    """(p, ts, val, w) -> device rows (k = p, v = ts << 32 | val, w).  A
    partition is taken as it is (mod 2^64) so that invalid ones can be sent."""
    out = np.empty(len(delta), dtype=ROW_DT)
    mask = (1 << 64) - 1
    for i, (p, ts, val, w) in enumerate(delta):
        assert 0 <= ts <= TMAX and 0 <= val <= TMAX
        out[i] = (int(p) & mask, (int(ts) << 32) | int(val), w)
    return out


class Driver:
    """Steps an operator and the model side by side."""

    def __init__(self, ctx, before, after, agg):
        self.op = ctx.rolling_create(before, after, agg=agg)
        self.before, self.after, self.agg = before, after, agg
        self.integral, self.acc = {}, {}

    def step(self, delta):
        got_rows = self.op.step(dev_rows(delta))
        _assert_consolidated(got_rows)
        got = zset(got_rows)
        exp = expected_delta(self.integral, delta, self.before, self.after,
                             self.agg)
        assert got == exp, (
            f"tick delta of {len(delta)} rows: {len(got)} output rows vs "
            f"{len(exp)} expected")
        self.integral = apply_delta(self.integral, delta)
        self.acc = zset_diff(self.acc, {k: -w for k, w in got.items()})
        return got_rows

    def finish(self):
        assert self.acc == full_output(self.integral, self.before, self.after,
                                       self.agg)
        in_rows, _, out_rows, _ = self.op.stats()
        # spine rows are counted per batch, before cross-batch cancellation
        assert in_rows >= len(self.integral)
        assert out_rows >= len(self.acc)
        self.op.close()


def _extreme(agg, lo=0, hi=TMAX):
    return hi if agg == "max" else lo


@pytest.mark.parametrize("case", load_golden("rolling_minmax.json")["cases"],
                         ids=lambda c: c["name"])
def test_golden_cases(ctx, case):
    d = Driver(ctx, case["before"], case["after"], case["agg"])
    for step, exp in zip(case["steps"], case["expected"]):
        got = zset(d.step([tuple(r) for r in step]))
        assert got == {((p << 32) | ts, m): w for p, ts, m, w in exp}
    d.finish()


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("tmax", [1000, 10 ** 6])
@pytest.mark.parametrize("before,after", RANGES)
def test_reference_proptest_shapes(ctx, before, after, tmax, agg):
    """The shapes of the reference's proptests (rolling_aggregate.rs
    :864-960) with a value column: few partitions, small batches, weights
    that cancel, values below 20 so that several rows share a time and the
    extreme is often retracted."""
    rng = np.random.default_rng(tmax + before % 1013 + after)
    d = Driver(ctx, before, after, agg)
    for _ in range(20):
        n = int(rng.integers(0, 51))
        d.step([(int(rng.integers(0, 5)), int(rng.integers(0, tmax)),
                 int(rng.integers(0, 20)), int(rng.integers(-2, 4)))
                for _ in range(n)])
    d.finish()


# ---- the batch primitive ----

def _batch(rng, parts):
    """A consolidated batch: per (partition, n) of parts, n distinct rows whose
    times repeat (about two values per time) and whose values include 0 and
    2^32-1.  Returns ROW_DT rows sorted by (k, v)."""
    ks, vs = [], []
    for p, n in parts:
        v = set()
        while len(v) < n:
            m = n - len(v)
            ts = rng.integers(0, n // 2 + 2, m).astype(np.uint64)
            val = rng.choice(np.array([0, TMAX, 1, 77, 1 << 31], np.uint64), m)
            rnd = rng.integers(0, 1 << 32, m).astype(np.uint64)
            val = np.where(rng.integers(0, 3, m) == 0, val, rnd)
            v.update(((ts << np.uint64(32)) | val).tolist())
        v = np.sort(np.array(list(v), dtype=np.uint64))[:n]
        ks.append(np.full(n, p, dtype=np.uint64))
        vs.append(v)
    rows = np.empty(sum(n for _, n in parts), dtype=ROW_DT)
    rows["k"], rows["v"] = np.concatenate(ks), np.concatenate(vs)
    rows["w"] = rng.integers(1, 4, len(rows)) * rng.choice([-1, 1], len(rows))
    return rows


def _check_batch(ctx, rows, agg):
    _assert_consolidated(rows)
    ts, val = rows["v"] >> np.uint64(32), rows["v"] & np.uint64(TMAX)
    for before, after in [(10, 3), (0, 0), (1 << 32, 1 << 32)]:
        got = ctx.rolling_minmax(rows, agg, before, after)
        exp = rows.copy()
        exp["w"] = rows_minmax(rows["k"], ts, val, before, after,
                               agg).astype(np.int64)
        assert got.tobytes() == exp.tobytes(), (len(rows), before, after)


# the radix-16 tree's level boundaries
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097])
def test_rolling_minmax_one_partition(ctx, n, agg):
    _check_batch(ctx, _batch(np.random.default_rng(n), [(5, n)]), agg)


@pytest.mark.parametrize("agg", AGGS)
def test_rolling_minmax_three_partitions(ctx, agg):
    rng = np.random.default_rng(3)
    rows = _batch(rng, [(0, 300), (7, 17), ((1 << 40) + 1, 1000)])
    _check_batch(ctx, rows, agg)
    # the extreme of one partition must not leak into its neighbours
    mid = rows[rows["k"] == 7].copy()
    mid["v"] = (mid["v"] >> np.uint64(32) << np.uint64(32)) | np.uint64(500)
    mid = np.unique(mid["v"])
    rows = np.concatenate([rows[rows["k"] == 0],
                           np.array([(7, v, 1) for v in mid], dtype=ROW_DT),
                           rows[rows["k"] > 7]])
    got = ctx.rolling_minmax(rows, agg, 1 << 32, 1 << 32)
    assert (got["w"][got["k"] == 7] == 500).all()
    with pytest.raises(RuntimeError):
        ctx.rolling_minmax(rows, "sum", 1, 1)
    assert len(ctx.rolling_minmax(rows[:0], agg, 1, 1)) == 0


# ---- the operator ----

@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("n", [16, 17, 256, 257, 4096, 4097, 8192, 8193])
def test_slice_size_boundaries(ctx, n, agg):
    """One dense partition, deltas touching all of it: the gathered slice
    crosses the radix-16 tree levels and the fused-sort capacity.  Every 7th
    row holds the extreme of each range that reaches it (a range spans 14
    times), and the second delta retracts exactly those."""
    rng = np.random.default_rng(n)
    d = Driver(ctx, 10, 3, agg)
    mid = rng.integers(100, 200, n)
    peak = [1000 + t % 13 if agg == "max" else t % 13 for t in range(n)]
    val = [peak[t] if t % 7 == 0 else int(mid[t]) for t in range(n)]
    d.step([(9, t, val[t], 1) for t in range(n)])
    out = d.step([(9, t, val[t], -1) for t in range(0, n, 7)])
    assert len(out) > n        # every surviving time re-emits
    d.finish()


@pytest.mark.parametrize("agg", AGGS)
def test_one_time_with_many_values(ctx, agg):
    d = Driver(ctx, 4, 4, agg)
    hot = [(2, 50, 10 + 3 * i, 1 if i % 5 else -1) for i in range(3000)]
    # neighbours inside and outside the hot time's range [46, 54], their
    # values between the hot time's extremes (10 and 9007)
    near = [(2, 44, 5000, 1), (2, 47, 5001, 1), (2, 54, 5002, 2),
            (2, 55, 5003, 1), (3, 50, 1, 1)]
    out = d.step(hot + near)
    key = (2 << 32) | 50
    assert int((out["k"] == key).sum()) == 1
    top = max(r[2] for r in hot) if agg == "max" else min(r[2] for r in hot)
    # retract the hot time's extreme value, of either sign
    w = d.integral[(2, 50, top)]
    out = d.step([(2, 50, top, -w)])
    assert int(((out["k"] == key) & (out["w"] > 0)).sum()) == 1
    # ... and then everything positive at it: the time stops emitting
    out = d.step([(p, ts, v, -1) for (p, ts, v), w in d.integral.items()
                  if (p, ts) == (2, 50) and w > 0])
    assert int(((out["k"] == key) & (out["w"] > 0)).sum()) == 0
    assert int(((out["k"] == key) & (out["w"] < 0)).sum()) == 1
    d.finish()


@pytest.mark.parametrize("agg", AGGS)
def test_late_row_updates_later_aggregates(ctx, agg):
    d = Driver(ctx, 5000, 0, agg)
    first = d.step([(3, t, 1000 + t, 1) for t in range(3000)])
    assert len(first) == 3000
    late = d.step([(3, 0, _extreme(agg, 1, 10 ** 6), 1)])
    # every output retracts and re-emits with the late row's value
    assert len(late) == 6000
    assert int((late["w"] == -1).sum()) == 3000
    d.finish()


@pytest.mark.parametrize("agg", AGGS)
def test_multi_batch_spines(ctx, agg):
    rng = np.random.default_rng(6)
    d = Driver(ctx, 100, 20, agg)
    split = {0: 1, 2: -1, 4: 1}     # one row's weight across ticks
    peak = (0, 2500, _extreme(agg, 5, 5000))    # partition 0's extreme
    max_batches = 0
    for tick, n in enumerate([4000, 1500, 500, 150, 40, 10]):
        delta = [(int(rng.integers(0, 3)), int(rng.integers(0, 5000)),
                  int(rng.integers(100, 1000)), int(rng.integers(1, 4)))
                 for _ in range(n)]
        if tick in split:
            delta.append(peak + (split[tick],))
        d.step(delta)
        max_batches = max(max_batches, d.op.stats()[1])
    assert max_batches >= 3, "the cross-batch gather never ran"
    assert d.integral[peak] == 1
    d.finish()


@pytest.mark.parametrize("agg", AGGS)
def test_partition_edges(ctx, agg):
    p = (1 << 32) - 2
    lo, hi = (2, 9) if agg == "max" else (9, 2)
    d = Driver(ctx, TMAX, TMAX, agg)
    d.step([(p, 0, lo, 2), (p, TMAX, hi, 3)])
    d.step([(p + 1, 0, TMAX, 5), (p + 1, TMAX, 0, 7)])
    far = _extreme(agg)
    assert d.acc == {((p << 32), hi): 1, ((p << 32) | TMAX, hi): 1,
                     (((p + 1) << 32), far): 1,
                     (((p + 1) << 32) | TMAX, far): 1}
    before_stats = d.op.stats()
    for bad in ([(1 << 32, 5, 1, 1)],
                [(p, 1, 1, 1), (1 << 40, 0, 1, 1), (p + 1, 3, 1, 1)]):
        with pytest.raises(RuntimeError):
            d.op.step(dev_rows(bad))
        assert d.op.stats() == before_stats
    d.step([(p, 17, 4, 1), (p + 1, TMAX, 0, -7), (p + 1, 0, TMAX, -5),
            (p + 1, 9, 3, 1)])
    d.finish()
    z = Driver(ctx, 0, 0, agg)          # zero-width range at the clamps
    z.step([(0, 0, 1, 1), (0, 0, 8, 1), (0, TMAX, TMAX, 1), (p + 1, 0, 0, 1),
            (p + 1, TMAX, 6, 1)])
    z.step([(0, TMAX, TMAX, 1), (0, TMAX, 0, -1), (p + 1, 0, 0, -1),
            (0, 0, hi, -1)])
    z.finish()
