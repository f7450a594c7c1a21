"""Watermark-bounded state of the rolling Max / Min on the GPU:
dbsp_truncate_below mode 2 (time = v >> 32) against a numpy mask, and
dbsp_rolling_step_wm / _compact / _wm_stats on Max and Min handles against
the FULL, never-truncated model of tests/rolling_minmax_model.py."""
import numpy as np
import pytest

from dbsp_amd import ROW_DT
from helpers import rows_of, zset
from rolling_minmax_model import AGGS, apply_delta, full_output, zset_diff
from rolling_wm_model import quasi_monotone_stream

pytestmark = pytest.mark.gpu

TMAX = (1 << 32) - 1
TILE = 2048             # rows per block of the truncation kernel
SWEEP_FLOOR = 4096


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
    """(p, ts, val, w) -> device rows (k = p, v = ts << 32 | val, w)."""
    return rows_of([(p, (int(ts) << 32) | int(val), w)
                    for p, ts, val, w in delta])


# ---- kernel parity ----

def _spine_rows(rng, n, tmax=1000):
    """n consolidated rows (p, ts << 32 | val, w) in many short partitions,
    times ascending inside each and sometimes repeated with another value.
    Returns the rows and their times."""
    rows = np.empty(n, dtype=ROW_DT)
    if n == 0:
        return rows, np.empty(0, dtype=np.uint64)
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.integers(1, 7)))
    lens[-1] -= sum(lens) - n
    p = np.repeat(np.arange(len(lens), dtype=np.uint64) * np.uint64(3), lens)
    ts = np.concatenate([np.sort(rng.choice(tmax, size=m, replace=True))
                         for m in lens]).astype(np.uint64)
    # ascending values keep rows of one (p, ts) distinct and in order
    val = np.arange(n, dtype=np.uint64) * np.uint64(1000) + \
        rng.integers(0, 1000, n).astype(np.uint64)
    rows["k"], rows["v"] = p, (ts << np.uint64(32)) | val
    rows["w"] = rng.integers(1, 4, n) * rng.choice([-1, 1], n)
    return rows, ts


def _with_last_time(rows, t):
    rows = rows.copy()
    rows["v"][-1] = (np.uint64(t) << np.uint64(32)) | \
        (rows["v"][-1] & np.uint64(TMAX))
    return rows


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1,
         5 * TILE + 1]


@pytest.mark.parametrize("n", SIZES)
def test_truncate_below_mode2_matches_mask(ctx, n):
    rng = np.random.default_rng(7 * n + 2)
    rows, ts = _spine_rows(rng, n)
    _assert_consolidated(rows)
    cases = [("bound 0", rows, 0, n),
             ("dead prefix in every partition", rows, 500, None),
             ("bound above every time", rows, 1000, 0),
             ("bound 2^32", rows, 1 << 32, 0),
             ("bound 2^64-1", rows, (1 << 64) - 1, 0)]
    if n:
        cases.append(("all kept", rows, int(ts.min()), n))
        cases.append(("none kept", rows, int(ts.max()) + 1, 0))
        r2 = _with_last_time(rows, 5000)
        cases.append(("only the last row", r2, 5000, 1))
        r3 = _with_last_time(rows, TMAX)
        cases.append(("bound 2^32-1", r3, TMAX, 1))
        cases.append(("bound 2^32, a row at 2^32-1", r3, TMAX + 1, 0))
    for name, r, bound, n_exp in cases:
        got = ctx.truncate_below(r, 2, bound)
        exp = r[(r["v"] >> np.uint64(32)) >= np.uint64(bound)]
        assert n_exp is None or len(exp) == n_exp, name
        assert got.tobytes() == exp.tobytes(), (name, n)
        _assert_consolidated(got)


def test_truncate_below_mode2_ignores_the_low_half(ctx):
    rows = rows_of([(1, (5 << 32) | TMAX, 1), (1, 6 << 32, -2),
                    (2, (4 << 32) | TMAX, 3), (2, (7 << 32) | 1, 1)])
    got = ctx.truncate_below(rows, 2, 6)
    assert got.tobytes() == rows[[1, 3]].tobytes()
    with pytest.raises(RuntimeError):
        ctx.truncate_below(rows, 3, 6)


# ---- operator against the FULL (never truncated) model integral ----

class FullModel:
    """Unbounded model.  R(I) of the previous tick is kept, so a tick's
    expected_delta = R(I + delta) - R(I) costs one full_output."""

    def __init__(self, before, after, agg):
        self.before, self.after, self.agg = before, after, agg
        self.integral, self.rel = {}, {}

    def step(self, delta):
        self.integral = apply_delta(self.integral, delta)
        rel = full_output(self.integral, self.before, self.after, self.agg)
        out = zset_diff(rel, self.rel)
        self.rel = rel
        return out


TICKS, ROWS = 120, 500


def _valued(stream, seed, vmax=20):
    """The (p, ts, w) stream with a value column: small values, so rows share
    (p, ts, val) and cancel, and the extreme is often retracted."""
    rng = np.random.default_rng(seed)
    return [([(p, ts, int(rng.integers(0, vmax)), w) for p, ts, w in delta], wm)
            for delta, wm in stream]


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("before,after", [(1000, 0), (500, 500), (0, 0),
                                          (3, 7)])
def test_bounded_equals_unbounded(ctx, before, after, agg):
    """The reference's quasi-monotone shape: two bounded operators (policy
    sweeps; compact() after every tick) must both output what the unbounded
    model does on its full integral."""
    stream = _valued(quasi_monotone_stream(11 + before + after, TICKS, ROWS),
                     before + after)
    full = FullModel(before, after, agg)
    lazy = ctx.rolling_create(before, after, agg=agg)
    eager = ctx.rolling_create(before, after, agg=agg)
    for i, (delta, wm) in enumerate(stream):
        exp = full.step(delta)
        for op in (lazy, eager):
            rows = op.step(dev_rows(delta), watermark=wm)
            _assert_consolidated(rows)
            assert zset(rows) == exp, f"tick {i}"
        eager.compact()
    wm, lb, late, sweeps = lazy.wm_stats()
    assert (wm, lb, late) == (stream[-1][1], stream[-1][1] - before - after, 0)
    assert sweeps >= 2
    assert eager.wm_stats()[3] >= 2 * TICKS
    assert lazy.stats()[0] < len(full.integral) // 4
    lazy.close()
    eager.close()


@pytest.mark.parametrize("agg", AGGS)
def test_state_bound(ctx, agg):
    """Rows that never repeat, weight +1, after = 0: trace rows are exact,
    and within 2 * live + 4096 + the rows since the last sweep."""
    before, after = 1000, 0
    stream = _valued(quasi_monotone_stream(5, TICKS, ROWS, unique=True), 5,
                     vmax=1 << 20)
    bounded = ctx.rolling_create(before, after, agg=agg)
    unbounded = ctx.rolling_create(before, after, agg=agg)
    all_ts = np.empty(0, dtype=np.int64)
    peak = 0
    for i, (delta, wm) in enumerate(stream):
        a = bounded.step(dev_rows(delta), watermark=wm)
        b = unbounded.step(dev_rows(delta))
        assert a.tobytes() == b.tobytes(), f"tick {i}"
        all_ts = np.concatenate([all_ts, np.array([r[1] for r in delta])])
        lb = max(wm - before - after, 0)
        assert bounded.wm_stats()[:2] == (wm, lb)
        live = int((all_ts >= lb).sum())
        in_rows, _, out_rows, _ = bounded.stats()
        print(f"tick {i}: live {live} in_rows {in_rows} out_rows {out_rows}")
        assert in_rows <= 2 * live + SWEEP_FLOOR + len(delta), f"tick {i}"
        assert out_rows <= 2 * live + SWEEP_FLOOR + len(delta), f"tick {i}"
        peak = max(peak, in_rows, out_rows)
    bounded.compact()
    in_rows, _, out_rows, _ = bounded.stats()
    assert (in_rows, out_rows) == (live, live)
    assert bounded.wm_stats()[2] == 0
    assert bounded.wm_stats()[3] >= 4
    u_in, _, u_out, _ = unbounded.stats()
    assert u_in == TICKS * ROWS == len(all_ts) and u_out >= TICKS * ROWS
    assert peak < u_in // 4
    # the compacted state still steps like the unbounded one
    delta = [(p, int(all_ts.max()) + 1 + p, 7, 1) for p in range(5)]
    assert bounded.step(dev_rows(delta), watermark=stream[-1][1]).tobytes() == \
        unbounded.step(dev_rows(delta)).tobytes()
    bounded.close()
    unbounded.close()


# ---- late rows, errors ----

class WmDriver:
    """Steps an operator next to a model that keeps the FULL integral of the
    rows that were not late: the outputs must not show the truncation."""

    def __init__(self, ctx, before, after, agg):
        self.op = ctx.rolling_create(before, after, agg=agg)
        self.model = FullModel(before, after, agg)
        self.wm, self.late = 0, 0

    def step(self, delta, watermark=None):
        rows = self.op.step(dev_rows(delta), watermark=watermark)
        _assert_consolidated(rows)
        self.wm = max(self.wm, watermark or 0)
        cons = [k + (w,) for k, w in apply_delta({}, delta).items()]
        kept = [r for r in cons if r[1] >= self.wm]
        self.late += len(cons) - len(kept)
        assert zset(rows) == self.model.step(kept)
        lb = max(self.wm - self.model.before - self.model.after, 0)
        assert self.op.wm_stats()[:3] == (self.wm, lb, self.late)
        return rows


@pytest.mark.parametrize("agg", AGGS)
def test_late_rows(ctx, agg):
    d = WmDriver(ctx, 10, 0, agg)
    d.step([(1, 100, 4, 1), (1, 105, 6, 2), (2, 101, 5, 1)], 100)
    # 99 and 40 are late by v >> 32 whatever their value, 100 (== wm) is not;
    # the pair at 50 cancels first
    out = d.step([(1, 99, TMAX, 5), (1, 100, 9, 1), (2, 50, 3, 1),
                  (2, 50, 3, -1), (3, 40, 0, -2), (2, 104, 1, 1)], 100)
    assert len(out) > 0
    assert d.op.wm_stats()[2] == 2
    stats, wms = d.op.stats(), d.op.wm_stats()
    # only late rows: empty output, nothing but late_rows moves
    assert len(d.step([(1, 3, 1, 1), (2, 99, TMAX, -1)], 7)) == 0
    assert d.op.stats() == stats
    assert d.op.wm_stats() == (wms[0], wms[1], wms[2] + 2, wms[3])
    # a smaller watermark does not lower wm
    d.step([(1, 100, 2, 1)], 50)
    assert d.op.wm_stats()[0] == 100
    # an empty step still advances it
    d.step([], 130)
    assert d.op.wm_stats()[:2] == (130, 120)
    d.step([(1, 129, TMAX, 1), (1, 130, 0, 1)], 0)
    assert d.op.wm_stats()[2] == wms[2] + 3
    d.op.close()


@pytest.mark.parametrize("agg", AGGS)
def test_error_atomicity(ctx, agg):
    d = WmDriver(ctx, 10, 5, agg)
    d.step([(1, 100, 1, 1), (2, 120, 8, 3)], 90)
    stats, wms = d.op.stats(), d.op.wm_stats()
    for bad in ([(1 << 32, 200, 1, 1), (1, 95, 1, 1)],  # 95 would be late at 99
                [(1 << 32, 200, 0, 1)],
                [(1, 150, 2, 1), (1 << 40, 160, 0, -1), (3, 170, 4, 1)]):
        with pytest.raises(RuntimeError):
            d.op.step(dev_rows(bad), watermark=99)
        assert d.op.stats() == stats
        assert d.op.wm_stats() == wms
    # a bad partition below the watermark is late, not an error
    d.step([(1 << 40, 10, 1, 1), (1, 99, 3, 1)], 99)
    assert d.op.wm_stats()[0] == 99 and d.op.wm_stats()[2] == wms[2] + 1
    d.op.close()


@pytest.mark.parametrize("agg", AGGS)
def test_compact_with_nothing_to_do(ctx, agg):
    op = ctx.rolling_create(5, 5, agg=agg)
    op.compact()                            # empty spines
    assert op.stats() == (0, 0, 0, 0)
    op.step(dev_rows([(1, 10, 3, 1), (1, 12, 4, 1)]), watermark=3)
    op.compact()                            # bound 0: everything stays
    assert op.stats() == (2, 1, 2, 1)
    op.step(dev_rows([]), watermark=1000)
    op.compact()                            # everything goes
    assert op.stats() == (0, 0, 0, 0)
    assert len(op.step(dev_rows([(1, 1000, 9, 2)]))) == 1
    op.close()
