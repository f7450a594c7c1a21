"""Watermark-bounded state of the rolling aggregate on the GPU:
dbsp_truncate_below (the order-preserving spine truncation kernel) against a
numpy mask, and dbsp_rolling_step_wm / _compact / _wm_stats and engine query
101 with a lateness against the models of tests/rolling_model.py (unbounded,
FULL integral) and tests/rolling_wm_model.py (bounded)."""
import numpy as np
import pytest

from dbsp_amd import KIND_BID, ROW_DT, gen
from helpers import rows_of, zset
from rolling_model import apply_delta, full_output, zset_diff
from rolling_wm_model import BoundedModel, quasi_monotone_stream

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


# ---- kernel parity ----

def _spine_rows(rng, n, mode, tmax=1000):
    """n consolidated rows in many short partitions, times ascending inside
    each: mode 0 (p, ts, w), mode 1 (p<<32|ts, sum, w).  Returns the rows and
    their times."""
    rows = np.empty(n, dtype=ROW_DT)
    if n == 0:
        return rows, np.empty(0, dtype=np.uint64)
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.integers(1, 7)))
    lens[-1] -= sum(lens) - n
    p = np.repeat(np.arange(len(lens), dtype=np.uint64) * np.uint64(3), lens)
    ts = np.concatenate([np.sort(rng.choice(tmax, size=m, replace=False))
                         for m in lens]).astype(np.uint64)
    w = rng.integers(1, 4, n) * rng.choice([-1, 1], n)
    if mode == 0:
        rows["k"], rows["v"] = p, ts
    else:
        rows["k"] = (p << np.uint64(32)) | ts
        rows["v"] = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2)
    rows["w"] = w
    return rows, ts


def _with_last_time(rows, mode, t):
    rows = rows.copy()
    if mode == 0:
        rows["v"][-1] = t
    else:
        rows["k"][-1] = (rows["k"][-1] >> np.uint64(32) << np.uint64(32)) \
            | np.uint64(t)
    return rows


# below / at / above one tile, several tiles plus one row; the kernel runs one
# block per tile and does not grid-stride, so there is no grid cap to pass
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1,
         5 * TILE + 1]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_truncate_below_matches_mask(ctx, n, mode):
    rng = np.random.default_rng(7 * n + mode)
    rows, ts = _spine_rows(rng, n, mode)
    _assert_consolidated(rows)
    cases = [("bound 0", rows, 0, n),
             ("dead prefix in every partition", rows, 500, None),
             ("bound above every time", rows, 1000, 0),
             ("bound 2^64-1", rows, (1 << 64) - 1, 0)]
    if n:
        cases.append(("all kept", rows, int(ts.min()), n))
        cases.append(("none kept", rows, int(ts.max()) + 1, 0))
        r2 = _with_last_time(rows, mode, 5000)
        cases.append(("only the last row", r2, 5000, 1))
        r3 = _with_last_time(rows, mode, TMAX)
        cases.append(("bound 2^32-1", r3, TMAX, 1))
        cases.append(("bound 2^32", r3, TMAX + 1, 0))
    for name, r, bound, n_exp in cases:
        got = ctx.truncate_below(r, mode, bound)
        t = r["v"] if mode == 0 else r["k"] & np.uint64(TMAX)
        exp = r[t >= np.uint64(bound)]
        assert n_exp is None or len(exp) == n_exp, name
        assert got.tobytes() == exp.tobytes(), (name, n, mode)
        _assert_consolidated(got)


def test_truncate_below_mode0_compares_the_whole_value(ctx):
    rows = rows_of([(1, 5, 1), (1, 1 << 40, -2), (2, (1 << 32) + 1, 3)])
    got = ctx.truncate_below(rows, 0, 1 << 33)
    assert got.tobytes() == rows[1:2].tobytes()
    # mode 1 looks at the low 32 bits of the key only
    rows = rows_of([((7 << 32) | 4, 9, 1), ((7 << 32) | 6, 9, -1),
                    ((9 << 32) | 5, 0, 2)])
    got = ctx.truncate_below(rows, 1, 5)
    assert got.tobytes() == rows[1:].tobytes()


# ---- operator against the FULL (never truncated) model integral ----

class FullModel:
    """Unbounded model.  R(I) of the previous tick is kept, so a tick's
    expected_delta = R(I + delta) - R(I) costs one full_output."""

    def __init__(self, before, after):
        self.before, self.after = before, after
        self.integral, self.rel = {}, {}

    def step(self, delta):
        self.integral = apply_delta(self.integral, delta)
        rel = full_output(self.integral, self.before, self.after)
        out = zset_diff(rel, self.rel)
        self.rel = rel
        return out


TICKS, ROWS = 120, 500


@pytest.mark.parametrize("before,after", [(1000, 0), (500, 500), (0, 0),
                                          (3, 7)])
def test_bounded_equals_unbounded(ctx, before, after):
    """The reference's quasi-monotone shape: two bounded operators (policy
    sweeps; compact() after every tick) must both output what the unbounded
    model does on its full integral."""
    stream = quasi_monotone_stream(11 + before + after, TICKS, ROWS)
    full = FullModel(before, after)
    lazy = ctx.rolling_create(before, after)
    eager = ctx.rolling_create(before, after)
    for i, (delta, wm) in enumerate(stream):
        exp = full.step(delta)
        for op in (lazy, eager):
            rows = op.step(rows_of(delta), watermark=wm)
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


def test_state_bound(ctx):
    """Rows that never repeat, weight +1, after = 0: trace rows are exact."""
    before, after = 1000, 0
    stream = quasi_monotone_stream(5, TICKS, ROWS, unique=True)
    bounded = ctx.rolling_create(before, after)
    unbounded = ctx.rolling_create(before, after)
    all_ts = np.empty(0, dtype=np.int64)
    peak = 0
    for i, (delta, wm) in enumerate(stream):
        a = bounded.step(rows_of(delta), watermark=wm)
        b = unbounded.step(rows_of(delta))
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
    in_rows, in_b, out_rows, out_b = bounded.stats()
    assert (in_rows, out_rows) == (live, live)
    assert bounded.wm_stats()[2] == 0
    assert bounded.wm_stats()[3] >= 4
    u_in, _, u_out, _ = unbounded.stats()
    assert u_in == TICKS * ROWS == len(all_ts) and u_out >= TICKS * ROWS
    assert peak < u_in // 4
    # the compacted state still steps like the unbounded one
    delta, wm = [(p, int(all_ts.max()) + 1 + p, 1) for p in range(5)], stream[-1][1]
    assert bounded.step(rows_of(delta), watermark=wm).tobytes() == \
        unbounded.step(rows_of(delta)).tobytes()
    bounded.close()
    unbounded.close()


# ---- late rows, errors, mixed calls ----

class WmDriver:
    """Steps an operator and the bounded model side by side."""

    def __init__(self, ctx, before, after):
        self.op = ctx.rolling_create(before, after)
        self.model = BoundedModel(before, after)

    def step(self, delta, watermark=None):
        rows = self.op.step(rows_of(delta), watermark=watermark)
        _assert_consolidated(rows)
        exp = self.model.step(delta, watermark or 0)
        assert zset(rows) == exp
        wm, lb, late, _ = self.op.wm_stats()
        assert (wm, lb, late) == (self.model.wm, self.model.lower_bound(),
                                  self.model.late_rows)
        return rows


def test_late_rows(ctx):
    d = WmDriver(ctx, 10, 0)
    d.step([(1, 100, 1), (1, 105, 2), (2, 101, 1)], 100)
    # 99 and 40 are late, 100 (== wm) is not; the pair at 50 cancels first
    out = d.step([(1, 99, 5), (1, 100, 1), (2, 50, 1), (2, 50, -1),
                  (3, 40, -2), (2, 104, 1)], 100)
    assert len(out) > 0
    assert d.op.wm_stats()[2] == 2
    stats, wms = d.op.stats(), d.op.wm_stats()
    # only late rows: empty output, nothing but late_rows moves
    assert len(d.step([(1, 3, 1), (2, 99, -1)], 7)) == 0
    assert d.op.stats() == stats
    assert d.op.wm_stats() == (wms[0], wms[1], wms[2] + 2, wms[3])
    # a smaller watermark does not lower wm
    d.step([(1, 100, 1)], 50)
    assert d.op.wm_stats()[0] == 100
    # an empty step still advances it
    d.step([], 130)
    assert d.op.wm_stats()[:2] == (130, 120)
    d.step([(1, 129, 1), (1, 130, 1)], 0)
    assert d.op.wm_stats()[2] == wms[2] + 3
    d.op.close()


def test_error_atomicity(ctx):
    d = WmDriver(ctx, 10, 5)
    d.step([(1, 100, 1), (2, 120, 3)], 90)
    stats, wms = d.op.stats(), d.op.wm_stats()
    for bad in ([(1, 1 << 32, 1), (1, 95, 1)],      # 95 would be late at 99
                [(1 << 32, 200, 1)],
                [(1, 150, 1), (3, 1 << 40, -1)]):
        with pytest.raises(RuntimeError):
            d.op.step(rows_of(bad), watermark=99)
        assert d.op.stats() == stats
        assert d.op.wm_stats() == wms
    # a bad partition below the watermark is late, not an error
    d.step([(1 << 40, 10, 1), (1, 99, 1)], 99)
    assert d.op.wm_stats()[0] == 99 and d.op.wm_stats()[2] == wms[2] + 1
    d.op.close()


def test_plain_step_is_step_wm_zero(ctx):
    a = WmDriver(ctx, 20, 3)
    b = WmDriver(ctx, 20, 3)
    ticks = [([(1, 50, 1), (2, 60, 2)], 50), ([(1, 49, 1), (1, 70, 1)], None),
             ([(2, 80, -1), (2, 10, 4)], 65), ([(1, 64, 1), (2, 66, 1)], None),
             ([], None), ([(1, 90, 2)], 0)]
    for delta, wm in ticks:
        ra = a.step(delta, wm)                          # plain step on None
        rb = b.step(delta, 0 if wm is None else wm)
        assert ra.tobytes() == rb.tobytes()
        assert a.op.wm_stats() == b.op.wm_stats()
        assert a.op.stats() == b.op.stats()
    assert a.op.wm_stats()[2] == 3
    a.op.close()
    b.op.close()


def test_compact_with_nothing_to_do(ctx):
    op = ctx.rolling_create(5, 5)
    op.compact()                            # empty spines
    assert op.stats() == (0, 0, 0, 0)
    op.step(rows_of([(1, 10, 1), (1, 12, 1)]), watermark=3)
    op.compact()                            # bound 0: everything stays
    assert op.stats() == (2, 1, 2, 1)
    op.step(rows_of([]), watermark=1000)
    op.compact()                            # everything goes
    assert op.stats() == (0, 0, 0, 0)
    assert len(op.step(rows_of([(1, 1000, 2)]))) == 1
    op.close()


# ---- engine query 101 ----

def test_engine_query_101_lateness(ctx):
    from dbsp_amd.engine import Engine
    n_events, tick, before, lateness = 20000, 1000, 50, 150
    events = gen.generate(n_events, rate=10_000.0)
    bt = events["f3"][events["kind"] == KIND_BID].astype(np.int64)
    assert (np.diff(bt) >= 0).all(), "bid times are not monotone"
    for lo in range(0, n_events, tick):     # nothing can be late
        e = events[lo:lo + tick]
        t = e["f3"][e["kind"] == KIND_BID].astype(np.int64)
        assert t.max() - t.min() <= lateness
    assert bt.max() - bt.min() > 4 * (lateness + before)

    def run(with_lateness):
        eng = Engine(ctx, query=101)
        eng.rolling_init(before, 0)
        if with_lateness:
            eng.rolling_lateness(lateness)
        eng.stage(events)
        outs = []
        for lo in range(0, n_events, tick):
            eng.step_staged(lo, lo + tick)
            outs.append(eng.output())
        with pytest.raises(RuntimeError):
            eng.rolling_lateness(lateness)      # rejected after stepping
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

    q3 = Engine(ctx, query=3)
    with pytest.raises(RuntimeError):
        q3.rolling_lateness(1)      # another query
    with pytest.raises(RuntimeError):
        q3.rolling_stats()
    q3.close()
