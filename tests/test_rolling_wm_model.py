"""The bounded rolling-aggregate model (tests/rolling_wm_model.py) against
the unbounded one (tests/rolling_model.py): truncating the integral below
watermark - (before + after) changes no tick's output as long as no row is
below the watermark."""
import pytest

from rolling_model import apply_delta, expected_delta
from rolling_wm_model import (BoundedModel, lower_bound,
                              quasi_monotone_stream, truncate)

RANGES = [(1000, 0), (500, 500), (0, 0), (3, 7)]


@pytest.mark.parametrize("before,after", RANGES)
def test_bounded_equals_unbounded_on_quasi_monotone_streams(before, after):
    m = BoundedModel(before, after)
    full = {}
    peak = 0
    for delta, wm in quasi_monotone_stream(before + after, 40, 60):
        assert all(ts >= wm for _, ts, _ in delta)
        assert m.step(delta, wm) == expected_delta(full, delta, before, after)
        full = apply_delta(full, delta)
        assert m.integral == truncate(full, m.lower_bound())
        peak = max(peak, len(m.integral))
    assert m.late_rows == 0
    assert m.wm > 10_000 and m.lower_bound() == m.wm - before - after
    assert peak < len(full) // 3, "the bound never bit"


def test_unique_stream_has_no_repeats():
    seen = set()
    for delta, _ in quasi_monotone_stream(3, 30, 50, unique=True):
        assert len(delta) == 50
        for p, ts, w in delta:
            assert w == 1 and (p, ts) not in seen
            seen.add((p, ts))


def test_late_rows_are_dropped_and_counted():
    m = BoundedModel(10, 0)
    assert m.step([(1, 100, 1), (1, 105, 2)], 100) == \
        expected_delta({}, [(1, 100, 1), (1, 105, 2)], 10, 0)
    before_integral = dict(m.integral)
    # 99 is late; 100 (== wm) is not; the pair at 50 cancels before the count
    out = m.step([(1, 99, 5), (1, 100, 1), (2, 50, 1), (2, 50, -1)], 0)
    assert out == expected_delta(before_integral, [(1, 100, 1)], 10, 0)
    assert (m.wm, m.late_rows) == (100, 1)
    # only late rows: nothing but the counter moves
    snap = dict(m.integral)
    assert m.step([(1, 3, 1), (2, 99, -1)], 7) == {}
    assert (m.wm, m.late_rows, m.integral) == (100, 3, snap)


def test_watermark_is_monotone():
    m = BoundedModel(5, 5)
    m.step([], 1000)
    m.step([], 10)
    assert (m.wm, m.lower_bound()) == (1000, 990)


def test_bound_saturates():
    assert lower_bound(500, 1000, 0) == 0           # wm < before + after
    assert lower_bound(1000, 600, 400) == 0
    assert lower_bound(1001, 600, 400) == 1
    assert lower_bound(1 << 32, 1 << 33, 0) == 0    # before = 2^33
    assert lower_bound((1 << 64) - 1, (1 << 64) - 1, 1) == 0    # overflow
    assert lower_bound((1 << 64) - 1, 1 << 33, 0) == (1 << 64) - 1 - (1 << 33)
    # nothing is ever truncated while the bound is 0
    for before, after in [(20_000, 0), (1 << 33, 0)]:
        m = BoundedModel(before, after)
        full = {}
        for delta, wm in quasi_monotone_stream(9, 8, 30):
            assert m.step(delta, wm) == \
                expected_delta(full, delta, before, after)
            full = apply_delta(full, delta)
        assert m.wm > 0 and m.lower_bound() == 0 and m.integral == full


def test_invalid_surviving_row_changes_nothing():
    m = BoundedModel(10, 0)
    m.step([(1, 100, 1)], 50)
    snap = (m.wm, m.late_rows, dict(m.integral))
    with pytest.raises(ValueError):
        m.step([(1, 1 << 32, 1), (1, 60, 1)], 70)
    assert (m.wm, m.late_rows, m.integral) == snap
    # an out-of-range partition below the watermark is simply late
    m.step([(1 << 40, 10, 1)], 70)
    assert (m.wm, m.late_rows) == (70, 1)
