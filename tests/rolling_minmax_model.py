"""numpy model of the incremental partitioned rolling aggregate with the Max
and Min aggregators (reference partitioned_rolling_aggregate<TS, V, Agg>,
operator/time_series/rolling_aggregate.rs:235-321; semantics restated in
include/dbsp_hip.h at dbsp_roll_agg).

The reference's own rolling tests use a Fold sum only, so nothing here was
recorded from it: every rule is restated from the cited lines.

  rows      An integral is a dict {(partition, ts, val): weight} without zero
            weights; a delta is an iterable of (partition, ts, val, weight).
            On the device a row is (k = partition, v = ts << 32 | val, w).
  range     range_of(ts) = [sat_sub(ts, before), min(ts + after, 2^32 - 1)],
            closed (RelRange::range_of, time_series/range.rs:93-110).
  emit      A time (p, ts) emits iff some row of the integral at it has
            w > 0: eval walks the values of a time and breaks at the first
            `!weight.le0()` (rolling_aggregate.rs:572-592), so a time emits
            once however many values it holds, and never if all its rows are
            negative.
  value     M(p, ts) = the max (min) of val over the integral rows of
            partition p with time in range_of(ts) and ANY non-zero weight:
            Max::aggregate / Min::aggregate return the last / first value
            whose weight `!is_zero()` (aggregate/max.rs:36-55, min.rs:38-57);
            the tree's leaves are that aggregate per time
            (radix_tree/updater.rs:393) and inner nodes and range queries
            combine them with Agg::Semigroup (rolling_aggregate.rs:575-577).
            The range holds ts and an emitting time has a row, so M exists.
  output    R(I) = {(p << 32 | ts, M(p, ts)): +1} over the emitting times; a
            tick's output is R(I + delta) - R(I) (retractions plus
            insertions, rolling_aggregate.rs:601-603).

Outputs are Z-set dicts {(k, v): weight}, the form helpers.zset() gives for
engine rows."""
import numpy as np

TMAX = (1 << 32) - 1
AGGS = ("max", "min")


def apply_delta(integral, delta):
    """New integral = integral + delta (zero weights dropped)."""
    out = dict(integral)
    for p, ts, val, w in delta:
        key = (int(p), int(ts), int(val))
        nw = out.get(key, 0) + int(w)
        if nw:
            out[key] = nw
        else:
            out.pop(key, None)
    return out


def full_output(integral, before, after, agg):
    """R(I), vectorised: all partitions in one array sorted by
    (p << 32 | ts, val); a time's run and its range are searchsorted bounds
    over p << 32 | ts, M one ufunc.reduceat over the values."""
    assert agg in AGGS
    if not integral:
        return {}
    n = len(integral)
    cols = np.fromiter((x for k in integral for x in k), dtype=np.uint64,
                       count=3 * n).reshape(n, 3)
    w = np.fromiter(integral.values(), dtype=np.int64, count=n)
    order = np.lexsort((cols[:, 2], cols[:, 1], cols[:, 0]))
    p, ts, val = (cols[order, i] for i in range(3))
    w = w[order]
    key = (p << np.uint64(32)) | ts
    head = np.ones(n, dtype=bool)
    head[1:] = key[1:] != key[:-1]
    hi_ = np.flatnonzero(head)                  # first row of each time
    emits = np.maximum.reduceat((w > 0).astype(np.int8), hi_) > 0
    hp, hts, hkey = p[hi_], ts[hi_], key[hi_]
    b = np.uint64(min(int(before), TMAX))
    a = np.uint64(min(int(after), TMAX))
    lo = np.where(hts >= b, hts - b, np.uint64(0))
    hi = np.minimum(hts + a, np.uint64(TMAX))
    base = hp << np.uint64(32)
    i0 = np.searchsorted(key, base | lo, side="left")
    i1 = np.searchsorted(key, base | hi, side="right")
    assert (i0 < i1).all()                      # the range holds the time
    uf = np.maximum if agg == "max" else np.minimum
    # reduceat over [i0, i1) pairs: the even results; one pad so i1 = n indexes
    padded = np.concatenate([val, val[-1:]])
    pairs = np.stack([i0, i1], axis=1).ravel()
    m = uf.reduceat(padded, pairs)[::2]
    return {(int(k), int(x)): 1
            for k, x, e in zip(hkey.tolist(), m.tolist(), emits.tolist()) if e}


def rows_minmax(p, ts, val, before, after, agg):
    """The batch primitive (dbsp_rolling_minmax): for rows sorted by
    (p, ts, val), per row the extreme val over its partition's rows with time
    in range_of(ts), whatever the weights.  Arrays in, uint64 array out."""
    assert agg in AGGS
    p, ts, val = (np.asarray(x, dtype=np.uint64) for x in (p, ts, val))
    if len(p) == 0:
        return np.empty(0, dtype=np.uint64)
    b = np.uint64(min(int(before), TMAX))
    a = np.uint64(min(int(after), TMAX))
    lo = np.where(ts >= b, ts - b, np.uint64(0))
    hi = np.minimum(ts + a, np.uint64(TMAX))
    # partitions up to 2^64-1: rank them so that rank << 32 | ts fits
    rank = np.searchsorted(np.unique(p), p).astype(np.uint64)
    base = rank << np.uint64(32)
    key = base | ts
    i0 = np.searchsorted(key, base | lo, side="left")
    i1 = np.searchsorted(key, base | hi, side="right")
    uf = np.maximum if agg == "max" else np.minimum
    padded = np.concatenate([val, val[-1:]])
    return uf.reduceat(padded, np.stack([i0, i1], axis=1).ravel())[::2]


def zset_diff(a, b):
    """a - b over Z-set dicts."""
    d = dict(a)
    for k, w in b.items():
        nw = d.get(k, 0) - w
        if nw:
            d[k] = nw
        else:
            d.pop(k, None)
    return d


def expected_delta(before_integral, delta, before, after, agg):
    """One tick's output: R(I + delta) - R(I)."""
    after_integral = apply_delta(before_integral, delta)
    return zset_diff(full_output(after_integral, before, after, agg),
                     full_output(before_integral, before, after, agg))


def brute_output(integral, before, after, agg):
    """O(n^2) restatement of full_output in plain Python integers."""
    assert agg in AGGS
    pick = max if agg == "max" else min
    out = {}
    for (p, ts, _), w in integral.items():
        if w <= 0:
            continue
        lo = max(ts - before, 0)
        hi = min(ts + after, TMAX)
        m = pick(v2 for (p2, t2, v2), w2 in integral.items()
                 if p2 == p and lo <= t2 <= hi and w2 != 0)
        out[((p << 32) | ts, m)] = 1
    return out
