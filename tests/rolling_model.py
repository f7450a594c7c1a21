"""numpy model of the incremental partitioned rolling aggregate (linear
weight-sum aggregator; reference operator/time_series/rolling_aggregate.rs
:487-604, semantics restated in include/dbsp_hip.h at dbsp_rolling_step).

An integral is a dict {(partition, ts): weight} without zero weights; a
delta is an iterable of (partition, ts, weight) triples.  Outputs are Z-set
dicts {(partition<<32 | ts, sum as u64 bits): weight}, the form
helpers.zset() gives for engine rows.

The model keeps all partitions in one array sorted by partition<<32 | ts,
takes the cumulative weight sum and finds each row's range ends with two
searchsorted calls."""
import numpy as np

TMAX = (1 << 32) - 1
MASK64 = (1 << 64) - 1


def apply_delta(integral, delta):
    """New integral = integral + delta (zero weights dropped)."""
    out = dict(integral)
    for p, ts, w in delta:
        key = (int(p), int(ts))
        nw = out.get(key, 0) + int(w)
        if nw:
            out[key] = nw
        else:
            out.pop(key, None)
    return out


def full_output(integral, before, after):
    """R(I): {(p<<32|ts, S(p, ts)): 1 for every (p, ts) with I[p, ts] > 0},
    S = sum of I over partition p and times in [ts - before, ts + after]
    (saturating at 0 and 2^32-1)."""
    if not integral:
        return {}
    items = sorted(integral.items())
    p = np.array([k[0] for k, _ in items], dtype=np.uint64)
    ts = np.array([k[1] for k, _ in items], dtype=np.uint64)
    w = np.array([v for _, v in items], dtype=np.int64)
    b = np.uint64(min(int(before), TMAX))
    a = np.uint64(min(int(after), TMAX))
    lo = np.where(ts >= b, ts - b, np.uint64(0))
    hi = np.minimum(ts + a, np.uint64(TMAX))
    base = p << np.uint64(32)
    key = base | ts
    cum = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(w)])
    i0 = np.searchsorted(key, base | lo, side="left")
    i1 = np.searchsorted(key, base | hi, side="right")
    sums = cum[i1] - cum[i0]
    out = {}
    for kk, s, ww in zip(key.tolist(), sums.tolist(), w.tolist()):
        if ww > 0:
            out[(kk, s & MASK64)] = 1
    return out


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


def expected_delta(before_integral, delta, before, after):
    """One tick's output: R(I + delta) - R(I)."""
    after_integral = apply_delta(before_integral, delta)
    return zset_diff(full_output(after_integral, before, after),
                     full_output(before_integral, before, after))


def brute_output(integral, before, after):
    """O(n^2) restatement of full_output in plain Python integers."""
    out = {}
    for (p, ts), w in integral.items():
        if w <= 0:
            continue
        lo = max(ts - before, 0)
        hi = min(ts + after, TMAX)
        s = sum(w2 for (p2, t2), w2 in integral.items()
                if p2 == p and lo <= t2 <= hi)
        out[((p << 32) | ts, s & MASK64)] = 1
    return out
