"""numpy model of the watermark-bounded rolling aggregate
(dbsp_rolling_step_wm in include/dbsp_hip.h; reference
partitioned_rolling_aggregate_with_watermark, operator/time_series/
rolling_aggregate.rs:155-220), built on tests/rolling_model.py.

The model keeps a monotone watermark wm and, after every tick, ONLY the
integral rows with ts >= lb = sat_sub(wm, before + after); a tick's output is
rolling_model.expected_delta on that truncated integral.  Delta rows below
the (already raised) watermark are dropped and counted after the delta is
consolidated, as the operator does.

Also the stream generators the CPU and GPU tests share: the reference's
quasi-monotone shape (input_trace_quasi_monotone, rolling_aggregate.rs
:896-913: tick i draws its times from [i*step, i*step + window))."""
import numpy as np

from rolling_model import apply_delta, expected_delta

U64 = 1 << 64
T32 = 1 << 32


def lower_bound(wm, before, after):
    both = before + after
    if both >= U64:         # before + after overflows u64
        return 0
    return max(wm - both, 0)


def truncate(integral, lb):
    return {k: w for k, w in integral.items() if k[1] >= lb}


class BoundedModel:
    def __init__(self, before, after):
        self.before, self.after = before, after
        self.wm = 0
        self.late_rows = 0
        self.integral = {}      # rows with ts >= lower_bound() only

    def lower_bound(self):
        return lower_bound(self.wm, self.before, self.after)

    def step(self, delta, watermark=0):
        """One tick; returns the output Z-set.  ValueError, with nothing
        changed, if a surviving row has a partition or time >= 2^32."""
        wm = max(self.wm, int(watermark))
        cons = [(p, ts, w) for (p, ts), w in apply_delta({}, delta).items()]
        kept = [r for r in cons if r[1] >= wm]
        if any(p >= T32 or ts >= T32 for p, ts, _ in kept):
            raise ValueError("partition or time >= 2^32")
        out = expected_delta(self.integral, kept, self.before, self.after)
        self.integral = apply_delta(self.integral, kept)
        self.wm = wm
        self.late_rows += len(cons) - len(kept)
        self.integral = truncate(self.integral, self.lower_bound())
        return out


def quasi_monotone_stream(seed, ticks, rows_per_tick, partitions=5,
                          window=10_000, step=2_000, lateness=10_000,
                          unique=False):
    """[(delta, watermark)] per tick.  Tick i has times in
    [i*step, i*step + window); the watermark is the largest time seen so far,
    the tick's own rows included, minus the lateness (watermark_monotonic,
    watermark.rs:33-75), so with lateness >= window no row is ever late.

    unique=False: random partitions and times, weights in [-2, 3] (rows
    repeat and cancel).  unique=True: every weight +1 and no (p, ts) twice,
    ts = step*i + 5*u + (i mod 5) with u drawn without replacement per
    partition (needs 5 * step == window: ticks i and i+5 share a residue but
    not a time range)."""
    rng = np.random.default_rng(seed)
    out, tmax = [], 0
    for i in range(ticks):
        if unique:
            assert 5 * step == window
            delta = []
            for p in range(partitions):
                m = rows_per_tick // partitions
                u = rng.choice(window // 5, size=m, replace=False)
                delta += [(p, step * i + 5 * int(x) + i % 5, 1) for x in u]
        else:
            ps = rng.integers(0, partitions, rows_per_tick)
            ts = rng.integers(i * step, i * step + window, rows_per_tick)
            ws = rng.integers(-2, 4, rows_per_tick)
            delta = [(int(p), int(t), int(w)) for p, t, w in zip(ps, ts, ws)]
        if delta:
            tmax = max(tmax, max(r[1] for r in delta))
        out.append((delta, max(tmax - lateness, 0)))
    return out
