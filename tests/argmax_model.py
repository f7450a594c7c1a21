"""Dict model of the incremental arg-max per group operator with ties
(dbsp_argmax_op in include/dbsp_hip.h) and a pure-Python restatement of the
reference's Nexmark q7 on it (crates/nexmark/src/queries/q7.rs:45-94).

Every rule is restated from the cited lines; nothing is executed from the
reference.

  rows      An integral is a dict {(k, v): weight} without zero weights; a
            delta is an iterable of (k, v, w).  k and v are 64-bit unsigned.
  group     g = k >> group_shift; rank = k >> rank_shift with rank_shift <=
            group_shift, so the rank includes the group bits, equal ranks
            imply the same group and (k, v) order is (group, rank, tie) order.
            q7 has the unit key () as its only group (q7.rs:88) and the price
            as the rank (q7.rs:82-93).
  presence  A row is present iff its total weight is non-zero, negative
            totals included: the rule of the top-K operator
            (aggregate/fold.rs:83-92), applied per row.
  relation  R(I): for every group with a present row, all present rows whose
            rank is the group's largest present rank, each at its own
            integral weight.  q7.rs:90-93 computes the largest price with
            aggregate(Min) over the negated price and joins it back to
            bids_by_price; the join multiplies the maximum's weight (+1) by
            the bid's weight, so every tie comes out at its own weight.
  diverges  Min::aggregate (operator/aggregate/min.rs:38-57) sums the
            weights of all rows sharing a price and skips the price if that
            sum is zero.  Here a rank stays present as long as any single
            row at it is present.  The two agree on every relation whose
            weights are positive (every Nexmark stream); they differ only
            when different rows at one rank carry weights of mixed sign that
            cancel.
  output    A tick's output is R(I + delta) - R(I), consolidated.

The operator also promises WHEN it reads a group's whole run (the refill
path), because its `groups_refilled` counter is tested.  With m a group's
largest present rank before the tick, the group is refilled iff it had a
present row before the tick and, after it, no present row of rank >= m
remains: its maximum drops, or it empties.  `refills()` counts those groups.
"""
import bisect

MASK64 = (1 << 64) - 1


def apply_delta(integral, delta):
    """integral + delta (zero weights dropped)."""
    out = dict(integral)
    for k, v, w in delta:
        key = (int(k) & MASK64, int(v) & MASK64)
        nw = out.get(key, 0) + int(w)
        if nw:
            out[key] = nw
        else:
            out.pop(key, None)
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


def zset_add(a, b):
    return zset_diff(a, {k: -w for k, w in b.items()})


def top_ranks(integral, group_shift, rank_shift):
    """{group: its largest present rank}; every row of an integral is
    present."""
    top = {}
    for k, _ in integral:
        g, r = k >> group_shift, k >> rank_shift
        if top.get(g, -1) < r:
            top[g] = r
    return top


def full_output(integral, group_shift, rank_shift):
    """R(I): the rows at their group's largest rank, at their weights."""
    top = top_ranks(integral, group_shift, rank_shift)
    return {key: w for key, w in integral.items()
            if key[0] >> rank_shift == top[key[0] >> group_shift]}


def brute_output(integral, group_shift, rank_shift):
    """O(n^2) restatement of full_output: a row is kept iff no row of its
    group has a greater rank."""
    out = {}
    for key, w in integral.items():
        g, r = key[0] >> group_shift, key[0] >> rank_shift
        if not any(o[0] >> group_shift == g and o[0] >> rank_shift > r
                   for o in integral):
            out[key] = w
    return out


def refills(integral, delta, group_shift, rank_shift):
    """How many groups the tick sends down the refill path (the rule in the
    module docstring); also returns how many groups the delta touches after
    consolidation."""
    d = apply_delta({}, delta)
    before = top_ranks(integral, group_shift, rank_shift)
    after = top_ranks(apply_delta(integral, delta), group_shift, rank_shift)
    touched = {key[0] >> group_shift for key in d}
    refilled = {g for g in touched
                if g in before and after.get(g, -1) < before[g]}
    return len(refilled), len(touched)


def step(integral, delta, group_shift, rank_shift):
    """One tick: (new integral, output delta, groups refilled, groups
    touched)."""
    after = apply_delta(integral, delta)
    out = zset_diff(full_output(after, group_shift, rank_shift),
                    full_output(integral, group_shift, rank_shift))
    n_refill, n_groups = refills(integral, delta, group_shift, rank_shift)
    return after, out, n_refill, n_groups


class Model:
    """The same rules kept incrementally (sorted per-group lists), so that a
    long stream costs the deltas and the tie sets, not ticks x integral.
    `step` returns (output delta, groups refilled, groups touched);
    tests/test_argmax_model.py holds it to the functions above."""

    def __init__(self, group_shift, rank_shift):
        self.group_shift, self.rank_shift = group_shift, rank_shift
        self.integral = {}
        self.groups = {}      # group -> sorted present rows
        self.acc = {}         # the accumulated output = R(integral)

    def _ties(self, g):
        rows = self.groups.get(g, [])
        if not rows:
            return {}
        top = rows[-1][0] >> self.rank_shift
        lo = bisect.bisect_left(rows, (top << self.rank_shift, 0))
        return {key: self.integral[key] for key in rows[lo:]}

    def step(self, delta):
        gs, rs = self.group_shift, self.rank_shift
        d = apply_delta({}, delta)
        old, old_top = {}, {}
        for key in d:
            g = key[0] >> gs
            if g not in old:
                old[g] = self._ties(g)
                rows = self.groups.get(g, [])
                old_top[g] = rows[-1][0] >> rs if rows else None
        for key, dw in d.items():
            g = key[0] >> gs
            w0 = self.integral.get(key, 0)
            w1 = w0 + dw
            if w1:
                self.integral[key] = w1
            else:
                del self.integral[key]
            rows = self.groups.setdefault(g, [])
            if w0 == 0 and w1 != 0:
                bisect.insort(rows, key)
            elif w0 != 0 and w1 == 0:
                rows.pop(bisect.bisect_left(rows, key))
        out, n_refill = {}, 0
        for g, ties0 in old.items():
            rows = self.groups.get(g, [])
            if old_top[g] is not None and (
                    not rows or rows[-1][0] >> rs < old_top[g]):
                n_refill += 1
            out.update(zset_diff(self._ties(g), ties0))
        self.acc = zset_add(self.acc, out)
        return out, n_refill, len(old)


def random_stream(seed, ticks=120, rows=200, n_groups=40, group_shift=20,
                  rank_shift=4, n_ranks=256, retract=0.3):
    """Per-tick deltas [(k, v, w)]: about `rows` rows per tick over n_groups
    groups; a share `retract` of them takes back (w = -1) a row inserted in
    an earlier tick, the rest insert (w = +1) a row at a random rank and tie
    position, now and then one that is already there (its weight goes
    to 2)."""
    import random
    rng = random.Random(seed)
    live, out = [], []
    for _ in range(ticks):
        delta, fresh = [], []
        for _ in range(rows):
            if live and rng.random() < retract:
                i = rng.randrange(len(live))
                live[i], live[-1] = live[-1], live[i]
                k, v = live.pop()
                delta.append((k, v, -1))
            else:
                g = rng.randrange(n_groups)
                k = ((g << group_shift) | (rng.randrange(n_ranks) << rank_shift)
                     | rng.randrange(1 << min(rank_shift, 2)))
                v = rng.randrange(3)
                delta.append((k, v, 1))
                fresh.append((k, v))
        live.extend(fresh)
        out.append(delta)
    return out


# the seed and shifts tests/test_gpu_argmax.py runs; tests/test_argmax_model.py
# checks that both verdicts occur often enough under them
RANDOM_SEED = 7
RANDOM_SHIFTS = (20, 4)


# ---- query 7 (include/dbsp_hip.h at dbsp_engine_create) ----

Q7_GROUP_SHIFT = 59
Q7_RANK_SHIFT = 32
Q7_WATERMARK_LAG_MS = 4000      # WATERMARK_INTERVAL_SECONDS, queries/mod.rs:12
Q7_TUMBLE_MS = 10000            # TUMBLE_SECONDS, q7.rs:43


def q7_pack(auction, bidder, price, date_time):
    """k = price << 32 | date_time, v = auction << 32 | bidder."""
    return ((int(price) << 32) | int(date_time),
            (int(auction) << 32) | int(bidder))


def q7_unpack(k, v):
    """(auction, bidder, price, date_time) of a packed row."""
    return v >> 32, v & 0xFFFFFFFF, k >> 32, k & 0xFFFFFFFF


class Q7:
    """q7.rs:45-94 over bids (auction, bidder, price, date_time, w):
      watermark  watermark_monotonic(date_time - 4000) (q7.rs:60-61): the
                 largest date_time seen so far minus the lag, never going
                 back; a tick without bids leaves it where it is
      bounds     rounded = wm - wm % 10000; the window is [rounded
                 saturating-minus 10000, rounded) (q7.rs:64-70)
      window     the bids whose date_time lies in the window (q7.rs:73),
                 the tick's own bids included
      tail       the windowed bids at the largest price (q7.rs:82-93): the
                 arg-max model over one group, ranked by price
    `step` returns the tick's output Z-set over q7_pack rows."""

    def __init__(self):
        self.wm = 0
        self.bounds = (0, 0)
        self.bids = {}        # the integral of all bids, q7_pack rows
        self.windowed = {}    # the integral of the windowed bids
        self.model = Model(Q7_GROUP_SHIFT, Q7_RANK_SHIFT)
        self.tumbles = 0      # how often the bounds moved
        self.refills = 0

    def step(self, bids):
        rows = [q7_pack(a, b, p, t) + (int(w),) for a, b, p, t, w in bids]
        if not rows:
            return {}
        tmax = max(k & 0xFFFFFFFF for k, _, _ in rows)
        assert tmax >= Q7_WATERMARK_LAG_MS      # the precondition of q5
        self.wm = max(self.wm, tmax - Q7_WATERMARK_LAG_MS)
        rounded = self.wm - self.wm % Q7_TUMBLE_MS
        bounds = (max(rounded - Q7_TUMBLE_MS, 0), rounded)
        self.bids = apply_delta(self.bids, rows)
        if bounds != self.bounds:
            if self.bounds != (0, 0):
                self.tumbles += 1
            self.bounds = bounds
            now = {key: w for key, w in self.bids.items()
                   if bounds[0] <= key[0] & 0xFFFFFFFF < bounds[1]}
        else:
            now = apply_delta(self.windowed, [
                r for r in rows if bounds[0] <= r[0] & 0xFFFFFFFF < bounds[1]])
        delta = zset_diff(now, self.windowed)
        self.windowed = now
        out, n_refill, _ = self.model.step(
            [(k, v, w) for (k, v), w in delta.items()])
        self.refills += n_refill
        return out
