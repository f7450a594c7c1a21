"""Dict model of the incremental top-K per group operator (dbsp_topk_op in
include/dbsp_hip.h): the reference's Nexmark q19, an aggregate(Fold) that
keeps the last K values of a key's run followed by a flat_map
(crates/nexmark/src/queries/q19.rs:40-57).

Every rule is restated from the cited lines; nothing is executed from the
reference.

  rows      An integral is a dict {(k, v): weight} without zero weights; a
            delta is an iterable of (k, v, w).  k and v are 64-bit unsigned.
  group     g = k >> group_shift.  q19 indexes bids by (auction, (price,
            bid)) (q19.rs:41-44): the aggregate's key is the group, and its
            values, which the cursor walks in ascending order, are what is
            left of (k, v) below the group bits.  So (k, v) order is (group,
            rank) order.
  presence  A row is present iff its total weight is non-zero, negative
            totals included: Fold::aggregate walks the key's values and steps
            once per value on `!weight.is_zero()`, whatever the weight
            (aggregate/fold.rs:83-92).
  relation  Per group, the last min(K, present rows) present rows in (k, v)
            order: q19.rs:49-54 pops the front of a VecDeque at capacity and
            pushes every value at the back, so the K values seen last
            survive.  Each is output with weight +1 (the flat_map of
            q19.rs:56 over the aggregate's one output per key).
  output    A tick's output is R(I + delta) - R(I), consolidated.

The operator also promises WHEN it reads a group's whole run (the refill
path), because its `groups_refilled` counter is tested.  With Oc_g the
group's top-K before the tick, a group is refilled iff some row r of it
VANISHES in the tick (present before, absent after) with len(Oc_g) == K and
r >= Oc_g[0]; `refills()` counts those groups.
"""

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


def groups_of(integral, shift):
    """{group: sorted present rows}; every row of an integral is present
    (fold.rs:83-92: non-zero weight, either sign)."""
    g = {}
    for key in integral:
        g.setdefault(key[0] >> shift, []).append(key)
    for rows in g.values():
        rows.sort()
    return g


def full_output(integral, K, shift):
    """R(I): the last <= K rows of every group, each at +1 (q19.rs:49-56)."""
    out = {}
    for rows in groups_of(integral, shift).values():
        for key in rows[-K:]:
            out[key] = 1
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


def refills(integral, delta, K, shift):
    """How many groups the tick sends down the refill path (the verdict rule
    in the module docstring); also returns how many groups the delta
    touches after consolidation."""
    d = apply_delta({}, delta)
    before = groups_of(integral, shift)
    touched, refilled = set(), set()
    for key, dw in d.items():
        g = key[0] >> shift
        touched.add(g)
        w0 = integral.get(key, 0)
        if w0 != 0 and w0 + dw == 0:            # vanish
            top = before.get(g, [])[-K:]
            if len(top) == K and key >= top[0]:
                refilled.add(g)
    return len(refilled), len(touched)


def step(integral, delta, K, shift):
    """One tick: (new integral, output delta, groups refilled, groups
    touched)."""
    after = apply_delta(integral, delta)
    out = zset_diff(full_output(after, K, shift),
                    full_output(integral, K, shift))
    n_refill, n_groups = refills(integral, delta, K, shift)
    return after, out, n_refill, n_groups


def brute_output(integral, K, shift):
    """O(n^2) restatement of full_output: a row is kept iff fewer than K
    rows of its group are greater."""
    out = {}
    for key in integral:
        g = key[0] >> shift
        above = sum(1 for other in integral
                    if other[0] >> shift == g and other > key)
        if above < K:
            out[key] = 1
    return out


class Model:
    """The same rules kept incrementally (sorted per-group lists), so that a
    long stream costs the deltas and not ticks x integral.  `step` returns
    (output delta, groups refilled, groups touched); tests/test_topk_model.py
    holds it to the functions above."""

    def __init__(self, K, shift):
        self.K, self.shift = K, shift
        self.integral = {}
        self.groups = {}      # group -> sorted present rows
        self.acc = {}         # the accumulated output = R(integral)

    def step(self, delta):
        import bisect
        K, shift = self.K, self.shift
        d = apply_delta({}, delta)
        n_refill, n_groups = refills_sorted(self.integral, self.groups, d, K,
                                            shift)
        old = {}
        for key in d:
            g = key[0] >> shift
            if g not in old:
                old[g] = list(self.groups.get(g, [])[-K:])
        for key, dw in d.items():
            g = key[0] >> shift
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
        out = {}
        for g, top0 in old.items():
            top1 = self.groups.get(g, [])[-K:]
            s0, s1 = set(top0), set(top1)
            for key in s1 - s0:
                out[key] = 1
            for key in s0 - s1:
                out[key] = -1
        self.acc = zset_add(self.acc, out)
        return out, n_refill, n_groups


def refills_sorted(integral, groups, d, K, shift):
    """refills() over a consolidated delta dict and ready per-group lists."""
    touched, refilled = set(), set()
    for key, dw in d.items():
        g = key[0] >> shift
        touched.add(g)
        w0 = integral.get(key, 0)
        if w0 != 0 and w0 + dw == 0:
            top = groups.get(g, [])[-K:]
            if len(top) == K and key >= top[0]:
                refilled.add(g)
    return len(refilled), len(touched)


def random_stream(seed, ticks=200, rows=300, n_groups=40, shift=20,
                  retract=0.3):
    """Per-tick deltas [(k, v, w)]: about `rows` rows per tick over n_groups
    groups; a share `retract` of them takes back (w = -1) a row inserted in
    an earlier tick, the rest insert (w = +1) a row at a random rank, now and
    then one that is already there (its weight goes to 2)."""
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
                k = (g << shift) | rng.randrange(1 << min(shift, 12))
                v = rng.randrange(4)
                delta.append((k, v, 1))
                fresh.append((k, v))
        live.extend(fresh)
        out.append(delta)
    return out


# the seed tests/test_gpu_topk.py runs; tests/test_topk_model.py checks that
# both verdicts occur often enough under it
RANDOM_SEED = 19


# ---- query 19 packing (include/dbsp_hip.h at dbsp_engine_create) ----

Q19_SHIFT = 27


def q19_pack(auction, bidder, price, date_time=0):
    """k = auction << 27 | price, v = bidder << 32 | date_time."""
    return (int(auction) << 27) | int(price), (int(bidder) << 32) | int(date_time)


def q19_unpack(k, v):
    """(auction, bidder, price, date_time) of a packed row."""
    return k >> 27, v >> 32, k & ((1 << 27) - 1), v & ((1 << 32) - 1)
