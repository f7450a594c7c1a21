"""Dict model of the incremental antijoin / semijoin operator (dbsp_antijoin_op).

The rules, each with the reference item it restates (crates/dbsp/src/operator):

  * antijoin(A, B) = A - A |><| distinct(B) (join.rs:298-319): the rows of A
    whose key is not present in B.  Here B is a key set (I2::Val = ()), so
    the join with distinct(B) keeps a row of A, with its own weight, iff its
    key is present (join.rs:313); that kept part is this model's SEMIJOIN
    mode, and ANTIJOIN is the minus around it (join.rs:317-319).
  * a key is PRESENT iff its total weight in the integral of B is > 0
    (distinct.rs: the output weight is 1 iff the accumulated weight is
    positive).  A key at net -1 is absent.
  * per tick, with A, B the integrals before the tick and B' the key set after:
        d(A |> B) = dA * [k not in B'] + A * ([k not in B'] - [k not in B])
    The second term is non-zero only for keys whose presence FLIPS this tick;
    the model counts those keys (keys flipped), the rows of A under them
    (rows gathered: rows of the consolidated integral, non-zero weights) and
    the rows of the consolidated dA the first term drops (rows filtered).

The model does not use the formula: it recomputes full_output after the tick
and subtracts the one before, and only counts along the formula's terms.
Z-sets are {(k, v): w} for rows and {k: w} for keys, zero weights dropped.
"""

import random

from dbsp_amd import KIND_AUCTION, KIND_BID

ANTIJOIN, SEMIJOIN = 0, 1


def zset_add(a, b, sign=1):
    out = dict(a)
    for key, w in b.items():
        nw = out.get(key, 0) + sign * w
        if nw:
            out[key] = nw
        else:
            out.pop(key, None)
    return out


def present(integral_b, k):
    """distinct.rs: positive accumulated weight."""
    return integral_b.get(k, 0) > 0


def full_output(integral_a, integral_b, mode):
    """join.rs:298-319 over whole integrals: A restricted to the absent
    (ANTIJOIN) or present (SEMIJOIN) keys, weights unchanged."""
    keep_present = mode == SEMIJOIN
    return {(k, v): w for (k, v), w in integral_a.items()
            if present(integral_b, k) == keep_present}


def consolidate_rows(triples):
    out = {}
    for k, v, w in triples:
        out[(k, v)] = out.get((k, v), 0) + w
    return {key: w for key, w in out.items() if w}


def consolidate_keys(pairs):
    out = {}
    for k, w in pairs:
        out[k] = out.get(k, 0) + w
    return {k: w for k, w in out.items() if w}


class Model:
    def __init__(self, mode):
        assert mode in (ANTIJOIN, SEMIJOIN)
        self.mode = mode
        self.integral_a = {}   # {(k, v): w}
        self.integral_b = {}   # {k: w}
        self.acc = {}          # sum of every delta returned so far

    def step(self, dA, dB):
        """dA: [(k, v, w)], dB: [(k, w)], both raw.  Returns (expected delta
        zset, keys flipped, rows gathered, rows filtered)."""
        da, db = consolidate_rows(dA), consolidate_keys(dB)
        before = full_output(self.integral_a, self.integral_b, self.mode)
        new_b = zset_add(self.integral_b, db)
        flipped = {k for k in db
                   if present(self.integral_b, k) != present(new_b, k)}
        gathered = sum(1 for (k, _v) in self.integral_a if k in flipped)
        keep_present = self.mode == SEMIJOIN
        filtered = sum(1 for (k, _v) in da
                       if present(new_b, k) != keep_present)
        self.integral_a = zset_add(self.integral_a, da)
        self.integral_b = new_b
        after = full_output(self.integral_a, self.integral_b, self.mode)
        delta = zset_add(after, before, -1)
        self.acc = zset_add(self.acc, delta)
        return delta, len(flipped), gathered, filtered


def random_stream(seed, ticks=30, keys=64, retract=0.3):
    """[(dA, dB)] with about `retract` of each side's rows taking back a row
    or key sent earlier."""
    rng = random.Random(seed)
    sent_a, sent_b, out = [], [], []
    for _ in range(ticks):
        dA, dB = [], []
        for _ in range(rng.randrange(0, 12)):
            if sent_a and rng.random() < retract:
                k, v, w = rng.choice(sent_a)
                dA.append((k, v, -w))
            else:
                row = (rng.randrange(keys), rng.randrange(4),
                       rng.choice((1, 1, 2, -1)))
                dA.append(row)
                sent_a.append(row)
        for _ in range(rng.randrange(0, 8)):
            if sent_b and rng.random() < retract:
                k, w = rng.choice(sent_b)
                dB.append((k, -w))
            else:
                key = (rng.randrange(keys), rng.choice((1, 1, 2)))
                dB.append(key)
                sent_b.append(key)
        out.append((dA, dB))
    return out


def q103_deltas(ev):
    """Engine query 103's two inputs out of an event slice: the auctions as
    (id, seller, w) and the bids' auction keys as (auction, w)."""
    a = ev[ev["kind"] == KIND_AUCTION]
    b = ev[ev["kind"] == KIND_BID]
    return (list(zip(a["f0"].tolist(), a["f1"].tolist(), a["w"].tolist())),
            list(zip(b["f0"].tolist(), b["w"].tolist())))
