"""Pattern builders and CPU references for the keyed aggregates: the three
aggregate + upsert modes (`Ctx.agg_linear_upsert`, `agg_max_upsert`,
`agg_last10_upsert`), the per-batch linear sum over a spine
(`Ctx.agg_sum_spine`) and the incremental distinct (`Ctx.distinct_inc`).

The references are written from the reference operators (aggregate/mod.rs
:129-156, max.rs:36-55, queries/q6.rs:97-110 over fold.rs:76-96, upsert.rs
:161-208, distinct.rs:404-462) in numpy and Python ints, independently of the
kernels and of the C++ oracle.  Builders are deterministic; an upsert case is
dict(name, keys, in_rows, out_rows, meta).  Nothing here needs a GPU."""
import functools

import numpy as np

from dbsp_amd import ROW_DT

M64 = (1 << 64) - 1
MAX_TRACE_BATCHES = 24
PRICE_BITS = 27                 # q6 val = auction << 27 | price
PRICE_MAX = (1 << PRICE_BITS) - 1
AUCTION_MAX = (1 << (64 - PRICE_BITS)) - 1
LAST_N = 10                     # NUM_AUCTIONS_PER_SELLER
MODES = ("linear", "max", "last10")
SIZES = (1, 255, 256, 257, 2048, 2049, 65537)


def _rows(k, v, w):
    out = np.empty(len(k), dtype=ROW_DT)
    out["k"] = np.asarray(k, dtype=np.uint64)
    out["v"] = np.asarray(v, dtype=np.uint64)
    out["w"] = np.asarray(w, dtype=np.int64)
    return out


EMPTY = _rows([], [], [])


def rows_of(triples):
    """Consolidated rows from (k, v, w) triples given in (k, v) order."""
    r = _rows([t[0] for t in triples], [t[1] for t in triples],
              [t[2] for t in triples])
    assert consolidated(r), "triples ascend by (k, v), weights non-zero"
    return r


def consolidated(r):
    if len(r) and not np.all(r["w"] != 0):
        return False
    if len(r) < 2:
        return True
    k, v = r["k"], r["v"]
    return bool(np.all((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) &
                                           (v[1:] > v[:-1]))))


def bid(auction, price):
    assert 0 <= auction <= AUCTION_MAX and 0 <= price <= PRICE_MAX
    return auction * (1 << PRICE_BITS) + price


def key_run(rows, key):
    k = np.ascontiguousarray(rows["k"])
    lo = int(np.searchsorted(k, np.uint64(key), side="left"))
    hi = int(np.searchsorted(k, np.uint64(key), side="right"))
    return rows[lo:hi]


# ---- the references ----

def new_value(mode, run, variant=None):
    """The aggregate of one key's rows (cursor order), None when there is
    none.  `variant` names a wrong last-10 fold for the model tests: "first"
    keeps the first 10, "positive" only rows of positive weight, "mask20"
    a 20-bit price."""
    if mode == "linear":
        s = sum(int(w) for w in run["w"])
        return s & M64 if s != 0 else None
    live = [int(v) for v, w in zip(run["v"], run["w"])
            if (w > 0 if variant == "positive" else w != 0)]
    if not live:
        return None
    if mode == "max":
        return live[-1]
    assert mode == "last10", mode
    top = live[:LAST_N] if variant == "first" else live[-LAST_N:]
    bits = 20 if variant == "mask20" else PRICE_BITS
    return sum(v % (1 << bits) for v in top) // len(top)


def ref_upsert(mode, keys, in_rows, out_rows, variant=None):
    """Raw rows in kernel order: per key the new row (key, value, +1) when
    the aggregate exists, then the key's output-trace rows negated, in trace
    order (Upsert::eval before its per-key consolidation)."""
    ik = np.ascontiguousarray(in_rows["k"])
    ok = np.ascontiguousarray(out_rows["k"])
    keys = np.asarray(keys, dtype=np.uint64)
    ilo = np.searchsorted(ik, keys, side="left")
    ihi = np.searchsorted(ik, keys, side="right")
    olo = np.searchsorted(ok, keys, side="left")
    ohi = np.searchsorted(ok, keys, side="right")
    out = []
    for i, key in enumerate(keys.tolist()):
        if ihi[i] > ilo[i]:
            nv = new_value(mode, in_rows[ilo[i]:ihi[i]], variant)
            if nv is not None:
                out.append((key, nv, 1))
        for t in range(olo[i], ohi[i]):
            out.append((key, int(out_rows["v"][t]), -int(out_rows["w"][t])))
    return _rows([t[0] for t in out], [t[1] for t in out],
                 [t[2] for t in out])


def ref_sum_spine(delta, batches):
    """(keys, rows): the delta's distinct keys, and (key, sum, +1) for every
    key whose weights summed over all batches are non-zero, by key."""
    keys = np.unique(np.ascontiguousarray(delta["k"]))
    tot = np.zeros(len(keys), dtype=object)
    for b in batches:
        bk = np.ascontiguousarray(b["k"])
        lo = np.searchsorted(bk, keys, side="left")
        hi = np.searchsorted(bk, keys, side="right")
        cs = np.concatenate([[0], np.cumsum(b["w"].astype(object))])
        tot = tot + (cs[hi] - cs[lo])
    keep = [i for i in range(len(keys)) if tot[i] != 0]
    return keys, _rows([int(keys[i]) for i in keep],
                       [int(tot[i]) & M64 for i in keep], [1] * len(keep))


def ref_distinct(delta, batches):
    """Per delta pair [before + dw > 0] - [before > 0], before = the pair's
    weight summed over the batches; pairs with 0 dropped, delta order."""
    total = {}
    for b in batches:
        for k, v, w in zip(b["k"].tolist(), b["v"].tolist(), b["w"].tolist()):
            total[(k, v)] = total.get((k, v), 0) + w
    out = []
    for k, v, w in zip(delta["k"].tolist(), delta["v"].tolist(),
                       delta["w"].tolist()):
        before = total.get((k, v), 0)
        o = int(before + w > 0) - int(before > 0)
        if o:
            out.append((k, v, o))
    return _rows([t[0] for t in out], [t[1] for t in out],
                 [t[2] for t in out])


def sorted_rows(r):
    return np.sort(np.asarray(r, dtype=ROW_DT), order=["k", "v", "w"])


# ---- upsert patterns ----

def _case(name, keys, in_rows, out_rows, **meta):
    keys = np.asarray(keys, dtype=np.uint64)
    assert np.all(keys[1:] > keys[:-1]), "delta keys ascend"
    assert consolidated(in_rows) and consolidated(out_rows), name
    return {"name": name, "keys": keys, "in_rows": in_rows,
            "out_rows": out_rows, "meta": meta}


def _price(i, seed):
    return (i * 2654435761 + seed * 40503) % (PRICE_MAX + 1)


@functools.lru_cache(maxsize=None)
def last10_cases():
    triples, meta = [], {}
    # one seller per run length; the auction ids ascend, the prices do not
    for s, n in enumerate((1, 9, 10, 11, 12, 100)):
        key = 100 + s
        triples += [(key, bid(50 + j, _price(j, s)), 1 + j % 3)
                    for j in range(n)]
        meta[key] = n
    out = [_case("last10-run-lengths", sorted(meta), rows_of(triples),
                 rows_of([(103, 5, 1), (105, 77, 2)]), lengths=meta)]
    t = ([(1, bid(j, 0), 1) for j in range(12)] +
         [(2, bid(j, PRICE_MAX), 1) for j in range(12)] +
         # every high bit of the val set: none may reach the sum
         [(3, bid(AUCTION_MAX, PRICE_MAX - 11 + j), 1) for j in range(12)] +
         [(4, bid(AUCTION_MAX - 1, 1), 1), (4, bid(AUCTION_MAX, 2), 1)] +
         # above 2^20: a 20-bit mask loses it
         [(5, bid(9, (1 << 20) + 5), 1)])
    out.append(_case("last10-price-edges", [1, 2, 3, 4, 5], rows_of(t), EMPTY,
                     floor_key=4))
    t = ([(7, bid(j, 100 + j), -1 if j % 3 == 0 else 2) for j in range(14)] +
         [(8, bid(j, 1000 + 7 * j), -1 - j % 2) for j in range(12)] +
         [(9, bid(1, 40), -5)])
    out.append(_case("last10-negative-weights", [7, 8, 9], rows_of(t),
                     rows_of([(8, 3, 1)]), mixed_key=7, negative_keys=(8, 9)))
    return out


@functools.lru_cache(maxsize=None)
def max_cases():
    t = ([(10, 500, 2)] +
         [(11, 3 * j, 1 + j % 2) for j in range(257)] +
         [(12, 7, 1), (12, 9, 3), (12, 11, -2)] +
         [(13, M64, 1)])
    return [_case("max-runs", [10, 11, 12, 13], rows_of(t),
                  rows_of([(11, 768, 1), (12, 9, 1)]),
                  lengths={10: 1, 11: 257, 12: 3, 13: 1}, negative_last=12)]


@functools.lru_cache(maxsize=None)
def linear_cases():
    t = ([(20, 0, 4), (20, 1, -4)] +                    # sums to zero
         [(21, 0, 2), (21, 5, -9)] +                    # negative sum
         [(22, j, 1 + j % 4) for j in range(1000)] +    # a run of 1000
         [(23, 0, -(1 << 62))])
    return [_case("linear-sums", [20, 21, 22, 23], rows_of(t),
                  rows_of([(20, 6, 1), (21, 3, 1)]), zero_key=20,
                  negative_key=21, long_key=22)]


@functools.lru_cache(maxsize=None)
def key_cases():
    """Cases every mode runs.  A one-row run (k, 7, 7) aggregates to 7 under
    all three modes: the weight sum, the largest val and the only price."""
    in_t = rows_of([(0, 7, 7), (10, 7, 7), (10, 9, 1), (20, 7, 7),
                    (40, 1, 1), (40, 2, -1), (M64, 7, 7)])
    out_t = rows_of([(0, 3, 1), (20, 7, 1), (30, 4, 1), (30, 6, -2),
                     (30, 8, 1), (40, 5, -1), (40, 9, 2), (M64, 1, 1)])
    out = [
        _case("keys-ends", [0, M64], in_t, out_t),
        _case("keys-first-last-of-trace", [0, 10, M64], in_t, out_t),
        _case("keys-same-val", [20], in_t, out_t, same=(20, 7)),
        _case("keys-only-in", [10], in_t, out_t),
        _case("keys-only-out", [30], in_t, out_t),
        _case("keys-out-several-vals", [30, 40], in_t, out_t),
        _case("keys-all", [0, 5, 10, 15, 20, 30, 40, 50, M64], in_t, out_t),
        _case("keys-empty-in", [0, 20, 30], EMPTY, out_t),
        _case("keys-empty-out", [0, 10, 40], in_t, EMPTY),
        _case("keys-both-empty", [1, 2], EMPTY, EMPTY),
        _case("keys-none", [], in_t, out_t),
    ]
    lo = rows_of([(10, 7, 7), (20, 1, 1), (20, 2, 2)])
    out.append(_case("keys-absent", [5, 15, 25, M64 - 1], lo,
                     rows_of([(10, 1, 1), (20, 9, 1)]),
                     absent=(5, 15, 25, M64 - 1)))
    return out


@functools.lru_cache(maxsize=None)
def size_case(nd):
    """nd delta keys over traces holding 0..3 rows of each, and keys of
    their own in between."""
    i = np.arange(nd, dtype=np.int64)
    keys = (i * 5 + 3).astype(np.uint64)
    cnt_in = (i * 7 + 1) % 4
    cnt_out = (i * 5 + 2) % 3

    def trace(cnt, seed):
        k = np.repeat(keys, cnt)
        extra = (i[::3] * 5 + 4).astype(np.uint64)   # keys no delta names
        start = np.repeat(np.cumsum(cnt) - cnt, cnt)
        j = np.arange(len(k), dtype=np.int64) - start
        v = (j * 11 + (np.repeat(i, cnt) + seed) % 9).astype(np.uint64)
        w = (np.arange(len(k), dtype=np.int64) + seed) % 5 - 2
        w[w == 0] = 4
        r = np.concatenate([_rows(k, v, w),
                            _rows(extra, extra % np.uint64(13),
                                  np.ones(len(extra), dtype=np.int64))])
        return r[np.lexsort((r["v"], r["k"]))]

    return _case(f"size-{nd}", keys, trace(cnt_in, 1), trace(cnt_out, 2),
                 nd=nd)


# ---- the sum over a spine ----

def _spread(nkeys, step, reps, seed):
    k = np.repeat(np.arange(nkeys, dtype=np.uint64) * np.uint64(step), reps)
    j = np.arange(len(k), dtype=np.int64)
    w = (j * 3 + seed) % 7 - 3
    w[w == 0] = 5
    return _rows(k, (j % reps).astype(np.uint64), w)


@functools.lru_cache(maxsize=None)
def sum_cases():
    """(name, delta, batches, meta)."""
    out = []
    delta = _spread(300, 2, 1, 0)
    for nb in (1, 2, MAX_TRACE_BATCHES):
        batches = [EMPTY if (nb > 1 and b % 4 == 1) else
                   _spread(200 + 10 * b, 1 + b % 3, 1 + b % 2, b)
                   for b in range(nb)]
        out.append((f"sum-nb{nb}", delta, batches, {"nb": nb}))
    out.append(("sum-all-empty", delta, [EMPTY, EMPTY], {"nb": 2}))
    out.append(("sum-no-batches", delta, [], {"nb": 0}))
    # keys 0..9: cancel inside one batch (3), only across batches (4, 5)
    a = rows_of([(3, 0, 2), (3, 1, -2), (4, 0, 6), (5, 0, -1), (6, 0, 1)])
    b = rows_of([(4, 0, -4), (5, 1, 3), (7, 0, 2)])
    c = rows_of([(4, 9, -2), (5, 0, -2), (M64, 0, 1)])
    d = _rows(list(range(10)) + [M64], [0] * 11, [1] * 11)
    out.append(("sum-cancel-across-batches", d, [a, b, c],
                {"zero_keys": (3, 4, 5), "nb": 3}))
    some = [_spread(50, 1, 2, 1), _spread(400, 3, 1, 2)]
    n = 600
    out.append(("uniq-all-equal",
                _rows([9] * n, range(n), [1] * n), some, {"nkeys": 1}))
    out.append(("uniq-all-distinct",
                _rows(range(0, 2 * n, 2), [0] * n, [1] * n), some,
                {"nkeys": n}))
    out.append(("uniq-one-row", _rows([6], [1], [-1]), some, {"nkeys": 1}))
    # heads at positions 255, 256 and 257: a block's last row, the next
    # block's first and second
    k = np.zeros(n, dtype=np.uint64)
    k[255:], k[256:], k[257:] = 2, 4, 6
    out.append(("uniq-heads-255-256-257", _rows(k, range(n), [1] * n), some,
                {"nkeys": 4, "heads": (0, 255, 256, 257)}))
    # one run across the block edge, 250..260
    k = np.arange(n, dtype=np.uint64) * np.uint64(3)
    k[250:261] = k[250]
    out.append(("uniq-run-across-256", _rows(k, range(n), [1] * n), some,
                {"nkeys": n - 10}))
    out.append(("uniq-empty", EMPTY, some, {"nkeys": 0}))
    return out


# ---- distinct ----

@functools.lru_cache(maxsize=None)
def distinct_cases():
    """(name, delta, batches, meta)."""
    t = rows_of([(5, 1, 1), (5, 2, 2), (6, 9, 1), (6, 12, 1), (8, 3, 1),
                 (8, 4, 1)])
    out = [
        ("distinct-val-absent", rows_of([(5, 0, 1), (5, 3, 1), (6, 10, 1)]),
         [t], {}),
        # (5, 9) is above key 5's run; key 6 opens with the same val
        ("distinct-val-above-run-next-key-equal",
         rows_of([(5, 9, 1), (6, 9, -1)]), [t], {}),
        # key 8's run ends the batch: a val above it has no row after
        ("distinct-run-ends-batch", rows_of([(8, 4, -1), (8, 5, 1),
                                             (9, 0, 1)]), [t], {}),
        ("distinct-no-batches", rows_of([(1, 1, 1), (1, 2, -1)]), [], {}),
    ]
    # totals that cross zero only when summed: +2 -3 +1 = 0, -1 +2 = +1
    b0 = rows_of([(1, 1, 2), (2, 1, -1), (3, 1, 1), (4, 1, -2)])
    b1 = rows_of([(1, 1, -3), (2, 1, 2), (3, 1, 1), (4, 1, 1)])
    b2 = rows_of([(1, 1, 1), (3, 1, -1)])
    out.append(("distinct-cross-zero-over-batches",
                rows_of([(1, 1, 1), (2, 1, -1), (3, 1, -1), (4, 1, 2),
                         (4, 2, 1)]), [b0, b1, b2], {}))
    nb = MAX_TRACE_BATCHES
    batches = []
    for b in range(nb):
        k = np.arange(b % 3, 400, 3, dtype=np.uint64)
        batches.append(_rows(k, k % np.uint64(4),
                             np.where((k + np.uint64(b)) % np.uint64(5) < 2,
                                      -1, 1)))
    dk = np.arange(0, 400, dtype=np.uint64)
    delta = _rows(dk, dk % np.uint64(4), np.where(dk % np.uint64(2) == 0, 1, -1)
                  * (1 + (dk % np.uint64(3)).astype(np.int64)))
    out.append(("distinct-nb24", delta, batches, {"nb": nb}))
    return out
