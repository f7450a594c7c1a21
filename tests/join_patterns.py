"""Pattern builders and CPU references for the join kernels: the spine join
(`Ctx.join_spine`, both routes), the single-batch `Ctx.join` and the chained
join tail (`Ctx.join_tail`).

`ref_join` is written from the projection layouts documented in
include/dbsp_hip.h, in numpy integer arithmetic mod 2^64 (div / mod by powers
of two, no shifts or masks), and finds the matches with np.searchsorted: it
shares nothing with the kernel's proj_out / gallop_run or the C++ oracle's
proj_emit.  Every builder is deterministic in its seed and returns a list of
cases (name, delta, batches, meta); the tail builders return
(name, plans, cap, meta).  Nothing here needs a GPU."""
import numpy as np

from dbsp_amd import ROW_DT, oracle

M64 = (1 << 64) - 1
MAX_TRACE_BATCHES = 24  # kernels_iface.hpp
FUSE_MAX = 8192         # delta rows of the small route and of a tail plan
FUSE_THREADS = 1024     # threads of the scan / tail workgroup (8 rows each);
                        # a combined total within it stays on chip
PROBE_BLOCK = 256       # BLK: threads of a k_join_probe_multi block
PROBE_STRIDE = 8 * 256  # JPROBE_BLOCKS * BLK: rows one probe sweep covers
SCAN_BLOCK = 2048       # SORT_TILE = BLK * SORT_ITEMS: rows per block of
                        # scan_exclusive (kernels.hip), route 1's scan
TAIL_CAP = 32768        # Q3_EMIT_CAP (engine.cpp), the default capacity

RUN_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 1000)
SIZES_SMALL = (1, 255, 256, 257, 2047, 2048, 2049, 8191, 8192)
SIZES_BIG = (8193, SCAN_BLOCK - 1, SCAN_BLOCK + 1, 19999, 20000)
NB_GRID = (1, 2, 3, MAX_TRACE_BATCHES)

# value layouts of the q4 / q6 projections, most significant field first
BID = (("dt", 37), ("price", 27))
AUC4 = (("dt", 36), ("dur", 24), ("tag", 4))    # tag = category
AUC6 = (("dt", 28), ("dur", 16), ("tag", 20))   # tag = seller


def _rows(k, v, w):
    out = np.empty(len(k), dtype=ROW_DT)
    out["k"] = np.asarray(k, dtype=np.uint64)
    out["v"] = np.asarray(v, dtype=np.uint64)
    out["w"] = np.asarray(w, dtype=np.int64)
    return out


EMPTY = _rows([], [], [])


def sorted_kv(r, distinct=True):
    if len(r) < 2:
        return True
    k, v = r["k"], r["v"]
    gt = v[1:] > v[:-1] if distinct else v[1:] >= v[:-1]
    return bool(np.all((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & gt)))


def pack(layout, **fields):
    v = 0
    for name, bits in layout:
        f = int(fields[name])
        assert 0 <= f < (1 << bits), (name, f)
        v = v * (1 << bits) + f
    assert v <= M64
    return v


def unpack(layout, v):
    """Fields of a uint64 array, by div / mod from the low end."""
    v = np.asarray(v, dtype=np.uint64)
    out = {}
    for name, bits in reversed(layout):
        m = np.uint64(1 << bits)
        out[name] = v % m
        v = v // m
    return out


# ---- the reference ----

def match_ranges(delta, batches):
    """lo[i, b], cnt[i, b]: batch b's rows lo .. lo + cnt - 1 hold the key of
    delta row i."""
    nd, nb = len(delta), len(batches)
    lo = np.zeros((nd, nb), dtype=np.int64)
    cnt = np.zeros((nd, nb), dtype=np.int64)
    dk = np.ascontiguousarray(delta["k"])
    for b, t in enumerate(batches):
        tk = np.ascontiguousarray(t["k"])
        lo[:, b] = np.searchsorted(tk, dk, side="left")
        cnt[:, b] = np.searchsorted(tk, dk, side="right") - lo[:, b]
    return lo, cnt


def project(proj, param, k, v1, v2):
    """(hi, lo, valid) of the 13 projections of include/dbsp_hip.h."""
    two32 = np.uint64(1 << 32)
    ok = np.ones(len(k), dtype=bool)
    if proj == 0:
        return v2, v1, ok
    if proj == 1:
        return v1, v2, ok
    if proj == 2:
        return k, (v1 % two32) * two32 + v2 % two32, ok
    if proj in (3, 4):
        v = v1 if proj == 3 else v2
        dt = v % two32
        return k, (v - dt) + (dt - dt % np.uint64(param)), ok
    if proj == 5:
        return v2, k, ok
    if proj == 6:
        return v1, k, ok
    if proj == 7:
        return k, (v2 % two32) * two32 + v1 % two32, ok
    if proj == 8:
        return k, v2, ok
    assert proj in (9, 10, 11, 12), proj
    bid_v, auc_v = (v1, v2) if proj in (9, 11) else (v2, v1)
    layout = AUC4 if proj in (9, 10) else AUC6
    bid, auc = unpack(BID, bid_v), unpack(layout, auc_v)
    tag_bits = dict(layout)["tag"]
    with np.errstate(over="ignore"):
        hi = k * np.uint64(1 << tag_bits) + auc["tag"]  # mod 2^64
    ok = (bid["dt"] >= auc["dt"]) & (bid["dt"] <= auc["dt"] + auc["dur"])
    return hi, bid["price"], ok


def ref_join(delta, batches, proj, param=0):
    """The raw rows of delta x spine in the kernels' order: delta row major,
    then batch, then trace position; an invalid q4 / q6 pair keeps its slot
    with weight 0."""
    nd, nb = len(delta), len(batches)
    if nd == 0 or nb == 0:
        return EMPTY.copy()
    lo, cnt = match_ranges(delta, batches)
    c = cnt.reshape(-1)
    total = int(c.sum())
    if total == 0:
        return EMPTY.copy()
    seg = np.repeat(np.arange(nd * nb), c)
    within = np.arange(total) - (np.cumsum(c) - c)[seg]
    i, b = seg // nb, seg % nb
    lens = np.array([len(t) for t in batches], dtype=np.int64)
    base = np.cumsum(lens) - lens
    trace = np.concatenate(batches)
    g = base[b] + lo.reshape(-1)[seg] + within
    k, v1, v2 = delta["k"][i], delta["v"][i], trace["v"][g]
    with np.errstate(over="ignore"):
        w = delta["w"][i] * trace["w"][g]
        hi, lo_out, ok = project(proj, param, k, v1, v2)
    return _rows(hi, lo_out, np.where(ok, w, 0))


def merged_trace(batches):
    """One (k, v)-sorted batch holding every row of the spine (unconsolidated:
    what the single-trace oracle join takes)."""
    t = np.concatenate(batches) if len(batches) else EMPTY.copy()
    return t[np.lexsort((t["v"], t["k"]))]


def plan_view(pl):
    """(delta, batches) as the kernels see plan `pl`, or None when one of its
    lengths is poisoned (negative, or a delta above FUSE_MAX)."""
    delta, batches = pl["delta"], list(pl["batches"])
    nd = pl.get("nd")
    nd = len(delta) if nd is None else nd
    if nd < 0 or nd > FUSE_MAX:
        return None
    if pl.get("fresh"):
        tn = pl.get("tn")
        tn = len(batches[0]) if tn is None else tn
        if tn < 0:
            return None
        batches = [batches[0][:tn]]
    return delta[:nd], batches


def ref_tail(plans, cap=TAIL_CAP):
    """Verdicts, plan-local offsets, capacity-buffer rows and consolidated
    store of the chained join tail.  A tick-fresh trace of length 0 is an
    empty trace, not a poisoned one: the plan is healthy with total 0."""
    totals, offsets, raws = [], [], []
    for pl in plans:
        view = plan_view(pl)
        if view is None:
            totals.append(-1)
            offsets.append(None)
            continue
        d, bs = view
        raw = ref_join(d, bs, pl["proj"], 0)
        per_row = match_ranges(d, bs)[1].sum(axis=1)
        totals.append(len(raw))
        offsets.append((np.cumsum(per_row) - per_row).astype(np.uint64))
        raws.append(raw)
    bad = any(t < 0 for t in totals)
    tot = sum(t for t in totals if t >= 0)
    flag = 1 if bad or tot > cap else 0
    rows = np.concatenate(raws) if raws else EMPTY.copy()
    fused = not flag and tot <= FUSE_MAX
    return {
        "totals": totals, "offsets": offsets,
        "d_total": -1 if flag else tot, "d_flag": flag,
        "d_final": len(oracle.consolidate(rows)) if fused else -1,
        "store": oracle.consolidate(rows) if fused else None,
        "capbuf": rows if not flag and not fused else None,
    }


# ---- CPU models of the two searches, with their classic wrong variants ----

GALLOP_WRONG = ("lt_final", "rem_minus_one", "loop_le_nt", "loop_stops_early")
OWNER_WRONG = ("lt", "first_equal", "short")


def gallop_model(tk, key, lo, variant="right"):
    """gallop_run of kernels.hip: the length of key's run starting at lo.
    A read outside [0, nt) raises IndexError.
      lt_final          `<` for `<=` in the closing binary search
      rem_minus_one     the closing window one short
      loop_le_nt        the doubling loop's bound `<= nt` for `< nt`
      loop_stops_early  the doubling loop's bound `< nt - 1`"""
    nt = len(tk)

    def at(i):
        if not 0 <= i < nt:
            raise IndexError(i)
        return int(tk[i])
    if lo >= nt or at(lo) != key:
        return 0
    hi, step = lo, 1
    while True:
        if variant == "loop_le_nt":
            inside = hi + step <= nt
        elif variant == "loop_stops_early":
            inside = hi + step < nt - 1
        else:
            inside = hi + step < nt
        if not (inside and at(hi + step) == key):
            break
        hi += step
        step *= 2
    rem = min(step, nt - hi) - (1 if variant == "rem_minus_one" else 0)
    a, b = 0, rem
    while a < b:
        m = (a + b) // 2
        x = at(hi + m)
        if (x < key) if variant == "lt_final" else (x <= key):
            a = m + 1
        else:
            b = m
    return hi + a - lo


def owner_model(offsets, o, variant="right"):
    """The emit's search for the delta row that owns output slot o:
    upper_bound(offsets, o) - 1 over the exclusive offsets.
      lt           `<` for `<=` (lower_bound - 1)
      first_equal  the first of the rows sharing the owner's offset
      short        the search range one row short (hi = nd - 1)"""
    nd = len(offsets)
    lo, hi = 0, nd - 1 if variant == "short" else nd
    while lo < hi:
        mid = (lo + hi) // 2
        x = int(offsets[mid])
        if (x < o) if variant == "lt" else (x <= o):
            lo = mid + 1
        else:
            hi = mid
    i = lo - 1
    if variant == "first_equal":
        while i > 0 and offsets[i - 1] == offsets[i]:
            i -= 1
    return i


# ---- row material ----

def _weights(rng, n):
    """Small weights, never 0 and of both signs from two rows on: a fixed
    cycle entered at a random place.  Products stay far from 2^63."""
    cycle = np.array([1, -2, 3, -1, 2, -5], dtype=np.int64)
    return cycle[(int(rng.integers(0, 6)) + np.arange(n)) % 6]


def _trace_batch(rng, keys, tag):
    """Rows over the sorted `keys`; v = tag << 40 | position, so a row's v
    names its batch and place and (k, v) is sorted."""
    keys = np.asarray(keys, dtype=np.uint64)
    assert np.all(keys[1:] >= keys[:-1])
    pos = np.arange(len(keys), dtype=np.uint64)
    return _rows(keys, (np.uint64(tag + 1) << np.uint64(40)) | pos,
                 _weights(rng, len(keys)))


def _delta(rng, keys):
    """Rows over the sorted `keys` (repeats allowed); v = 7 * position + 1."""
    keys = np.asarray(keys, dtype=np.uint64)
    assert np.all(keys[1:] >= keys[:-1])
    pos = np.arange(len(keys), dtype=np.uint64)
    return _rows(keys, 7 * pos + 1, _weights(rng, len(keys)))


# ---- runs ----

FILL = 37  # rows on each open side of a run: no multiple of 8
MID_KEY = (1 << 33) + 5


def pat_run(length, place, key, seed=11):
    """One key's run of `length` rows at the `place` of its batch ("start",
    "end", "middle", "whole"), with key - 1 and key + 1 directly beside it
    where the place has that side.  None when the key leaves no room."""
    below = place in ("end", "middle")
    above = place in ("start", "middle")
    if (below and key < 1 + 10 * FILL) or (above and key > M64 - 1 - 10 * FILL):
        return None
    rng = np.random.default_rng(seed)
    lo_keys = [key - 1 - 10 * j for j in range(FILL)][::-1] if below else []
    hi_keys = [key + 1 + 10 * j for j in range(FILL)] if above else []
    tkeys = lo_keys + [key] * length + hi_keys
    probe = {key - 1, key + 1, key - 6, key + 6, key - 11, key + 11,
             tkeys[0] - 3, tkeys[-1] + 3, tkeys[0], tkeys[-1]}
    dkeys = sorted(x for x in probe if 0 <= x <= M64 and x != key)
    dkeys = sorted(dkeys + [key, key])  # two delta rows probe the run
    meta = {"length": length, "place": place, "key": key,
            "run_at": len(lo_keys), "nt": len(tkeys)}
    name = f"run L={length} {place} key={key:#x}"
    return name, _delta(rng, dkeys), [_trace_batch(rng, tkeys, 0)], meta


def run_cases(seed=11):
    out = []
    for length in RUN_LENGTHS:
        for key in (MID_KEY, 0, M64):
            for place in ("start", "end", "middle", "whole"):
                c = pat_run(length, place, key, seed)
                if c is not None:
                    out.append(c)
    return out


# ---- batches ----

K_FIRST, K_LAST, K_ALT, K_ALL, K_OPP = 1000, 1010, 1020, 1030, 1040


def pat_batches(nb, empty_at=None, seed=12):
    """A spine of nb batches: K_FIRST only in batch 0, K_LAST only in the
    last, K_ALT in the even batches, K_ALL in all, K_OPP (nb >= 2) in the
    first and the last with the same v and opposite weights; batch b holds
    b % 3 + 1 rows of each of its keys and five keys of its own.  empty_at:
    that batch is empty instead and keeps its slot."""
    rng = np.random.default_rng(seed)
    batches = []
    for b in range(nb):
        if b == empty_at:
            batches.append(EMPTY.copy())
            continue
        reps = b % 3 + 1
        keys = [K_ALL] * reps
        if b == 0:
            keys += [K_FIRST] * reps
        if b == nb - 1:
            keys += [K_LAST] * reps
        if b % 2 == 0:
            keys += [K_ALT] * reps
        keys += [5000 + 100 * b + j for j in range(5)]
        t = _trace_batch(rng, sorted(keys), b)
        if nb >= 2 and b in (0, nb - 1):
            opp = _rows([K_OPP], [7], [3 if b == 0 else -3])
            t = np.concatenate([t, opp])
            t = t[np.lexsort((t["v"], t["k"]))]
        batches.append(t)
    dkeys = [0, K_FIRST - 1, K_FIRST, K_LAST, K_LAST, K_ALT, K_ALL, K_ALL + 1,
             K_OPP, 5002, 5000 + 100 * (nb - 1), 5000 + 100 * nb + 50, M64]
    where = {None: "", 0: " empty first", nb - 1: " empty last"}.get(
        empty_at, " empty middle")
    return (f"batches nb={nb}{where}", _delta(rng, sorted(dkeys)), batches,
            {"nb": nb, "empty_at": empty_at})


def batch_cases(seed=12):
    out = [pat_batches(nb, None, seed) for nb in NB_GRID]
    for nb in NB_GRID[1:]:
        for at in sorted({0, nb // 2, nb - 1}):
            out.append(pat_batches(nb, at, seed))
    return out


# ---- hot key ----

HOT_RUNS = (3000, 1500, 517)  # one key's rows in the three batches
HOT1, HOT2 = 1 << 20, (1 << 20) + 4096


def pat_hot(shape, zeros, seed=13):
    """One delta row on HOT1, whose 5017 matches lie unevenly in 3 batches,
    with `zeros` zero-match delta rows directly "before" it, "after" it, on
    "both" sides, or "between" it and a second hot row on HOT2; "last": the
    hot row is the delta's last row, behind the zero-match run."""
    rng = np.random.default_rng(seed)
    two = shape == "between"
    batches = []
    for b, n in enumerate(HOT_RUNS):
        keys = [10, 20 + b] + [HOT1] * n
        if two:
            keys += [HOT2] * HOT_RUNS[(b + 1) % 3]
        keys += [HOT2 + 100 + b, HOT2 + 200]
        batches.append(_trace_batch(rng, keys, b))
    z_before = list(range(HOT1 - zeros, HOT1))
    z_after = list(range(HOT1 + 1, HOT1 + 1 + zeros))
    dkeys = [10, 21]
    if shape in ("before", "both", "last"):
        dkeys += z_before
    dkeys.append(HOT1)
    if shape in ("after", "both", "between"):
        dkeys += z_after
    if two:
        dkeys.append(HOT2)
    if shape != "last":
        dkeys += [HOT2 + 101, HOT2 + 150, HOT2 + 200]
    meta = {"shape": shape, "zeros": zeros,
            "hot_row": dkeys.index(HOT1), "nd": len(dkeys)}
    return f"hot {shape} zeros={zeros}", _delta(rng, dkeys), batches, meta


def hot_cases(seed=13):
    return [pat_hot("before", 300, seed), pat_hot("after", 300, seed),
            pat_hot("between", 9, seed), pat_hot("both", 1, seed),
            pat_hot("last", 65, seed)]


# ---- sizes ----

def pat_size(nd, seed=14):
    """nd delta rows on keys 3 i + 1; batch 0 holds one row for every fifth
    delta row, batch 1 two rows for every seventh, and both hold the first
    and the last delta row's key; keys 3 i + 2 match nothing."""
    rng = np.random.default_rng(seed)
    i = np.arange(nd, dtype=np.uint64)
    edge = (i == 0) | (i == nd - 1)
    k0 = np.concatenate([3 * i[(i % 5 == 0) | edge] + 1, 3 * i[i % 11 == 3] + 2])
    i1 = i[(i % 7 == 0) | edge]
    k1 = np.concatenate([3 * i1 + 1, 3 * i1 + 1])
    batches = [_trace_batch(rng, np.sort(k0), 0),
               _trace_batch(rng, np.sort(k1), 1)]
    return f"size nd={nd}", _delta(rng, 3 * i + 1), batches, {"nd": nd}


def size_cases(seed=14):
    return [pat_size(nd, seed) for nd in SIZES_SMALL + SIZES_BIG]


def spine_cases():
    """Every (name, delta, batches, meta) case of the spine join."""
    return run_cases() + batch_cases() + hot_cases() + size_cases()


# ---- projections ----

def _wide(rng, n):
    """Distinct sorted 64-bit-wide vals with both halves busy."""
    v = rng.integers(0, 1 << 63, size=4 * n, dtype=np.uint64) * np.uint64(2) \
        + rng.integers(0, 2, size=4 * n, dtype=np.uint64)
    return np.unique(v)[:n]


def pat_proj_plain(proj, param=0, seed=15):
    """Projections 0..8: 12 keys (0 and 2^64 - 1 among them), 64-bit-wide
    vals on both sides, a two-batch trace.  For the rounding projections
    every fourth val's low half is a multiple of param already."""
    rng = np.random.default_rng(seed + proj)
    keys = np.array([0, 3, 4, 1 << 31, 1 << 32, (1 << 32) + 1, 1 << 40,
                     (1 << 63) - 1, 1 << 63, M64 - 2, M64 - 1, M64],
                    dtype=np.uint64)

    def side(n_per_key, step):
        k = np.repeat(keys[::step], n_per_key)
        v = rng.permutation(_wide(rng, len(k)))
        if param:
            low = v % np.uint64(1 << 32)
            snap = np.arange(len(v)) % 4 == 0
            v = np.where(snap, v - low % np.uint64(param), v)
        r = _rows(k, v, _weights(rng, len(k)))
        return r[np.lexsort((r["v"], r["k"]))]
    delta, b0, b1 = side(3, 1), side(2, 2), side(3, 3)
    return (f"proj {proj} param={param}", delta, [b0, b1],
            {"proj": proj, "param": param})


def _auction_fields(layout):
    bits = dict(layout)
    dt_max, dur_max, tag_max = ((1 << bits[f]) - 1 for f in ("dt", "dur", "tag"))
    return [(0, 0, 0), (0, dur_max, tag_max), (5000, 0, tag_max),
            (5000, dur_max, 0), (dt_max, dur_max, tag_max), (dt_max, 0, 0),
            (77777, 1000, 3)]


PRICE_MAX = (1 << 27) - 1
Q_KEYS = (0, 7, (1 << 60) + 3, M64)


def pat_proj_auction(proj, param, seed=16):
    """Projections 9..12: per auction key, seven auctions with every field at
    0 and at its maximum, and bids at a_dt - 1, a_dt, a_dt + dur and
    a_dt + dur + 1 of each, at prices 0, 12345 and 2^27 - 1.  The delta is
    the bids (9, 11) or the auctions (10, 12); the other side is split over
    two batches row by row.  meta["pairs"]: (key, auction v, bid v, tag,
    price, valid) of every pair at a window edge, from the plain fields."""
    rng = np.random.default_rng(seed + proj)
    layout = AUC4 if proj in (9, 10) else AUC6
    aucs = _auction_fields(layout)
    times = sorted({t for dt, dur, _ in aucs
                    for t in (dt - 1, dt, dt + dur, dt + dur + 1) if t >= 0})
    prices = (0, 12345, PRICE_MAX)
    a_rows, b_rows, pairs = [], [], []
    for key in Q_KEYS:
        for dt, dur, tag in aucs:
            av = pack(layout, dt=dt, dur=dur, tag=tag)
            a_rows.append((key, av))
            for t in (dt - 1, dt, dt + dur, dt + dur + 1):
                if t >= 0:
                    pairs.append((key, av, pack(BID, dt=t, price=12345), tag,
                                  12345, dt <= t <= dt + dur))
        for t in times:
            for p in prices:
                b_rows.append((key, pack(BID, dt=t, price=p)))

    def rows(kv):
        kv = sorted(set(kv))
        return _rows([k for k, _ in kv], [v for _, v in kv],
                     _weights(rng, len(kv)))
    auc, bid = rows(a_rows), rows(b_rows)
    delta, trace = (bid, auc) if proj in (9, 11) else (auc, bid)
    batches = [trace[0::2], trace[1::2]]
    return (f"proj {proj} param={param}", delta, batches,
            {"proj": proj, "param": param, "pairs": pairs,
             "tag_bits": dict(layout)["tag"]})


def proj_cases():
    """(name, delta, batches, meta) with meta["proj"], meta["param"]: all 13
    projections, param in {1, 10000} where it is read."""
    out = [pat_proj_plain(p) for p in (0, 1, 2, 5, 6, 7, 8)]
    out += [pat_proj_plain(p, param) for p in (3, 4) for param in (1, 10000)]
    out += [pat_proj_auction(p, param)
            for p, param in ((9, 1), (10, 10000), (11, 10000), (12, 1))]
    return out


# ---- tail ----

def _plan(delta, batches, proj, **kw):
    return dict(delta=delta, batches=batches, proj=proj, **kw)


def _single_matches(rng, n, base, tag):
    """n delta rows, each matching exactly one trace row."""
    keys = base + 2 * np.arange(n, dtype=np.uint64)
    return _delta(rng, keys), [_trace_batch(rng, keys, tag)]


TAIL_TOTALS = (0, 1, FUSE_THREADS - 1, FUSE_THREADS, FUSE_THREADS + 1,
               FUSE_MAX - 1, FUSE_MAX, FUSE_MAX + 1, TAIL_CAP, TAIL_CAP + 1)


def pat_tail_total(total, cap=TAIL_CAP, seed=21):
    """Two plans whose combined total is exactly `total`: min(total // 2,
    3000) single matches in the first, the rest as one hot row's run over two
    batches between zero-match rows in the second."""
    rng = np.random.default_rng(seed)
    a = min(total // 2, 3000)
    d0, t0 = _single_matches(rng, a, 100, 0)
    rest = total - a
    hot = 1 << 30
    t1 = [_trace_batch(rng, [5] + [hot] * (rest // 3) + [hot + 9], 1),
          _trace_batch(rng, [hot] * (rest - rest // 3) + [hot + 2], 2)]
    d1 = _delta(rng, [hot - 2, hot - 1, hot, hot + 1, hot + 3])
    return (f"tail total={total}", [_plan(d0, t0, 0), _plan(d1, t1, 1)], cap,
            {"total": total})


def pat_tail_cross(stride, last=100, seed=22):
    """Plans of 8192, 8192 and `last` delta rows: combined rows 8191 | 8192
    and 16383 | 16384 are the ends of the offset cells' three buffers
    (last = 8192 fills the third one too).  Every `stride`-th delta row
    matches, and so do the first and the last row of every plan: both sides
    of each crossing."""
    rng = np.random.default_rng(seed)
    plans = []
    for p, n in enumerate((FUSE_MAX, FUSE_MAX, last)):
        i = np.arange(n, dtype=np.uint64)
        keys = 1000 * (p + 1) + 2 * i
        hit = (i % stride == p) | (i == 0) | (i == n - 1)
        plans.append(_plan(_delta(rng, keys),
                           [_trace_batch(rng, keys[hit], 2 * p),
                            _trace_batch(rng, keys[hit & (i % 2 == 0)],
                                         2 * p + 1)], p % 2))
    return (f"tail cross stride={stride} last={last}", plans, TAIL_CAP,
            {"stride": stride, "last": last})


def pat_tail_empty(at, seed=23):
    """Three plans, plan `at` with no delta rows."""
    rng = np.random.default_rng(seed)
    plans = []
    for p in range(3):
        d, t = _single_matches(rng, 0 if p == at else 40 + 300 * p,
                               50 + 5000 * p, p)
        plans.append(_plan(d, t, p % 2))
    return f"tail empty plan {at}", plans, TAIL_CAP, {"empty": at}


def pat_tail_cancel(left, n, seed=24):
    """Two plans whose rows cancel pairwise, under projections 0 and 1 with
    the sides swapped: (k, a, +w) x (k, p, 1) -> (p, a, w) and (k, p, -w) x
    (k, a, 1) -> (p, a, -w).  The first plan emits n rows, the second cancels
    all but `left` of them."""
    k = 10 + 3 * np.arange(n, dtype=np.uint64)
    a = 7 * np.arange(n, dtype=np.uint64) + 1
    p = (np.uint64(1) << np.uint64(40)) + np.arange(n, dtype=np.uint64)
    w = 1 + (np.arange(n) % 3)
    one = np.ones(n, dtype=np.int64)
    m = n - left
    plans = [_plan(_rows(k, a, w), [_rows(k, p, one)], 0),
             _plan(_rows(k[:m], p[:m], -w[:m]), [_rows(k[:m], a[:m], one[:m])],
                   1)]
    return (f"tail cancel n={n} left={left}", plans, TAIL_CAP,
            {"left": left, "n": n})


def pat_tail_poison(kind, at, seed=25):
    """Three healthy plans (the third on a tick-fresh one-batch trace), then
    one length replaced: kind "nd=-1" / "nd=8193" on plan `at`; "tn=-1" /
    "tn=0" / "tn=30" on the fresh plan.  tn = 0 is an empty trace and tn = 30
    a trace shorter than its columns: neither is a poison, and the plan sees
    that many trace rows."""
    rng = np.random.default_rng(seed)
    plans = []
    for p in range(3):
        d, t = _single_matches(rng, 60 + 500 * p, 50 + 5000 * p, p)
        plans.append(_plan(d, t, p % 2))
    plans[2]["fresh"] = True
    if kind.startswith("nd="):
        plans[at]["nd"] = int(kind[3:])
    else:
        assert at == 2
        plans[at]["tn"] = int(kind[3:])
    return f"tail {kind} plan {at}", plans, TAIL_CAP, {"kind": kind, "at": at}


def pat_tail_deep(seed=26):
    """nb = 24 in one plan, nb = 1 in the other."""
    _, d0, b0, _ = pat_batches(MAX_TRACE_BATCHES, 12, seed)
    rng = np.random.default_rng(seed)
    d1, t1 = _single_matches(rng, 300, 77, 30)
    return ("tail nb=24 and nb=1", [_plan(d0, b0, 1), _plan(d1, t1, 0)],
            TAIL_CAP, {})


def pat_tail_size(nd, seed=27):
    """One plan on the size pattern of nd delta rows."""
    _, delta, batches, _ = pat_size(nd, seed)
    return f"tail nd={nd}", [_plan(delta, batches, 0)], TAIL_CAP, {"nd": nd}


def tail_cases():
    out = [pat_tail_total(t) for t in TAIL_TOTALS]
    out += [pat_tail_size(nd) for nd in SIZES_SMALL]
    out += [pat_tail_cross(97), pat_tail_cross(5), pat_tail_cross(97, FUSE_MAX)]
    out += [pat_tail_empty(at) for at in range(3)]
    out += [pat_tail_cancel(left, n) for n in (400, 1500) for left in (0, 1)]
    out += [pat_tail_poison(kind, at) for kind in ("nd=-1", "nd=8193")
            for at in range(3)]
    out += [pat_tail_poison(kind, 2) for kind in ("tn=-1", "tn=0", "tn=30")]
    out.append(pat_tail_deep())
    return out
