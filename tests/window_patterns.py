"""Pattern builders and CPU references for the window stage: the device
watermark (`Ctx.wm_update`) and the ranges / emit pair over a spine
(`Ctx.window_spine`, host bounds or chained behind the watermark).

`ref_wm` is written from queries/q5.rs:85-96 and q8.rs:62-71 in Python ints;
`ref_window_spine` from operator/time_series/window.rs:144-220 with
np.searchsorted.  Neither shares anything with the kernels or the C++ oracle.
Every builder is deterministic and returns a list of cases (dicts with at
least "name", "batches", "tick", "bounds" = (s0, e0, s1, e1, have_prev)).
Nothing here needs a GPU."""
import functools

import numpy as np

from dbsp_amd import ROW_DT

M64 = (1 << 64) - 1
MAX_TRACE_BATCHES = 24  # kernels_iface.hpp
BLK = 256               # threads of an emit block
GRID_CAP = 16384        # grid_for's block cap (kernels.hip)
RUN_LENGTHS = (1, 2, 255, 256, 257)
BOUND_NAMES = ("s0", "e0", "s1", "e1")
# the overlapping slide the run patterns sit on
BASE = {"s0": 1000, "e0": 7000, "s1": 3000, "e1": 9000}

Q5 = (10000, 2000, 4000)    # (width, tumble, lag), queries/q5.rs:73-87
Q8 = (10000, 10000, 10000)  # queries/q8.rs:46-71
LAG0 = (10000, 2000, 0)
WM_PARAMS = {"q5": Q5, "q8": Q8, "lag0": LAG0}


def _rows(k, v, w):
    out = np.empty(len(k), dtype=ROW_DT)
    out["k"] = np.asarray(k, dtype=np.uint64)
    out["v"] = np.asarray(v, dtype=np.uint64)
    out["w"] = np.asarray(w, dtype=np.int64)
    return out


EMPTY = _rows([], [], [])


def batch_of(runs, seed=0):
    """A consolidated batch from [(key, run length)], keys ascending: within
    a run the vals ascend, the weights are non-zero and of both signs."""
    keys = [int(k) for k, _ in runs]
    assert keys == sorted(set(keys)), "keys ascend"
    lens = np.array([n for _, n in runs], dtype=np.int64)
    n = int(lens.sum())
    if n == 0:
        return EMPTY
    k = np.repeat(np.array(keys, dtype=np.uint64), lens)
    start = np.repeat(np.cumsum(lens) - lens, lens)
    j = np.arange(n, dtype=np.int64) - start
    v = (j * 3 + seed).astype(np.uint64)
    w = (np.arange(n, dtype=np.int64) * 7 + seed) % 5 - 2
    w[w == 0] = 3
    return _rows(k, v, w)


def run_lengths(batch, key):
    return int(np.count_nonzero(batch["k"] == np.uint64(key)))


# ---- the references ----

def ref_wm(state, gmax, width, tumble, lag):
    """One watermark step.  state = (wm, s0, e0, have_prev); gmax: the tick's
    max event time, None or 0 when it has none.  Returns (state after, the 6
    bounds words).  watermark_monotonic keeps the max of date_time - lag;
    the window is [rounded - width saturating at 0, rounded)."""
    wm, s0, e0, have_prev = (int(x) for x in state)
    if gmax:
        assert gmax >= lag, "below lag the reference itself overflows"
        wm = max(wm, int(gmax) - lag)
    rounded = wm - wm % tumble
    s1 = rounded - width if rounded >= width else 0
    return (wm, s1, rounded, 1), [s0, e0, s1, rounded, have_prev, 0]


def model_wm(state, gmax, width, tumble, lag, variant):
    """Wrong watermarks: "round_first" keeps the rounded candidate as the
    watermark, "no_saturate" lets the start wrap."""
    wm, s0, e0, have_prev = (int(x) for x in state)
    if gmax:
        cand = int(gmax) - lag
        if variant == "round_first":
            cand -= cand % tumble
        wm = max(wm, cand)
    rounded = wm - wm % tumble
    s1 = rounded - width if rounded >= width else 0
    if variant == "no_saturate":
        s1 = (rounded - width) & M64
    return (wm, s1, rounded, 1), [s0, e0, s1, rounded, have_prev, 0]


def _seek(keys, bound, upper):
    return int(np.searchsorted(keys, np.uint64(bound),
                               side="right" if upper else "left"))


def ref_window_spine(batches, tick, have_prev, s0, e0, s1, e1, upper=()):
    """(table, rows): the region table (nreg x 5 int64: src, lo, len, sign,
    goff; src -1 = the tick batch) and the rows in table order.  Each cursor
    walk of Window::eval is a seek to the region's first bound and a run
    while key < its second.  `upper` names bounds sought with upper_bound
    instead: the wrong variants the patterns must tell from the right one."""
    def span(keys, a, b):
        (av, an), (bv, bn) = a, b
        lo = _seek(keys, av, an in upper)
        return lo, max(_seek(keys, bv, bn in upper) - lo, 0)

    S0, E0, S1, E1 = (s0, "s0"), (e0, "e0"), (s1, "s1"), (e1, "e1")
    regions = []
    for b, t in enumerate(batches):
        keys = np.ascontiguousarray(t["k"])
        r1 = r2 = r3 = (0, 0)
        if have_prev:
            # region 1: from s0 while key < s1 and key < e0
            r1 = span(keys, S0, S1 if s1 < e0 else E0)
            if e1 < e0:  # the window shrank on the right
                r2 = span(keys, E1, E0)
            # region 3: from max(e0, s1) while key < e1
            r3 = span(keys, E0 if e0 >= s1 else S1, E1)
        regions += [(b,) + r1 + (-1,), (b,) + r2 + (-1,), (b,) + r3 + (1,)]
    regions.append((-1,) + span(np.ascontiguousarray(tick["k"]), S1, E1)
                   + (1,))
    table = np.zeros((len(regions), 5), dtype=np.int64)
    parts, goff = [], 0
    for r, (src, lo, ln, sign) in enumerate(regions):
        table[r] = (src, lo, ln, sign, goff)
        goff += ln
        if ln:
            part = (tick if src < 0 else batches[src])[lo:lo + ln].copy()
            part["w"] *= sign
            parts.append(part)
    rows = np.concatenate(parts) if parts else EMPTY.copy()
    return table, rows


def table_diff(got, exp):
    """None when the tables agree, else a message.  The start and sign of an
    empty region name no row, so they are compared where len > 0 only."""
    if got.shape != exp.shape:
        return f"shape {got.shape} vs {exp.shape}"
    for r in range(len(exp)):
        cols = (0, 1, 2, 3, 4) if exp[r, 2] > 0 or got[r, 2] > 0 else (0, 2, 4)
        for c in cols:
            if got[r, c] != exp[r, c]:
                return (f"region {r} word {c}: {got[r, c]} vs {exp[r, c]} "
                        f"(got {got[r]}, expected {exp[r]})")
    return None


def model_emit_regions(table, total, strict=False):
    """The region of every output row by the emit's search over goff: the
    last region whose offset is <= o (strict: < o, the wrong variant; -1
    where it falls off the table)."""
    o = np.arange(total, dtype=np.int64)
    return np.searchsorted(table[:, 4], o,
                           side="left" if strict else "right") - 1


def ref_chain(batches, tick, chain):
    """The chained route: k_wm_update fed by the tick's first wm_n keys, then
    the ranges reading the published bounds and the device length bn.
    Returns dict(total, table, rows, bounds, state)."""
    wm_n = chain.get("wm_n", len(tick))
    bn = chain.get("bn", len(tick))
    state = tuple(int(x) for x in chain["state"])
    if wm_n < 0:  # err: state untouched, only the err word written
        return {"total": -1, "table": None, "rows": EMPTY, "state": list(state),
                "bounds": [0, 0, 0, 0, 0, 1]}
    gmax = int(tick["k"][wm_n - 1]) if wm_n > 0 else None
    state, bounds = ref_wm(state, gmax, chain["width"], chain["tumble"],
                           chain["lag"])
    out = {"state": list(state), "bounds": bounds}
    if bn < 0:
        out.update(total=-1, table=None, rows=EMPTY)
        return out
    s0, e0, s1, e1, have_prev, _ = bounds
    table, rows = ref_window_spine(batches, tick[:bn], have_prev, s0, e0, s1,
                                   e1)
    out.update(total=len(rows), table=table, rows=rows)
    return out


def chain_for(case, bn=None):
    """The chained form of a host-bounds case: a watermark already at e1, a
    lag that takes the tick's maximum down to 0, tumble 1 and width e1 - s1,
    so the device publishes exactly the case's bounds."""
    s0, e0, s1, e1, have_prev = case["bounds"]
    tick = case["tick"]
    n = len(tick) if bn is None else bn
    lag = int(tick["k"][n - 1]) if n > 0 else 0
    ch = {"state": (e1, s0, e0, have_prev), "width": e1 - s1, "tumble": 1,
          "lag": lag}
    if bn is not None:
        ch["wm_n"] = ch["bn"] = bn
    return ch


def zset_rows(rows):
    """Rows consolidated: sorted by (k, v), weights of equal pairs summed,
    zeros dropped."""
    r = np.asarray(rows, dtype=ROW_DT)
    if len(r) == 0:
        return r
    r = r[np.lexsort((r["v"], r["k"]))]
    head = np.ones(len(r), dtype=bool)
    head[1:] = (r["k"][1:] != r["k"][:-1]) | (r["v"][1:] != r["v"][:-1])
    sums = np.add.reduceat(r["w"], np.flatnonzero(head))
    out = r[head].copy()
    out["w"] = sums
    return out[sums != 0]


# ---- the patterns ----

def _case(name, batches, tick, bounds, **meta):
    s0, e0, s1, e1, _ = bounds
    assert s0 <= s1 <= e1 and s0 <= e0, (name, bounds)
    assert len(batches) <= MAX_TRACE_BATCHES
    return {"name": name, "batches": list(batches), "tick": tick,
            "bounds": tuple(bounds), "meta": meta}


def _run_batch(key, length, place, seed):
    """A batch with `length` rows of `key` at its start, middle or end; the
    neighbouring keys key-1 / key+1 hold one row each where the place leaves
    room for them."""
    below = [(key - 900, 2), (key - 400, 1), (key - 1, 1)]
    above = [(key + 1, 1), (key + 300, 3), (key + 800, 1)]
    runs = [(key, length)]
    if place in ("middle", "end"):
        runs = below + runs
    if place in ("middle", "start"):
        runs = runs + above
    return batch_of(runs, seed)


@functools.lru_cache(maxsize=None)
def run_cases():
    """Each bound in turn on, just below and just above a key carried by a
    run of 1, 2, 255, 256 or 257 rows at the start, middle and end of its
    batch; a second trace batch and the tick batch carry the same run."""
    spread = batch_of([(k, 1 + k % 3) for k in range(100, 10000, 613)], 5)
    out = []
    for which in BOUND_NAMES:
        key = BASE[which]
        for length in RUN_LENGTHS:
            for place in ("start", "middle", "end"):
                for off in (-1, 0, 1):
                    b = dict(BASE)
                    b[which] = key + off
                    batches = [_run_batch(key, length, place, 1), spread,
                               _run_batch(key, length, "middle", 2)]
                    tick = _run_batch(key, length, place, 4)
                    out.append(_case(
                        f"run-{which}{off:+d}-L{length}-{place}", batches,
                        tick, (b["s0"], b["e0"], b["s1"], b["e1"], 1),
                        which=which, key=key, length=length, place=place,
                        off=off))
    return out


def _shape_trace():
    t0 = batch_of([(0, 2)] + [(k, 1 + k % 4) for k in range(250, 12000, 250)]
                  + [(M64 - 1, 2), (M64, 3)], 1)
    t1 = batch_of([(k, 2) for k in range(125, 12000, 500)], 2)
    t2 = batch_of([(0, 1), (3000, 4), (7000, 4), (9000, 4), (M64 - 1, 1)], 3)
    tick = batch_of([(0, 1), (2999, 1), (3000, 2), (5000, 1), (6999, 1),
                     (7000, 1), (8999, 2), (9000, 1), (M64 - 1, 1),
                     (M64, 1)], 6)
    return [t0, t1, t2], tick


SHAPES = {
    "slide": (1000, 7000, 3000, 9000, 1),         # s1 < e0
    "jump": (1000, 3000, 5000, 9000, 1),          # s1 > e0
    "jump-exact": (1000, 5000, 5000, 9000, 1),    # s1 == e0
    "shrink": (1000, 9000, 3000, 7000, 1),        # e1 < e0
    "shrink-to-start": (1000, 9000, 3000, 3000, 1),
    "unchanged": (3000, 9000, 3000, 9000, 1),
    "empty-new": (1000, 7000, 9000, 9000, 1),     # s1 == e1
    "empty-old": (3000, 3000, 3000, 9000, 1),     # s0 == e0
    "first": (0, 0, 3000, 9000, 0),               # no previous window
    "start-0": (0, 5000, 0, 9000, 1),             # s1 = 0, key 0 inside
    "first-saturated": (0, 0, 0, 4000, 1),        # the start saturated at 0
    "end-max": (1000, 7000, 3000, M64, 1),        # 2^64-2 in, 2^64-1 out
}


@functools.lru_cache(maxsize=None)
def shape_cases():
    batches, tick = _shape_trace()
    return [_case(f"shape-{name}", batches, tick, b, shape=name)
            for name, b in SHAPES.items()]


@functools.lru_cache(maxsize=None)
def spine_cases():
    b = SHAPES["slide"]
    s0, e0, s1, e1, _ = b
    inside = batch_of([(k, 2) for k in range(s1, e0, 400)], 1)   # [s1, e0)
    below = batch_of([(k, 1) for k in range(0, s0, 100)], 2)
    above = batch_of([(k, 1) for k in range(e1, e1 + 1000, 100)], 3)
    mixed = batch_of([(k, 1 + k % 3) for k in range(500, 11000, 500)], 4)
    tick = batch_of([(k, 1) for k in range(2500, 9500, 700)], 5)
    neg = mixed.copy()
    neg["w"] = -neg["w"]
    out = [
        _case("spine-nb1", [mixed], tick, b, nb=1),
        _case("spine-nb2", [mixed, inside], tick, b, nb=2),
        _case("spine-nb3-below-inside-above", [below, inside, above], tick, b,
              nb=3),
        _case("spine-one-empty", [mixed, EMPTY, inside], tick, b, nb=3),
        _case("spine-all-empty", [EMPTY, EMPTY, EMPTY], tick, b, nb=3),
        _case("spine-nb0", [], tick, b, nb=0),
        _case("spine-empty-tick", [mixed, inside], EMPTY, b, nb=2),
        _case("spine-opposite-weights", [mixed, neg], tick, b, nb=2),
        _case("spine-nb24", [batch_of([(k, 1 + (k + i) % 3) for k in
                                       range(100 + 37 * i, 11000, 900)], i)
                             for i in range(24)], tick, b, nb=24),
        _case("spine-nb24-some-empty",
              [EMPTY if i % 5 == 0 else
               batch_of([(k, 2) for k in range(50 * i, 11000, 1300)], i)
               for i in range(24)], tick, b, nb=24),
    ]
    return out


def _only(regions, lengths=None, nb=MAX_TRACE_BATCHES, bounds=None):
    """nb batches whose rows fall in the named regions only: a region is
    (batch, which) with which 0 = retract, 1 = shrink, 2 = insert, or "tick".
    Rows of every other batch, and of the tick, lie outside both windows."""
    s0, e0, s1, e1, _ = bounds
    lengths = lengths or {}
    want = {}
    for reg in regions:
        want.setdefault(reg if reg == "tick" else reg[0], []).append(reg)

    def keys_for(reg, n):
        if reg == "tick" or reg[1] == 2:
            lo = s1 if reg == "tick" else max(e0, s1)
            return [(lo + i, 1) for i in range(n)]
        lo = s0 if reg[1] == 0 else e1
        return [(lo + i, 1) for i in range(n)]

    def build(owner, seed):
        runs = [(e0 + e1 + 10 + seed, 1)]  # above both windows
        for reg in want.get(owner, []):
            runs += keys_for(reg, lengths.get(reg, 3))
        return batch_of(sorted(runs), seed)

    return [build(b, b) for b in range(nb)], build("tick", 99)


@functools.lru_cache(maxsize=None)
def emit_cases():
    """Region tables the emit's search must walk: long stretches of empty
    regions (equal goff) before, between and after the occupied ones."""
    nb = MAX_TRACE_BATCHES
    slide, shrink = SHAPES["slide"], SHAPES["shrink"]
    out = []

    def add(name, regions, bounds, lengths=None, nb_=nb):
        batches, tick = _only(regions, lengths, nb_, bounds)
        out.append(_case(name, batches, tick, bounds, regions=list(regions),
                         lengths=dict(lengths or {})))

    add("emit-only-region-0", [(0, 0)], slide)
    add("emit-only-last-trace-region", [(nb - 1, 2)], slide)
    add("emit-only-tick", ["tick"], slide)
    add("emit-every-third-retract", [(b, 0) for b in range(nb)], slide)
    add("emit-every-third-insert", [(b, 2) for b in range(nb)], slide)
    add("emit-every-third-shrink", [(b, 1) for b in range(nb)], shrink)
    add("emit-every-third-batch", [(b, 2) for b in range(0, nb, 3)], slide)
    regs = [(b, w) for b in range(nb) for w in (0, 2)] + ["tick"]
    add("emit-len1-retract-insert", regs, slide, {r: 1 for r in regs})
    regs = [(b, w) for b in range(nb) for w in (0, 1)] + ["tick"]
    add("emit-len1-retract-shrink", regs, shrink, {r: 1 for r in regs})
    for total in (1, 255, 256, 257):
        half = total // 2
        regs = ([(1, 0)] if half else []) + ["tick"]
        add(f"emit-total-{total}", regs, slide,
            {(1, 0): half, "tick": total - half}, nb_=3)
    return out


GRID_TOTAL = GRID_CAP * BLK + 257


@functools.lru_cache(maxsize=None)
def grid_case():
    """A total one past what a capped grid covers in one sweep, from a
    two-batch trace: the emit's grid-stride loop takes a second turn."""
    s0, e0, s1, e1, _ = b = (0, 10, 10, 1 << 40, 1)
    n0 = GRID_TOTAL - 257 - 5
    k0 = np.arange(n0, dtype=np.uint64) // np.uint64(3) + np.uint64(e0)
    t0 = _rows(k0, np.arange(n0, dtype=np.uint64) % np.uint64(3),
               np.arange(n0, dtype=np.int64) % 3 + 1)
    t1 = batch_of([(2, 5)] + [(1000 + 2 * i, 1) for i in range(250)], 1)
    tick = batch_of([(5, 1)] + [(77 + 3 * i, 1) for i in range(7)], 2)
    return _case("emit-grid-stride", [t0, t1], tick, b, total=GRID_TOTAL)


@functools.lru_cache(maxsize=None)
def chain_cases():
    """The chained route's own edges: the tick batch's device length equal to
    it, shorter (the rows past it lie inside the window), zero, negative, and
    an err watermark.  Each is dict(name, batches, tick, chain)."""
    batches, _ = _shape_trace()
    batches = batches[:2]
    # sorted keys, all inside [s1, e1) = [3000, 9000)
    tick = batch_of([(k, 1 + k % 2) for k in range(3100, 8900, 200)], 7)
    base = _case("chain", batches, tick, SHAPES["slide"])
    full = len(tick)
    out = []
    for name, bn in (("equal", full), ("shorter", full - 9), ("one", 1),
                     ("zero", 0)):
        out.append({"name": f"chain-len-{name}", "batches": batches,
                    "tick": tick, "chain": chain_for(base, bn)})
    ch = chain_for(base, full)
    ch["bn"] = -1
    out.append({"name": "chain-len-negative", "batches": batches,
                "tick": tick, "chain": ch})
    ch = chain_for(base, full)
    ch["wm_n"] = -1
    out.append({"name": "chain-err-watermark", "batches": batches,
                "tick": tick, "chain": ch})
    # q5's and q8's own parameters moving a real watermark
    for pname, (width, tumble, lag) in WM_PARAMS.items():
        t = batch_of([(k, 1) for k in range(20000, 61000, 1500)], 8)
        out.append({"name": f"chain-{pname}-advance",
                    "batches": [batch_of([(k, 2) for k in
                                          range(15000, 60000, 900)], 9),
                                batch_of([(k, 1) for k in
                                          range(30000, 50000, 333)], 10)],
                    "tick": t,
                    "chain": {"state": (33000 + lag // 2, 22000, 32000, 1),
                              "width": width, "tumble": tumble, "lag": lag}})
    return out


def wm_sequences():
    """(name, (width, tumble, lag), ticks): each tick the max event time or
    None for an empty tick, replayed from the zero state.  Together: a first
    tick that is empty and one that is not, gmax == lag, the watermark one
    below, on and one above a tumble multiple, a late tick, an empty tick in
    mid-stream, a rounded watermark below, at and above the width, a zero
    maximum and 2^64-1."""
    out = []
    for pname, p in WM_PARAMS.items():
        width, tumble, lag = p
        ticks = [None, lag, lag + tumble - 1, lag + tumble, lag + tumble + 1,
                 lag + 1, None, lag + width - 1, lag + width,
                 lag + width + tumble, lag + width + tumble + 1, 0,
                 lag + 7 * width + tumble // 2, M64]
        out.append((f"wm-{pname}-walk", p, [t for t in ticks
                                            if t is None or t == 0 or
                                            t >= max(lag, 1)]))
        out.append((f"wm-{pname}-first-nonempty", p,
                    [lag + 3 * width + 7, None, lag + 3 * width + 8]))
    return out
