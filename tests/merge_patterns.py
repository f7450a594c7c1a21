"""Row and pattern builders shared by the accumulator-fold and the merge
tests, the size grid of the merge's three bands, and CPU models of the merge.

Every pattern takes (na, nb) and returns two consolidated batches (A, B), or
None when the pair cannot form it.  Nothing here needs a GPU."""
import numpy as np

from dbsp_amd import ROW_DT

M64 = (1 << 64) - 1
BASE = 1 << 20     # A's keys are BASE + 10 * i: room below, between and above
ABOVE = 1 << 40
PI = float(np.pi)

# merge_batches (engine.cpp) dispatches on na + nb
SMALL_MAX = 4096     # k_merge_small: one workgroup
MID_MAX = 32768      # k_merge_mid_fused; above it the merge-path kernels
FUSE_THREADS = 1024  # thread diagonals of k_merge_small (kernels.hip)
MERGE_MID_WGS = 32   # workgroup slices of k_merge_mid_fused (kernels.hip)
MP_TILE = 1024       # k_mp_partition / k_mp_merge_onepass tile (kernels.hip)

# the smallest (na, nb) at which each kernel's splitting changes shape
GRID = {
    "small": [(0, 0), (0, 1), (1, 0), (1, 1), (1023, 1), (1024, 1024),
              (2048, 2047), (2048, 2048), (3072, 1024), (4095, 1), (1, 4095)],
    "mid": [(2049, 2048), (4096, 1), (1, 4096), (4097, 0), (0, 4097),
            (8192, 8192), (24576, 8192), (16384, 16383), (16384, 16384),
            (32767, 1), (1, 32767)],
    # (16896, 16896) is exactly 33 tiles, (16897, 16896) one row more
    "merge_path": [(16385, 16384), (32768, 1), (1, 32768), (32769, 0),
                   (0, 32769), (16896, 16896), (16897, 16896), (50000, 15537),
                   (65536, 3)],
}


def band_of(total):
    if total <= SMALL_MAX:
        return "small"
    return "mid" if total <= MID_MAX else "merge_path"


def _rows(k, v, w):
    out = np.empty(len(k), dtype=ROW_DT)
    out["k"] = np.asarray(k, dtype=np.uint64)
    out["v"] = np.asarray(v, dtype=np.uint64)
    out["w"] = np.asarray(w, dtype=np.int64)
    return out


def _acc(na):
    i = np.arange(na, dtype=np.uint64)
    return _rows(BASE + 10 * i, i % 3, 1 + (i % 5).astype(np.int64))


def _sorted_distinct(r):
    if len(r) < 2:
        return True
    k, v = r["k"], r["v"]
    return bool(np.all((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1]))))


def _spread(na, nb):
    """nb distinct A indices, evenly spread (needs nb <= na)."""
    return (np.arange(nb, dtype=np.int64) * na) // nb


# ---- patterns: (na, nb) -> (A, B) or None when the pair cannot form it ----

def pat_interleaved(na, nb):
    a = _acc(na)
    j = np.arange(nb, dtype=np.uint64)
    gap = (j * np.uint64(na + 1)) // np.uint64(max(nb, 1))  # 0..na
    # between A[gap-1] and A[gap]; rows sharing a gap differ in v
    return a, _rows(BASE + 10 * gap - 5, j, 1 + (j % 3).astype(np.int64))


def pat_below(na, nb):
    j = np.arange(nb, dtype=np.uint64)
    return _acc(na), _rows(j, j % 2, np.full(nb, -3))


def pat_above(na, nb):
    j = np.arange(nb, dtype=np.uint64)
    return _acc(na), _rows(ABOVE + j, j % 2, np.full(nb, 7))


def pat_all_match(na, nb):
    if nb > na:
        return None
    a = _acc(na)
    t = a[_spread(na, nb)]
    return a, _rows(t["k"], t["v"], np.full(nb, 2))


def pat_all_cancel(na, nb):
    if nb > na:
        return None
    a = _acc(na)
    t = a[_spread(na, nb)]
    return a, _rows(t["k"], t["v"], -t["w"])


def _pat_runs(na, nb, final):
    size = 4 if final else 3
    groups = nb // size
    if groups == 0 or groups > na:
        return None
    a = _acc(na)
    t = a[_spread(na, groups)]
    k, v, w = [], [], []
    for r in t:
        kk = int(r["k"])
        k += [kk - 3, kk - 2, kk - 1]
        v += [5, 0, 9]
        w += [1, -1, 2]
        if final:  # alternately a surviving and a cancelling match
            k.append(kk)
            v.append(int(r["v"]))
            w.append(-int(r["w"]) if (kk // 10) % 2 else 4)
    rest = nb - groups * size  # the remainder shares the bound na
    k += [ABOVE + x for x in range(rest)]
    v += [0] * rest
    w += [1] * rest
    return a, _rows(k, v, w)


def pat_runs_open(na, nb):
    return _pat_runs(na, nb, final=False)


def pat_runs_final_equal(na, nb):
    return _pat_runs(na, nb, final=True)


def pat_same_key(na, nb):
    """Four A rows per key, v = 0, 4, 8, 12; B alternates an insertion just
    above a row's v and a match of the row."""
    if nb > na:
        return None
    i = np.arange(na, dtype=np.uint64)
    a = _rows(BASE + i // 4, 4 * (i % 4), 1 + (i % 5).astype(np.int64))
    t = a[_spread(na, nb)]
    odd = np.arange(nb) % 2 == 1
    return a, _rows(t["k"], np.where(odd, t["v"], t["v"] + 1),
                    np.where(odd, np.where(np.arange(nb) % 4 == 1, -t["w"], 3),
                             1))


def pat_extremes(na, nb):
    a = _acc(na)
    if na >= 1:
        a[0] = (0, 0, 2)
    if na >= 2:
        a[-1] = (M64, M64, 3)
    cand = [(0, 0, 5), (0, 1, 1), (M64, M64 - 1, 1), (M64, M64, -3)]
    take = cand[:nb] if nb < 4 else cand
    mid = nb - len(take)
    j = np.arange(mid, dtype=np.uint64)
    gap = 1 + (j * np.uint64(max(na - 2, 0))) // np.uint64(max(mid, 1))
    b = _rows([0] * 0, [], [])
    rows_mid = _rows(BASE + 10 * gap - 5, j, np.full(mid, 1))
    lo = [r for r in take if r[0] == 0]
    hi = [r for r in take if r[0] == M64]
    b = np.concatenate([_rows(*zip(*lo)) if lo else b, rows_mid,
                        _rows(*zip(*hi)) if hi else b])
    return a, b


def pat_straddle(na, nb, diagonals, off, below=False):
    """Equal pairs placed on cut positions.  Every B row placed here equals
    an A row; with a-first ties the b-half of a match on A[i] that follows j
    earlier matches lands at merged position i + 1 + j, so pair j matches
    A[d_j + off - 1 - j] to put its b-half at d_j + off (the same position
    holds the second half when the sides are swapped).  off = 0 puts the cut
    d_j exactly between the two halves, off = -1 / +1 put the whole pair just
    before / just after it.  Of the sorted diagonals those less than 2 past
    the previous one are skipped.  Weights alternate between cancelling and
    surviving; what is left of nb goes above all of A.  With below=True it
    goes below all of A instead and moves every pair up by that many
    positions, which brings the late cuts within reach.  None if nb is
    smaller than the number of diagonals or an index leaves [0, na)."""
    ds = []
    for d in sorted(diagonals):
        if not ds or d - ds[-1] >= 2:
            ds.append(d)
    if nb < len(ds):
        return None
    lead = nb - len(ds) if below else 0
    idx = np.array([d + off - 1 - j - lead for j, d in enumerate(ds)],
                   dtype=np.int64)
    if len(idx) and (idx[0] < 0 or idx[-1] >= na):
        return None
    a = _acc(na)
    t = a[idx]
    cancel = np.arange(len(ds)) % 2 == 0
    rest = np.arange(nb - len(ds), dtype=np.uint64)
    pairs = _rows(t["k"], t["v"], np.where(cancel, -t["w"], 6))
    if below:
        return a, np.concatenate([_rows(rest, rest % 2,
                                        np.full(len(rest), 1)), pairs])
    return a, np.concatenate([pairs, _rows(ABOVE + rest, rest % 2,
                                           np.full(len(rest), 1))])


def pat_high_bits(na, nb):
    """First half: interleaved rows whose keys differ only in bits 32..63
    (A holds the odd multiples of 2^32, B the even ones).  Second half: one
    key for all rows, which are ordered by v alone; v runs over x and
    x | 2^63, so the two groups differ only in bit 63."""
    low = 0x9E3779B9
    na2, nb2 = na // 2, nb // 2
    na1, nb1 = na - na2, nb - nb2
    i = np.arange(na1, dtype=np.uint64)
    j = np.arange(nb1, dtype=np.uint64)
    gap = (j * np.uint64(na1 + 1)) // np.uint64(max(nb1, 1))  # 0..na1
    first = np.searchsorted(gap, gap).astype(np.uint64)  # rows sharing a gap
    a1 = _rows(((2 * i + 1) << np.uint64(32)) | np.uint64(low),
               np.full(na1, 7), 1 + (i % 5).astype(np.int64))
    b1 = _rows(((2 * gap) << np.uint64(32)) | np.uint64(low),
               7 + j - first, 1 + (j % 3).astype(np.int64))
    n2 = na2 + nb2
    half = max((n2 + 1) // 2, 1)
    m = np.arange(n2, dtype=np.uint64)
    v2 = (m % np.uint64(half)) | ((m // np.uint64(half)) << np.uint64(63))
    in_b = np.zeros(n2, dtype=bool)
    if nb2:
        in_b[_spread(n2, nb2)] = True
    key2 = (0xFFFFFFFF << 32) | low
    va, vb = v2[~in_b], v2[in_b]
    a2 = _rows(np.full(na2, key2, dtype=np.uint64), va,
               2 + (np.arange(na2) % 3))
    b2 = _rows(np.full(nb2, key2, dtype=np.uint64), vb,
               -1 - (np.arange(nb2) % 2))
    return np.concatenate([a1, a2]), np.concatenate([b1, b2])


# ---- where the kernels cut the merged sequence ----

def boundaries(total):
    """The coarse cut positions (merged-sequence diagonals) of the band that
    `total` = na + nb falls in (merge_batches in engine.cpp: <= 4096 small,
    <= 32768 mid, merge-path above):
      small       k_merge_small: FUSE_THREADS = 1024 thread diagonals at
                  t * ceil(total / 1024)
      mid         k_merge_mid_fused: MERGE_MID_WGS = 32 workgroup slices
                  starting at w * ceil(total / 32), w = 1..31
      merge-path  k_mp_partition: tiles of MP_TILE = 1024 rows, at t * 1024
    Positions 0 and >= total cut nothing and are left out.  Of more than 64
    positions the first 32, the middle one and the last 31 are kept."""
    if total <= SMALL_MAX:
        step = -(-total // FUSE_THREADS)
    elif total <= MID_MAX:
        step = -(-total // MERGE_MID_WGS)
    else:
        step = MP_TILE
    cuts = list(range(step, total, step)) if step else []
    if len(cuts) > 64:
        cuts = cuts[:32] + [cuts[len(cuts) // 2]] + cuts[-31:]
    return cuts


def straddle_cuts(na, nb, off, below=False):
    """The cuts of boundaries(na + nb) that pat_straddle can reach, in the
    form it takes them.  A pair's first half is an A row: with the rest of B
    above all of A, pair j reaches no cut past na + j, and with it below, the
    r-th pair from the end reaches none before nb - r.  A cut next to
    another one is left out, because a control pair one position off it
    would straddle the neighbour.  None when no cut is left."""
    cuts = boundaries(na + nb)
    have = set(cuts)
    ds = []
    for d in (reversed(cuts) if below else cuts):
        r = len(ds)
        if d - 1 in have or d + 1 in have or (ds and abs(d - ds[-1]) < 2):
            continue
        i = d + off - nb + r if below else d + off - 1 - r
        if r < nb and 0 <= i < na:
            ds.append(d)
    return sorted(ds) or None


def pat_straddle_at(off, below=False):
    def pat(na, nb):
        ds = straddle_cuts(na, nb, off, below)
        return None if ds is None else pat_straddle(na, nb, ds, off, below)
    pat.__name__ = ("pat_straddle_" + {-1: "before", 0: "on", 1: "after"}[off]
                    + ("_late" if below else ""))
    return pat


MOVED = [pat_interleaved, pat_below, pat_above, pat_all_match, pat_all_cancel,
         pat_runs_open, pat_runs_final_equal, pat_same_key, pat_extremes]
MERGE_PATTERNS = (MOVED + [pat_high_bits]
                  + [pat_straddle_at(o) for o in (-1, 0, 1)]
                  + [pat_straddle_at(o, below=True) for o in (-1, 0, 1)])


# ---- CPU models ----

def f64_twin(r, scale):
    """The same keys with f64 weights w * scale (as bit patterns).  IEEE
    multiplication is sign-symmetric, so rows that cancel as integers are
    exact negations of each other here too."""
    out = r.copy()
    out["w"] = (r["w"].astype(np.float64) * scale).view(np.int64)
    return out


def kv_scale(r):
    """A finite scale per row that depends on (k, v) alone, spread over 40
    binades: f64_twin(r, kv_scale(r)) has irregular weights and still
    negates exactly where the integers cancel."""
    k, v = r["k"], r["v"]
    frac = ((k ^ (v * np.uint64(31))) % np.uint64(997)).astype(np.float64)
    return np.ldexp(1.0 + frac / 997.0,
                    ((k + v) % np.uint64(41)).astype(np.int64) - 20)


def numpy_merge(a, b, f64=False):
    """Independent model of the merge: concatenate, np.unique on (k, v), sum
    the weights per pair with np.add.at, drop the zero sums."""
    both = np.concatenate([a, b])
    if len(both) == 0:
        return both
    kv = np.empty(len(both), dtype=[("k", "<u8"), ("v", "<u8")])
    kv["k"], kv["v"] = both["k"], both["v"]
    uniq, inv = np.unique(kv, return_inverse=True)
    w = both["w"].view(np.float64) if f64 else both["w"]
    acc = np.zeros(len(uniq), dtype=w.dtype)
    np.add.at(acc, inv.reshape(-1), w)
    keep = acc != 0
    return _rows(uniq["k"][keep], uniq["v"][keep], acc[keep].view(np.int64))


def sliced_merge_no_adjust(a, b, cuts):
    """The bug the straddle patterns are there to catch: the merged sequence
    (a-first on ties) is cut at the plain merge-path diagonals `cuts`, with
    no adjustment, and every range is consolidated on its own.  An equal pair
    with a cut between its halves comes out as two rows."""
    both = np.concatenate([a, b])
    if len(both) == 0:
        return both
    s = both[np.lexsort((both["v"], both["k"]))]  # stable: a before b
    start = np.ones(len(s), dtype=bool)
    start[1:] = (s["k"][1:] != s["k"][:-1]) | (s["v"][1:] != s["v"][:-1])
    start[[c for c in cuts if 0 < c < len(s)]] = True
    at = np.flatnonzero(start)
    w = np.add.reduceat(s["w"], at)
    keep = w != 0
    return _rows(s["k"][at][keep], s["v"][at][keep], w[keep])


def dense_route(rows):
    """The dense-range probe of sort_consolidate_batch (engine.cpp): above
    8192 rows, a key box of at most cap = min(2^22, 8n) cells goes to the
    weight histogram (sort_cons_dense) instead of a sort."""
    n = len(rows)
    if n <= 8192:
        return False
    kr = int(rows["k"].max()) - int(rows["k"].min())
    vr = int(rows["v"].max()) - int(rows["v"].min())
    cap = min(1 << 22, 8 * n)
    return kr < cap and vr < cap and (kr + 1) * (vr + 1) <= cap
