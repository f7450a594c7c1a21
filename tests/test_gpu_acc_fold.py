"""The accumulator fold (`Ctx.acc_fold`, the kernel behind the q3 train's
in-train accumulator merge) against the CPU oracle's merge of the same rows.

A is the accumulator, B the small delta (at most 8192 rows); both are
consolidated.  Every pattern below is run over the full size grid where it
can be formed, and the result must equal the oracle's merge row for row
(int64 weights, sorted output: exact equality, no tolerance)."""
import numpy as np
import pytest

from dbsp_amd import ROW_DT, oracle

pytestmark = pytest.mark.gpu

NA = [0, 1, 1023, 1024, 1025, 40000]
NB = [0, 1, 63, 64, 65, 1024, 1025, 8192]
M64 = (1 << 64) - 1
BASE = 1 << 20     # A's keys are BASE + 10 * i: room below, between and above
ABOVE = 1 << 40
ERR_INTERNAL = -5  # DBSP_ERR_INTERNAL


def fold_slices(na):
    """The launcher's slicing rule (acc_fold_wgs in kernels_iface.hpp):
    ceil(na / 1024) workgroups, at least 1 and at most 64, each taking
    ceil(na / workgroups) consecutive A rows.  Returns the A indices at
    which a new slice starts."""
    wgs = min(64, max(1, -(-na // 1024)))
    per = -(-na // wgs) if na else 0
    return [w * per for w in range(1, wgs) if w * per < na]


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


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


def pat_slice_boundaries(na, nb):
    """A match and an insertion at the A indices one below, at and one above
    every slice boundary; what is left of nb goes past the end of A."""
    starts = fold_slices(na)
    if not starts or nb == 0:
        return None
    a = _acc(na)
    k, v, w = [], [], []
    for s in starts:
        for idx in (s - 1, s, s + 1):
            if not 0 <= idx < na or len(k) + 2 > nb:
                continue
            r = a[idx]
            k += [int(r["k"]) - 1, int(r["k"])]
            v += [7, int(r["v"])]
            w += [1, -int(r["w"]) if idx % 2 else 6]
    rest = nb - len(k)
    k += [ABOVE + x for x in range(rest)]
    v += [0] * rest
    w += [1] * rest
    return a, _rows(k, v, w)


PATTERNS = [pat_interleaved, pat_below, pat_above, pat_all_match,
            pat_all_cancel, pat_runs_open, pat_runs_final_equal,
            pat_same_key, pat_extremes, pat_slice_boundaries]


@pytest.mark.parametrize("pat", PATTERNS, ids=lambda p: p.__name__[4:])
def test_acc_fold_matches_oracle_merge(ctx, pat):
    formed = 0
    for na in NA:
        for nb in NB:
            ab = pat(na, nb)
            if ab is None:
                continue
            a, b = ab
            assert len(a) == na and len(b) == nb
            assert _sorted_distinct(a) and _sorted_distinct(b), (na, nb)
            formed += 1
            exp = oracle.merge(a, b)
            got = ctx.acc_fold(a, b)
            assert np.array_equal(got, exp), (
                f"{pat.__name__} na={na} nb={nb}: {len(got)} vs {len(exp)} "
                f"rows")
    assert formed >= 6


def test_acc_fold_cancel_to_empty(ctx):
    """na == nb with every row cancelled: the result is empty."""
    for n in (1, 1024, 1025):
        a, b = pat_all_cancel(n, n)
        assert len(ctx.acc_fold(a, b)) == 0


def test_acc_fold_poisoned_delta_length(ctx):
    """A delta length of -1 (the train's failed-speculation poison) reaches
    the kernel verbatim: internal error, no output, and the context goes on
    working."""
    a, b = pat_interleaved(1025, 65)
    with pytest.raises(RuntimeError, match=f"status {ERR_INTERNAL}$"):
        ctx.acc_fold(a, b, b_len=-1)
    assert np.array_equal(ctx.acc_fold(a, b), oracle.merge(a, b))
