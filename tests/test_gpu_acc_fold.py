"""The accumulator fold (`Ctx.acc_fold`, the kernel behind the q3 train's
in-train accumulator merge) against the CPU oracle's merge of the same rows.

A is the accumulator, B the small delta (at most 8192 rows); both are
consolidated.  Every pattern below is run over the full size grid where it
can be formed, and the result must equal the oracle's merge row for row
(int64 weights, sorted output: exact equality, no tolerance)."""
import numpy as np
import pytest

from dbsp_amd import oracle
from merge_patterns import (ABOVE, _acc, _rows, _sorted_distinct,
                            pat_above, pat_all_cancel, pat_all_match,
                            pat_below, pat_extremes, pat_interleaved,
                            pat_runs_final_equal, pat_runs_open, pat_same_key)

pytestmark = pytest.mark.gpu

NA = [0, 1, 1023, 1024, 1025, 40000]
NB = [0, 1, 63, 64, 65, 1024, 1025, 8192]
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
