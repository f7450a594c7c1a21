"""The merge pattern grid of tests/merge_patterns.py, checked without a GPU:
the builders give what they promise at every size of the three bands, the
C++ oracle agrees with an independent numpy model on every case (i64 and f64
weights), and the straddle pattern hits the cut and not its neighbour."""
import numpy as np
import pytest

from dbsp_amd import ROW_DT, oracle
from merge_patterns import (GRID, MERGE_PATTERNS, PI, _rows, _sorted_distinct,
                            band_of, boundaries, dense_route, f64_twin,
                            kv_scale, numpy_merge, pat_straddle,
                            sliced_merge_no_adjust, straddle_cuts)


def test_grid_sits_in_its_bands():
    for band, sizes in GRID.items():
        for na, nb in sizes:
            assert band_of(na + nb) == band, (na, nb)
    assert band_of(4096) == "small" and band_of(4097) == "mid"
    assert band_of(32768) == "mid" and band_of(32769) == "merge_path"


def test_boundaries():
    assert boundaries(0) == [] and boundaries(1) == []
    assert boundaries(2) == [1]
    assert boundaries(1024) == (list(range(1, 33)) + [512]
                                + list(range(993, 1024)))
    b = boundaries(4096)  # 1023 diagonals of 4 rows, thinned to 64
    assert len(b) == 64 and b[0] == 4 and b[31] == 128 and b[-1] == 4092
    assert boundaries(4097) == [129 * w for w in range(1, 32)]
    assert boundaries(32768) == [1024 * w for w in range(1, 32)]
    assert boundaries(32769) == [1024 * t for t in range(1, 33)]
    assert boundaries(33792) == [1024 * t for t in range(1, 33)]  # 33 tiles
    assert boundaries(33793) == [1024 * t for t in range(1, 34)]
    assert len(boundaries(65539)) == 64


@pytest.mark.parametrize("pat", MERGE_PATTERNS, ids=lambda p: p.__name__[4:])
def test_pattern_forms_and_oracle_matches_numpy(pat):
    for band, sizes in GRID.items():
        formed = 0
        for na, nb in sizes:
            ab = pat(na, nb)
            if ab is None:
                continue
            formed += 1
            a, b = ab
            assert a.dtype == ROW_DT and b.dtype == ROW_DT
            assert len(a) == na and len(b) == nb, (na, nb)
            assert _sorted_distinct(a) and _sorted_distinct(b), (na, nb)
            assert np.all(a["w"] != 0) and np.all(b["w"] != 0)
            exp = oracle.merge(a, b)
            assert np.array_equal(exp, numpy_merge(a, b)), (na, nb)
            assert np.array_equal(exp, oracle.merge(b, a)), (na, nb)
            for scale in (0.25, PI, None):
                fa = f64_twin(a, kv_scale(a) if scale is None else scale)
                fb = f64_twin(b, kv_scale(b) if scale is None else scale)
                fexp = oracle.merge_f64(fa, fb)
                assert np.array_equal(fexp, numpy_merge(fa, fb, f64=True)), (
                    na, nb, scale)
                # the pairs that cancel as integers cancel here, no others
                assert np.array_equal(fexp[["k", "v"]], exp[["k", "v"]])
        assert formed >= 4, (pat.__name__, band, formed)


def test_oracle_merge_f64_random_finite_weights():
    """Random finite f64 weights on the interleaved-with-matches shape: one
    IEEE add per output row, so the oracle equals the numpy model bit for
    bit; a pair whose sum is +0.0 is dropped."""
    rng = np.random.default_rng(5)
    for na, nb in [(1, 1), (2048, 2047), (8192, 8192), (16897, 16896)]:
        k = np.sort(rng.choice(4 * (na + nb), na + nb, replace=False))
        pick = rng.permutation(na + nb)
        ia, ib = np.sort(pick[:na]), np.sort(pick[na:])
        a = _rows(k[ia], ia % 3, np.zeros(na))
        b = _rows(k[ib], ib % 3, np.zeros(nb))
        share = min(na, nb) // 2  # matches: b repeats a's (k, v)
        b[:share] = a[:share]
        b = b[np.lexsort((b["v"], b["k"]))]
        assert _sorted_distinct(a) and _sorted_distinct(b)
        wa = rng.standard_normal(na) * 10.0 ** rng.integers(-30, 30, na)
        wb = rng.standard_normal(nb) * 10.0 ** rng.integers(-30, 30, nb)
        a["w"], b["w"] = wa.view(np.int64), wb.view(np.int64)
        # every other match cancels exactly
        pos = {(int(r["k"]), int(r["v"])): n for n, r in enumerate(a[:share])}
        for n, r in enumerate(b):
            m = pos.get((int(r["k"]), int(r["v"])))
            if m is not None and m % 2 == 0:
                b["w"][n] = (-wa[m]).view(np.int64)
        exp = oracle.merge_f64(a, b)
        assert np.array_equal(exp, numpy_merge(a, b, f64=True)), (na, nb)
        assert len(exp) == na + nb - share - (share + 1) // 2


def test_straddle_hits_the_cut_and_not_its_neighbour():
    """Off 0: merging every range between the plain merge-path cuts on its
    own differs from the oracle at every size where the pattern forms.  Off
    -1 and +1: the same model equals the oracle."""
    formed = {(off, below): 0 for off in (-1, 0, 1) for below in (0, 1)}
    for sizes in GRID.values():
        for na, nb in sizes:
            cuts = boundaries(na + nb)
            for off, below in formed:
                ds = straddle_cuts(na, nb, off, below)
                if ds is None:
                    continue
                assert set(ds) <= set(cuts)
                a, b = pat_straddle(na, nb, ds, off, below)
                formed[off, below] += 1
                exp = oracle.merge(a, b)
                for x, y in ((a, b), (b, a)):
                    got = sliced_merge_no_adjust(x, y, cuts)
                    if off == 0:
                        # both halves of every cut pair come out
                        assert len(got) > len(exp), (na, nb, below)
                        assert not np.array_equal(got, exp), (na, nb, below)
                    else:
                        assert np.array_equal(got, exp), (na, nb, off, below)
                # with no cut at all the model is the merge
                assert np.array_equal(sliced_merge_no_adjust(a, b, []), exp)
    assert min(formed.values()) >= 12, formed


def test_straddle_late_reaches_the_last_cuts():
    """Balanced sizes: the plain form reaches the first half of the cuts,
    the late form the second half, the last one included."""
    for na, nb in [(2048, 2048), (16384, 16384), (16896, 16896)]:
        cuts = boundaries(na + nb)
        early = straddle_cuts(na, nb, 0)
        late = straddle_cuts(na, nb, 0, below=True)
        assert early[0] == cuts[0] and late[-1] == cuts[-1]
        assert len(set(early) | set(late)) >= len(cuts) - 1


def test_straddle_positions():
    """The b-half of pair j sits at merged position d_j + off."""
    na, nb = 3072, 1024
    for ds, below in (([4, 8, 100, 2000, 3000], False),
                      ([1024, 1030, 2000, 4000, 4092], True)):
        for off in (-1, 0, 1):
            a, b = pat_straddle(na, nb, ds, off, below)
            assert len(b) == nb and _sorted_distinct(b)
            both = np.concatenate([a, b])
            order = np.lexsort((both["v"], both["k"]))  # stable: a first
            where = np.empty(len(both), dtype=np.int64)
            where[order] = np.arange(len(both))
            at = where[na + nb - len(ds):] if below else where[na:na + len(ds)]
            assert [int(x) for x in at] == [d + off for d in ds]
    assert pat_straddle(4, 1, [2, 4], 0) is None       # nb < len(diagonals)
    assert pat_straddle(4, 4, [1], -1) is None         # index -1
    assert pat_straddle(4, 4, [5], 0) is None          # index 4
    a, b = pat_straddle(8, 3, [2, 3, 4], 0)            # 3 is within 2 of 2
    assert np.array_equal(b[["k", "v"]][:2], a[["k", "v"]][[1, 2]])


def test_dense_route_predicate():
    def box(n, kr, vr):
        r = np.zeros(n, dtype=ROW_DT)
        r["k"][0], r["v"][0] = 5 + kr, 9 + vr
        r["k"][1:], r["v"][1:] = 5, 9
        return r
    assert not dense_route(box(8192, 0, 0))            # at most one chunk
    assert dense_route(box(8193, 0, 0))
    n = 10_000                                         # cap = 80000
    assert dense_route(box(n, 79_999, 0)) and dense_route(box(n, 0, 79_999))
    assert not dense_route(box(n, 80_000, 0))
    assert dense_route(box(n, 399, 199))               # 400 * 200 cells
    assert not dense_route(box(n, 400, 199))
    n = 1 << 20                                        # cap = 2^22, not 8n
    assert dense_route(box(n, (1 << 22) - 1, 0))
    assert not dense_route(box(n, 1 << 22, 0))
    assert not dense_route(box(n, 1 << 40, 1 << 30))   # no overflow games
