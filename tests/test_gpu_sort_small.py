"""The fused sort's small-batch path (integer weights, n <= 1024: one row per
thread, sorted and consolidated on chip) against the CPU oracle, at every row
count where the path or its bitonic network changes shape, and the first
counts past it that stay on the LDS bitonic.  Exact equality throughout.

The f64 instantiation shares the body but not the path; its output at
n = 512 and n = 1024 is pinned to the bytes recorded before the path existed
(tests/golden/sort_small_f64.json; provenance in sort_small_f64.README.md
beside it)."""
import numpy as np
import pytest

from dbsp_amd import ROW_DT
from dbsp_amd import oracle
from helpers import load_golden

pytestmark = pytest.mark.gpu

NS = [0, 1, 2, 3,            # trivial
      63, 64, 65,            # wave edges
      127, 128, 129,
      255, 256, 257,
      511, 512, 513,
      1023, 1024,            # last counts on the path
      1025, 1026]            # first on the LDS bitonic

U64_MAX = np.uint64(2**64 - 1)


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


def _rows(k, v, w):
    out = np.empty(len(k), dtype=ROW_DT)
    out["k"], out["v"], out["w"] = k, v, w
    return out


def _random(rng, n, key_range, val_range, w_range=3):
    return _rows(rng.integers(0, key_range, n, dtype=np.uint64),
                 rng.integers(0, val_range, n, dtype=np.uint64),
                 rng.integers(-w_range, w_range + 1, n))


def _zero_sum(n):
    """n weights of magnitude >= 1 where possible, summing to zero."""
    w = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int64)
    if n:
        w[-1] -= w.sum()
    return w


def _patterns(rng, n):
    full = _rows(rng.integers(0, 2**64, n, dtype=np.uint64),
                 rng.integers(0, 2**64, n, dtype=np.uint64),
                 rng.integers(-3, 4, n))
    yield "random full width", full
    yield "duplicate heavy", _random(rng, n, 40, 3)
    one = _rows(np.full(n, 12345, dtype=np.uint64),
                np.full(n, 678, dtype=np.uint64), np.ones(n, dtype=np.int64))
    yield "one segment, nonzero", one
    zero = one.copy()
    zero["w"] = _zero_sum(n)
    yield "one segment, zero sum", zero
    # every pair cancelled except one survivor
    m = max(n - 1, 0) // 2
    pk = rng.permutation(np.arange(1, 2 * n + 1, dtype=np.uint64))[:m]
    pw = rng.integers(1, 4, m)
    rest = n - 2 * m  # 1 or 2 copies of the survivor (0 rows at n = 0)
    surv = _rows(np.full(rest, 2**40 + 9, dtype=np.uint64),
                 np.full(rest, 5, dtype=np.uint64),
                 np.ones(rest, dtype=np.int64))
    canc = np.concatenate([_rows(pk, pk * np.uint64(3), pw),
                           _rows(pk, pk * np.uint64(3), -pw), surv])
    yield "cancelled but one", rng.permutation(canc)
    srt = np.sort(_random(rng, n, 2**20, 4), order=["k", "v"])
    yield "sorted", srt
    yield "reverse sorted", srt[::-1].copy()
    # rows equal to the pad row (maximum k and v) among ordinary ones
    npad = min(n, max(2, n // 3))
    body = _random(rng, n - npad, 2**64, 2**64)
    pad = _rows(np.full(npad, U64_MAX), np.full(npad, U64_MAX),
                np.ones(npad, dtype=np.int64))
    yield "pad-valued rows, nonzero", rng.permutation(
        np.concatenate([body, pad]))
    pad0 = pad.copy()
    pad0["w"] = _zero_sum(npad)
    yield "pad-valued rows, cancelling", rng.permutation(
        np.concatenate([body, pad0]))


@pytest.mark.parametrize("n", NS)
def test_sort_small_matches_oracle(ctx, n):
    rng = np.random.default_rng(1000 + n)
    for name, r in _patterns(rng, n):
        assert len(r) == n, name
        exp = oracle.consolidate(r)
        got = ctx.sort_consolidate(r)
        assert np.array_equal(got, exp), (
            f"n={n} {name}: {len(got)} vs {len(exp)} rows")


def test_sort_small_expected_shapes(ctx):
    """The patterns do what their names say (guards the test's own data)."""
    rng = np.random.default_rng(5)
    got = dict(_patterns(rng, 513))
    assert len(oracle.consolidate(got["one segment, nonzero"])) == 1
    assert len(oracle.consolidate(got["one segment, zero sum"])) == 0
    assert len(oracle.consolidate(got["cancelled but one"])) == 1
    padz = oracle.consolidate(got["pad-valued rows, cancelling"])
    assert not np.any((padz["k"] == U64_MAX) & (padz["v"] == U64_MAX))
    padn = oracle.consolidate(got["pad-valued rows, nonzero"])
    assert padn[-1]["k"] == U64_MAX and padn[-1]["w"] == 513 // 3


@pytest.mark.parametrize("n", [512, 1024])
def test_sort_f64_bytes_unchanged(ctx, n):
    g = load_golden("sort_small_f64.json")[str(n)]
    r = _rows(np.array(g["in_k"], dtype=np.uint64),
              np.array(g["in_v"], dtype=np.uint64),
              np.array(g["in_w_bits"], dtype=np.int64))
    assert len(r) == n
    exp = _rows(np.array(g["out_k"], dtype=np.uint64),
                np.array(g["out_v"], dtype=np.uint64),
                np.array(g["out_w_bits"], dtype=np.int64))
    got = ctx.sort_consolidate_f64(r)
    assert got.tobytes() == exp.tobytes()
