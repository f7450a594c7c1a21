"""The merge (`Ctx.merge`, `Ctx.merge_f64`: merge_batches in engine.cpp, the
end of every spine insert) against the CPU oracle, over a pattern grid at the
band, slice and tile edges of its three kernels.

Every pattern of tests/merge_patterns.py runs at every size of GRID where it
forms, in both argument orders (ties break a-first and the kernels are not
symmetric), with i64 weights and with the f64 twins w * 0.25 and w * pi.
One IEEE add per output row does not depend on the order, so every result
must equal the oracle's row for row and bit for bit, zero sums dropped."""
import numpy as np
import pytest

from dbsp_amd import oracle
from merge_patterns import (GRID, MERGE_PATTERNS, PI, _sorted_distinct,
                            f64_twin, pat_interleaved)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


@pytest.mark.parametrize("pat", MERGE_PATTERNS, ids=lambda p: p.__name__[4:])
def test_merge_matches_oracle(ctx, pat):
    for band, sizes in GRID.items():
        formed = 0
        for na, nb in sizes:
            ab = pat(na, nb)
            if ab is None:
                continue
            a, b = ab
            assert len(a) == na and len(b) == nb
            assert _sorted_distinct(a) and _sorted_distinct(b), (na, nb)
            formed += 1
            what = f"{pat.__name__} na={na} nb={nb}"
            exp = oracle.merge(a, b)
            for x, y, order in ((a, b, "ab"), (b, a, "ba")):
                got = ctx.merge(x, y)
                assert np.array_equal(got, exp), (
                    f"{what} {order}: {len(got)} vs {len(exp)} rows")
            for scale in (0.25, PI):
                fa, fb = f64_twin(a, scale), f64_twin(b, scale)
                fexp = oracle.merge_f64(fa, fb)
                for x, y, order in ((fa, fb, "ab"), (fb, fa, "ba")):
                    got = ctx.merge_f64(x, y)
                    assert np.array_equal(got, fexp), (
                        f"{what} f64 * {scale} {order}: {len(got)} vs "
                        f"{len(fexp)} rows")
        assert formed >= 4, (band, formed)


def test_mid_merge_back_to_back(ctx):
    """The mid kernel's cross-workgroup barrier keeps its scratch between
    launches and tags it with a generation counter that the i64 and the f64
    instantiation share.  Forty mid-band merges on one context, alternating
    the two, with a small-band and a merge-path merge between them: every
    result equals the first of its kind, which equals the oracle's."""
    a, b = pat_interleaved(8192, 8192)
    fa, fb = f64_twin(a, PI), f64_twin(b, PI)
    sa, sb = pat_interleaved(2048, 2047)
    la, lb = pat_interleaved(16897, 16896)
    first = {False: oracle.merge(a, b), True: oracle.merge_f64(fa, fb)}
    s_exp, l_exp = oracle.merge(sa, sb), oracle.merge(la, lb)
    for n in range(40):
        f64 = n % 2 == 1
        got = ctx.merge_f64(fa, fb) if f64 else ctx.merge(a, b)
        assert np.array_equal(got, first[f64]), f"call {n}"
        assert np.array_equal(ctx.merge(sa, sb), s_exp), f"small after {n}"
        assert np.array_equal(ctx.merge(la, lb), l_exp), f"large after {n}"
