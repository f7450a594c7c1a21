"""The keyed aggregates at their run, key and size edges.

k_agg_count / k_agg_emit in their three modes (`Ctx.agg_linear_upsert`,
`agg_max_upsert`, `agg_last10_upsert`) must give the reference's raw rows as
an exact sequence: per key the new row, then the key's output-trace rows
negated, in trace order.  `Ctx.agg_sum_spine` (unique_keys, k_agg_sum per
batch, k_emit_nonzero) must give the reference's keys in order and its rows
as a sorted set, the ticket order being undefined.  `Ctx.distinct_inc`
(k_distinct_count) must give the reference's rows in delta order."""
import functools

import numpy as np
import pytest

from agg_patterns import (MODES, SIZES, distinct_cases, key_cases,
                          last10_cases, linear_cases, max_cases, ref_distinct,
                          ref_sum_spine, ref_upsert, size_case, sorted_rows,
                          sum_cases)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _small_cases():
    return {c["name"]: c for c in
            last10_cases() + max_cases() + linear_cases() + key_cases()}


def _case(name):
    if name.startswith("size-"):
        return size_case(int(name[5:]))
    return _small_cases()[name]


@functools.lru_cache(maxsize=None)
def _expected(mode, name):
    c = _case(name)
    return ref_upsert(mode, c["keys"], c["in_rows"], c["out_rows"])


def _same(got, exp, what):
    assert len(got) == len(exp), f"{what}: {len(got)} vs {len(exp)} rows"
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0])
        raise AssertionError(f"{what}: row {at} is {got[at]}, not {exp[at]}")


def _upsert(ctx, mode, name):
    fn = {"linear": ctx.agg_linear_upsert, "max": ctx.agg_max_upsert,
          "last10": ctx.agg_last10_upsert}[mode]
    c = _case(name)
    _same(fn(c["keys"], c["in_rows"], c["out_rows"]), _expected(mode, name),
          f"{name} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_upsert_patterns_give_the_reference_sequence(ctx, mode):
    """Every run, price, weight and key pattern under every mode."""
    for name in _small_cases():
        _upsert(ctx, mode, name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nd", SIZES)
def test_upsert_sizes(ctx, nd, mode):
    """Delta lengths around the blocks of the count / emit grid and of the
    scan between them."""
    _upsert(ctx, mode, f"size-{nd}")


@pytest.mark.parametrize("name", [c[0] for c in sum_cases()])
def test_sum_over_a_spine(ctx, name):
    _, delta, batches, _ = next(c for c in sum_cases() if c[0] == name)
    exp_keys, exp_rows = ref_sum_spine(delta, batches)
    keys, rows = ctx.agg_sum_spine(delta, batches)
    assert np.array_equal(keys, exp_keys), f"{name}: unique keys"
    _same(sorted_rows(rows), sorted_rows(exp_rows), name)


@pytest.mark.parametrize("name", [c[0] for c in distinct_cases()])
def test_distinct_over_a_spine(ctx, name):
    _, delta, batches, _ = next(c for c in distinct_cases() if c[0] == name)
    _same(ctx.distinct_inc(delta, batches), ref_distinct(delta, batches),
          name)


def test_aggregates_back_to_back(ctx):
    """The largest delta, then a one-key one, on one context: counts,
    offsets and the accumulator of the first do not leak into the second."""
    sums = {c[0]: c for c in sum_cases()}
    for _ in range(2):
        for mode in MODES:
            _upsert(ctx, mode, f"size-{SIZES[-1]}")
            _upsert(ctx, mode, "keys-same-val")
        for name in ("sum-nb24", "uniq-one-row"):
            _, delta, batches, _ = sums[name]
            exp_keys, exp_rows = ref_sum_spine(delta, batches)
            keys, rows = ctx.agg_sum_spine(delta, batches)
            assert np.array_equal(keys, exp_keys), name
            _same(sorted_rows(rows), sorted_rows(exp_rows), name)
