"""The join kernels against whole spines at their run and size edges.

`Ctx.join_spine` route 1 (k_join_count_multi, scan_exclusive,
k_join_emit_multi), route 2 (k_join_probe_multi, k_join_scan_small, the emit
over prepared counts), the single-batch `Ctx.join` (k_join_count,
k_join_emit) and `Ctx.join_tail` (the probe that keeps the run starts, then
k_join_tail_small) run every pattern of tests/join_patterns.py and must give
the numpy reference's rows as an exact sequence: the order (delta row, then
batch, then trace position) is the kernels' contract, and the sequence pins
the length, weight-0 slots of invalid q4 / q6 pairs included."""
import functools

import numpy as np
import pytest

from join_patterns import (FUSE_MAX, batch_cases, hot_cases, merged_trace,
                           pat_tail_cross, pat_tail_total, proj_cases,
                           ref_join, ref_tail, run_cases, size_cases,
                           tail_cases, TAIL_CAP)

pytestmark = pytest.mark.gpu

FAMILIES = {"runs": run_cases, "batches": batch_cases, "hot": hot_cases,
            "sizes": size_cases}


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _family(name):
    return FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def _proj_cases():
    return proj_cases()


@functools.lru_cache(maxsize=None)
def _tail_cases():
    return {name: (plans, cap) for name, plans, cap, _ in tail_cases()}


def _same(got, exp, what):
    assert len(got) == len(exp), f"{what}: {len(got)} vs {len(exp)} rows"
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0])
        raise AssertionError(f"{what}: row {at} is {got[at]}, not {exp[at]}")


def _routes(ctx, name, delta, batches, proj, param):
    exp = ref_join(delta, batches, proj, param)
    for path in (1, 2):
        if path == 2 and len(delta) > FUSE_MAX:
            continue
        got = ctx.join_spine(delta, batches, proj, param, path=path)
        _same(got, exp, f"{name} proj={proj} route {path}")
    return exp


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_spine_routes_give_the_reference_sequence(ctx, family):
    """Routes 1 and 2 on every pattern, under (v2, v1) and (k, v2): the two
    together name the delta row, the key, the batch and the trace place of
    every output row."""
    for name, delta, batches, _ in _family(family):
        for proj in (0, 8):
            _routes(ctx, name, delta, batches, proj, 0)


def test_spine_routes_all_projections(ctx):
    for name, delta, batches, m in _proj_cases():
        _routes(ctx, name, delta, batches, m["proj"], m["param"])


def test_route_2_refuses_a_delta_above_its_bound(ctx):
    name, delta, batches, _ = next(c for c in _family("sizes")
                                   if len(c[1]) == FUSE_MAX + 1)
    with pytest.raises(RuntimeError, match="status -3"):
        ctx.join_spine(delta, batches, 0, path=2)


def test_single_batch_join(ctx):
    """`Ctx.join` on the one-batch patterns, on the hot-key and size patterns
    with their spine merged into one batch, and likewise on every projection
    pattern (8..12 have no other direct test)."""
    ran = 0
    for family in sorted(FAMILIES):
        for name, delta, batches, _ in _family(family):
            if len(batches) != 1 and family == "batches":
                continue
            ran += len(batches) == 1
            one = merged_trace(batches)
            for proj in (0, 8):
                _same(ctx.join(delta, one, proj),
                      ref_join(delta, [one], proj), f"{name} proj={proj}")
    assert ran >= 97  # every run pattern and the nb = 1 spine
    for name, delta, batches, m in _proj_cases():
        one = merged_trace(batches)
        _same(ctx.join(delta, one, m["proj"], m["param"]),
              ref_join(delta, [one], m["proj"], m["param"]), name)


def _check_tail(got, exp, what):
    for f in ("totals", "d_total", "d_flag", "d_final"):
        assert got[f] == exp[f], f"{what}: {f} is {got[f]}, not {exp[f]}"
    for p, (g, e) in enumerate(zip(got["offsets"], exp["offsets"])):
        assert (g is None) == (e is None), f"{what}: plan {p} offsets"
        if e is not None:
            assert np.array_equal(g, e), f"{what}: plan {p} offsets"
    for f in ("store", "capbuf"):
        assert (got[f] is None) == (exp[f] is None), f"{what}: {f}"
        if exp[f] is not None:
            _same(got[f], exp[f], f"{what} {f}")


@pytest.mark.parametrize("name", [c[0] for c in tail_cases()])
def test_tail_gives_the_reference(ctx, name):
    """Verdicts, plan-local offsets and rows of the chained join tail: the
    capacity buffer as the plan-major raw sequence, the output store as the
    consolidated batch."""
    plans, cap = _tail_cases()[name]
    _check_tail(ctx.join_tail(plans, cap), ref_tail(plans, cap), name)


def test_tails_back_to_back(ctx):
    """A large tail, then a tiny one with other shapes, on one context:
    offset cells, counts and buffers of the first do not leak into the
    second.  Twice: a total at the capacity, and three full-length plans."""
    tiny = pat_tail_total(1)
    for big in (pat_tail_total(TAIL_CAP), pat_tail_cross(5)):
        for name, plans, cap, _ in (big, tiny, big, tiny):
            _check_tail(ctx.join_tail(plans, cap), ref_tail(plans, cap),
                        f"{name} (back to back)")
