"""The window stage against whole spines at its bound and run edges.

`Ctx.window_spine` route 1 (k_window_ranges_multi with host bounds, then
k_window_emit_multi) and route 2 (k_wm_update, then the ranges reading the
device bounds and a device batch length, then the emit) run every pattern of
tests/window_patterns.py and must give the reference's region table, total
and rows as an exact sequence: the order (batch, then retract / shrink /
insert, the tick batch last) is the kernels' contract.  `Ctx.wm_update` runs
the watermark sequences through its three sources and must give the
reference's state and bounds words."""
import functools

import numpy as np
import pytest

from window_patterns import (M64, chain_cases, chain_for, emit_cases,
                             grid_case, ref_chain, ref_window_spine, ref_wm,
                             run_cases, shape_cases, spine_cases, table_diff,
                             wm_sequences)

pytestmark = pytest.mark.gpu

FAMILIES = {"runs": run_cases, "shapes": shape_cases, "spines": spine_cases,
            "emit": emit_cases}
SOURCES = ("host_n", "dev_n", "gmax")


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _expected(family, i):
    c = _cases(family)[i]
    s0, e0, s1, e1, hp = c["bounds"]
    return ref_window_spine(c["batches"], c["tick"], hp, s0, e0, s1, e1)


@functools.lru_cache(maxsize=None)
def _cases(family):
    return [grid_case()] if family == "grid" else FAMILIES[family]()


def _same(got, exp, what):
    assert len(got) == len(exp), f"{what}: {len(got)} vs {len(exp)} rows"
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0])
        raise AssertionError(f"{what}: row {at} is {got[at]}, not {exp[at]}")


def _check(got, total, table, rows, what):
    assert got["total"] == total, f"{what}: total {got['total']}, not {total}"
    if total < 0:
        assert got["table"] is None and len(got["rows"]) == 0, what
        return
    diff = table_diff(got["table"], table)
    assert diff is None, f"{what}: {diff}"
    _same(got["rows"], rows, what)


def _both_routes(ctx, family, i):
    c = _cases(family)[i]
    table, rows = _expected(family, i)
    got = ctx.window_spine(c["batches"], c["tick"], bounds=c["bounds"])
    _check(got, len(rows), table, rows, f"{c['name']} route 1")
    got = ctx.window_spine(c["batches"], c["tick"], chain=chain_for(c))
    assert tuple(got["bounds"]) == c["bounds"] + (0,), f"{c['name']} bounds"
    _check(got, len(rows), table, rows, f"{c['name']} route 2")


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_both_routes_give_the_reference_sequence(ctx, family):
    for i in range(len(_cases(family))):
        _both_routes(ctx, family, i)


def test_emit_grid_stride(ctx):
    """A total of 16384 * 256 + 257: the capped grid takes a second turn."""
    _both_routes(ctx, "grid", 0)


@pytest.mark.parametrize("name", [c["name"] for c in chain_cases()])
def test_chained_route_edges(ctx, name):
    """Device lengths equal to, shorter than and zero against the uploaded
    batch, the -1 verdicts of a negative length and of an err watermark, and
    q5's and q8's own parameters moving the watermark."""
    c = next(c for c in chain_cases() if c["name"] == name)
    exp = ref_chain(c["batches"], c["tick"], c["chain"])
    got = ctx.window_spine(c["batches"], c["tick"], chain=c["chain"])
    assert got["bounds"] == exp["bounds"], name
    assert got["state"] == exp["state"], name
    _check(got, exp["total"], exp["table"], exp["rows"], name)


def _keys_for(g):
    if g is None:
        return []
    return [g] if g < 2 else [g // 2, g]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("seq", [s[0] for s in wm_sequences()])
def test_watermark_sequences(ctx, seq, source):
    """State and bounds words tick by tick.  The reduced-maximum source is
    handed a non-empty key column it must ignore: 0 means no maximum."""
    _, (width, tumble, lag), ticks = next(s for s in wm_sequences()
                                          if s[0] == seq)
    state = [0, 0, 0, 0]
    for t, g in enumerate(ticks):
        exp_state, exp_bounds = ref_wm(state, g, width, tumble, lag)
        if source == "gmax":
            got = ctx.wm_update(state, source, keys=[7, M64 - 5], gmax=g or 0,
                                width=width, tumble=tumble, lag=lag)
        else:
            got = ctx.wm_update(state, source, keys=_keys_for(g), width=width,
                                tumble=tumble, lag=lag)
        assert got[0] == list(exp_state), f"{seq} tick {t} ({g}): state"
        assert got[1] == exp_bounds, f"{seq} tick {t} ({g}): bounds"
        state = got[0]


@pytest.mark.parametrize("source", ["host_n", "dev_n"])
def test_watermark_err_leaves_everything_but_the_err_word(ctx, source):
    width, tumble, lag = 10000, 2000, 4000
    state = [123457, 112000, 122000, 1]
    seeded = [0xA1, 0xB2, 0xC3, 0xD4, 0xE5, 0]
    keys = [200000, 300000]
    got_state, got_bounds = ctx.wm_update(state, source, keys=keys, n=-1,
                                          width=width, tumble=tumble, lag=lag,
                                          bounds=seeded)
    assert got_state == state
    assert got_bounds == seeded[:5] + [1]
    # the next good update is what it would have been without the err tick,
    # and clears the err word
    exp = ref_wm(state, keys[-1], width, tumble, lag)
    got = ctx.wm_update(got_state, source, keys=keys, width=width,
                        tumble=tumble, lag=lag, bounds=got_bounds)
    assert got[0] == list(exp[0]) and got[1] == exp[1]
    # a shorter length sees an earlier maximum
    exp = ref_wm(state, keys[0], width, tumble, lag)
    got = ctx.wm_update(state, source, keys=keys, n=1, width=width,
                        tumble=tumble, lag=lag)
    assert got[0] == list(exp[0]) and got[1] == exp[1]


def test_windows_back_to_back(ctx):
    """A 24-batch spine, then a one-row total, on one context and both
    routes: the region table and lengths of the first do not leak into the
    second."""
    big = next(i for i, c in enumerate(_cases("spines"))
               if c["name"] == "spine-nb24")
    tiny = next(i for i, c in enumerate(_cases("emit"))
                if c["name"] == "emit-total-1")
    for _ in range(2):
        _both_routes(ctx, "spines", big)
        _both_routes(ctx, "emit", tiny)
    err = next(c for c in chain_cases() if c["name"] == "chain-err-watermark")
    got = ctx.window_spine(err["batches"], err["tick"], chain=err["chain"])
    assert got["total"] == -1
    _both_routes(ctx, "emit", tiny)
