"""The incremental antijoin / semijoin operator (dbsp_antijoin_op) and its
batch primitive (dbsp_antijoin) on the GPU, against the dict model of
tests/antijoin_model.py.

Every stream runs through an antijoin and a semijoin operator: per-tick
outputs equal to the model, every output sorted, distinct and non-zero,
antijoin + semijoin equal to the consolidated dA tick by tick, the
accumulated output equal to dbsp_antijoin over the model's final integrals,
the three counters equal to the model's, and both spines within 24 batches."""
import numpy as np
import pytest

import antijoin_model as am
from dbsp_amd import ROW_DT
from helpers import rows_of

pytestmark = pytest.mark.gpu

ONES = (1 << 64) - 1
MODES = (am.ANTIJOIN, am.SEMIJOIN)


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


def _assert_consolidated(rows):
    if len(rows) == 0:
        return
    assert (rows["w"] != 0).all()
    k, v = rows["k"], rows["v"]
    inc = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1]))
    assert inc.all(), "output not sorted by (k, v) / not distinct"


def _zset(rows):
    """helpers.zset for rows already checked to be distinct and non-zero."""
    return dict(zip(zip(rows["k"].tolist(), rows["v"].tolist()),
                    rows["w"].tolist()))


def _key_rows(pairs):
    return rows_of([(k, 0, w) for k, w in pairs])


def _integral_rows(integral_a):
    return rows_of([(k, v, integral_a[(k, v)]) for k, v in sorted(integral_a)])


def _integral_keys(integral_b):
    return _key_rows([(k, integral_b[k]) for k in sorted(integral_b)])


def run_stream(ctx, ticks, check=None):
    """ticks: [(dA triples, dB (k, w) pairs)].  The contract in the module
    docstring; check(i, stats of both ops) runs after tick i.  Returns
    {mode: (stats, model, per-tick (flips, gathered, filtered))}."""
    from dbsp_amd.engine import AntiJoin
    ops = {m: AntiJoin(ctx, m) for m in MODES}
    models = {m: am.Model(m) for m in MODES}
    counts = {m: [] for m in MODES}
    try:
        for i, (dA, dB) in enumerate(ticks):
            a_rows, b_rows = rows_of(dA), _key_rows(dB)
            got = {}
            for m in MODES:
                out = ops[m].step(a_rows, b_rows)
                _assert_consolidated(out)
                exp, nf, ng, nd = models[m].step(dA, dB)
                assert _zset(out) == exp, f"mode {m} tick {i}"
                counts[m].append((nf, ng, nd))
                got[m] = exp
            assert am.zset_add(got[am.ANTIJOIN], got[am.SEMIJOIN]) == \
                am.consolidate_rows(dA), f"tick {i}"
            if check:
                check(i, {m: ops[m].stats() for m in MODES})
        stats = {m: ops[m].stats() for m in MODES}
    finally:
        for op in ops.values():
            op.close()
    for m in MODES:
        model, st = models[m], stats[m]
        assert model.acc == am.full_output(model.integral_a, model.integral_b,
                                           m)
        recomputed = ctx.antijoin(_integral_rows(model.integral_a),
                                  _integral_keys(model.integral_b), m)
        _assert_consolidated(recomputed)
        assert _zset(recomputed) == model.acc
        assert (st["keys_flipped"], st["rows_gathered"],
                st["rows_filtered"]) == tuple(
                    sum(c[j] for c in counts[m]) for j in range(3))
        assert st["a_batches"] <= 24 and st["b_batches"] <= 24
        assert st["a_rows"] >= len(model.integral_a)
    # the flips and the gathered rows do not depend on the mode
    assert stats[am.ANTIJOIN]["keys_flipped"] == \
        stats[am.SEMIJOIN]["keys_flipped"]
    assert stats[am.ANTIJOIN]["rows_gathered"] == \
        stats[am.SEMIJOIN]["rows_gathered"]
    return {m: (stats[m], models[m], counts[m]) for m in MODES}


# ---- presence edges ----

def test_presence_edges(ctx):
    ticks = [
        ([(1, 10, 1), (1, 11, -2), (2, 20, 1)], []),
        ([], [(1, 1)]),     # 0 -> 1: flip
        ([], [(1, 1)]),     # 1 -> 2
        ([], [(1, -1)]),    # 2 -> 1
        ([], [(1, -1)]),    # 1 -> 0: flip
        ([], [(1, -1)]),    # 0 -> -1: still absent
        ([(1, 12, 1)], []),  # a row under a key at -1: the key is absent
        ([], [(1, 2)]),     # -1 -> +1: flip
    ]
    res = run_stream(ctx, ticks)
    _, model, counts = res[am.ANTIJOIN]
    assert [c[0] for c in counts] == [0, 1, 0, 0, 1, 0, 0, 1]
    # the net-negative row (1, 11, -2) is re-emitted with the flip's sign
    assert [c[1] for c in counts] == [0, 2, 0, 0, 2, 0, 0, 3]
    assert model.acc == {(2, 20): 1}
    assert res[am.SEMIJOIN][1].acc == {(1, 10): 1, (1, 11): -2, (1, 12): 1}


def test_presence_split_over_batches(ctx):
    """The key X sits in three batches of the key spine at +1, -2 and +2:
    its presence is the sum over all of them."""
    X = 5000
    sizes = (1000, 400, 150, 50)
    weights = (1, -2, 2, None)      # X: +1, then -1, then +1 in total
    ticks = [([(X, v, 1) for v in range(3)] + [(7, 0, 1), (10 ** 6, 1, 1)],
              [])]
    base = 0
    for size, wx in zip(sizes, weights):
        keys = [(base + 3 * i, 1) for i in range(size - (wx is not None))]
        if wx is not None:
            keys.append((X, wx))
        ticks.append(([], keys))
        base += 10 ** 5
    ticks += [([], [(X, -1)]), ([], [(X, 1)]), ([(X, 9, 1)], [(X, 3)])]

    def check(i, stats):
        if i == len(sizes):
            for st in stats.values():
                assert st["b_batches"] >= 3
    res = run_stream(ctx, ticks, check)
    counts = res[am.ANTIJOIN][2]
    # X flips in the 1000, 400 and 150 ticks and in the two single-key ticks,
    # each time moving its three rows; the last tick flips nothing
    assert [c[1] for c in counts] == [0, 3, 3, 3, 0, 3, 3, 0]
    assert [c[0] for c in counts] == [0, 1000, 400, 150, 50, 1, 1, 0]


def test_key_and_value_range(ctx):
    ticks = [
        ([(0, 0, 1), (0, ONES, 1), (ONES, 0, 2), (ONES, ONES, -1),
          (1, 5, 1), (ONES - 1, 5, 1)], [(0, 1)]),
        ([], [(ONES, 1)]),
        ([(0, 7, 1), (ONES, 7, 1)], [(0, -1)]),
        ([], [(ONES, -1), (ONES - 1, 1), (1, 1)]),
    ]
    res = run_stream(ctx, ticks)
    assert res[am.ANTIJOIN][1].acc == {
        (0, 0): 1, (0, ONES): 1, (0, 7): 1, (ONES, 0): 2, (ONES, ONES): -1,
        (ONES, 7): 1}


def test_same_tick_a_and_b(ctx):
    ticks = [
        ([(5, 1, 1)], [(5, 1)]),        # row and key together
        ([(5, 1, -1)], [(5, -1)]),      # both retracted together
        ([(6, 1, 1), (6, 2, 1)], []),
        ([(6, 3, 1), (6, 1, -1), (8, 1, 1)], [(6, 1)]),  # flip + rows of it
        ([(6, 4, 2)], [(6, -1), (8, 1)]),
    ]
    res = run_stream(ctx, ticks)
    anti, semi = res[am.ANTIJOIN], res[am.SEMIJOIN]
    assert anti[2][0] == (1, 0, 1) and semi[2][0] == (1, 0, 0)
    assert anti[2][1] == (1, 1, 0)
    assert anti[1].acc == {(6, 2): 1, (6, 3): 1, (6, 4): 2}
    assert semi[1].acc == {(8, 1): 1}


def test_hot_key_over_batches(ctx):
    """3,000 values of one key in three batches of the row spine, flipped on
    and off: the emit is spread over its output rows, across blocks and
    batches."""
    ticks = [
        ([(7, v, 1) for v in range(2000)] + [(6, 0, 1), (8, 0, 1)], []),
        ([(7, v, 1 + v % 2) for v in range(2000, 2900)], []),
        ([(7, v, -1) for v in range(2900, 3000)], []),
        ([], [(7, 1)]),
        ([], [(7, 1), (6, 1)]),
        ([], [(7, -2)]),
    ]

    def check(i, stats):
        if i == 2:
            for st in stats.values():
                assert st["a_batches"] >= 2
    res = run_stream(ctx, ticks, check)
    assert [c[1] for c in res[am.ANTIJOIN][2]] == [0, 0, 0, 3000, 1, 3000]


def test_empty_inputs_and_no_flip(ctx):
    gathered = []

    def check(i, stats):
        gathered.append(stats[am.ANTIJOIN]["rows_gathered"])
    ticks = [
        ([], []),
        ([(1, 1, 1), (2, 1, 1)], []),
        ([], [(1, 1)]),
        ([], []),
        ([], [(3, 1), (3, -1)]),            # consolidates to nothing
        ([(4, 1, 1), (4, 1, -1)], []),      # likewise
        ([], [(1, 1), (2, -1)]),            # non-empty, flips nothing
    ]
    res = run_stream(ctx, ticks, check)
    assert gathered == [0, 0, 1, 1, 1, 1, 1]
    st = res[am.ANTIJOIN][0]
    assert st["keys_flipped"] == 1 and st["b_rows"] == 2


# ---- sizes around block and sort-regime edges ----

def _spread(i):
    """distinct, scattered 40-bit keys"""
    return (i * 0x9E3779B97F4A7C15) >> 24 & ((1 << 40) - 1)


@pytest.mark.parametrize("n", [255, 256, 257, 1024, 1025, 2049, 9000])
def test_da_sizes(ctx, n):
    nkeys = (n + 2) // 3
    rng = np.random.default_rng(n)
    dA = [(_spread(i // 3), i % 3, int(rng.integers(1, 3))) for i in range(n)]
    perm = rng.permutation(n)
    dA = [dA[j] for j in perm]
    ticks = [
        ([], [(_spread(g), 1) for g in range(0, nkeys, 2)]),
        (dA, []),
        ([], [(_spread(g), -1) for g in range(0, nkeys, 4)]),
    ]
    res = run_stream(ctx, ticks)
    c = res[am.ANTIJOIN][2]
    assert c[1][2] > 0 and c[1][2] < n and c[2][1] > 0


@pytest.mark.parametrize("n", [257, 9000])
def test_db_sizes(ctx, n):
    dA = [(_spread(g), v, 1) for g in range(0, n, 5) for v in range(2)]
    keys = [(_spread(g), 1) for g in range(n)]
    ticks = [
        (dA, []),
        ([], keys),
        ([], [(k, w) for k, w in keys[::2]]),        # 1 -> 2: no flip
        ([], [(k, -1) for k, _ in keys[1::2]]),      # every other one off
    ]
    res = run_stream(ctx, ticks)
    c = res[am.ANTIJOIN][2]
    assert c[1][0] == n and c[2] == (0, 0, 0) and c[3][0] == n // 2


def test_random_stream(ctx):
    res = run_stream(ctx, am.random_stream(11))
    st = res[am.ANTIJOIN][0]
    assert st["keys_flipped"] > 0 and st["rows_gathered"] > 0
    assert st["rows_filtered"] > 0


# ---- the batch primitive alone ----

def test_primitive(ctx):
    a = rows_of([(1, 1, 1), (1, 2, -1), (3, 0, 2), (ONES, ONES, 1)])
    empty = np.empty(0, dtype=ROW_DT)
    all_keys = _key_rows([(1, 1), (3, 2), (ONES, 1)])
    other = _key_rows([(0, 1), (2, 5), (3, -1), (ONES - 1, 1)])
    for m in MODES:
        assert len(ctx.antijoin(empty, all_keys, m)) == 0
        assert len(ctx.antijoin(empty, empty, m)) == 0
    assert ctx.antijoin(a, empty, am.ANTIJOIN).tobytes() == a.tobytes()
    assert len(ctx.antijoin(a, empty, am.SEMIJOIN)) == 0
    assert len(ctx.antijoin(a, all_keys, am.ANTIJOIN)) == 0
    assert ctx.antijoin(a, all_keys, am.SEMIJOIN).tobytes() == a.tobytes()
    # no key present: 3 is there at a negative weight
    assert ctx.antijoin(a, other, am.ANTIJOIN).tobytes() == a.tobytes()
    assert len(ctx.antijoin(a, other, am.SEMIJOIN)) == 0
    some = _key_rows([(1, 1)])
    assert ctx.antijoin(a, some, am.ANTIJOIN).tobytes() == a[2:].tobytes()
    assert ctx.antijoin(a, some, am.SEMIJOIN).tobytes() == a[:2].tobytes()


def test_unknown_mode_is_an_error(ctx):
    from dbsp_amd.engine import AntiJoin
    a = rows_of([(1, 1, 1)])
    for mode in (-1, 2):
        with pytest.raises(RuntimeError):
            AntiJoin(ctx, mode)
        with pytest.raises(RuntimeError):
            ctx.antijoin(a, _key_rows([(1, 1)]), mode)
