"""The incremental arg-max per group operator with ties (dbsp_argmax_op) and
its batch primitive (dbsp_argmax) on the GPU, against the dict model of
tests/argmax_model.py.

Every operator test runs its stream through a default operator and a
refill_all one: per-tick outputs byte-equal between the two and equal to the
model, every output sorted, distinct and non-zero, the accumulated output
equal to dbsp_argmax over the model's final integral, groups_refilled equal
to the model's count of the refill rule, groups_seen equal across the two
routes, and at most 24 batches per spine."""
import numpy as np
import pytest

import argmax_model as am
from dbsp_amd import ROW_DT
from helpers import rows_of, zset

pytestmark = pytest.mark.gpu

ONES = (1 << 64) - 1


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


def _rows(delta):
    """[(k, v, w)] or a ready ROW_DT array -> ROW_DT array."""
    if isinstance(delta, np.ndarray):
        return delta
    return rows_of(delta)


def _triples(delta):
    if isinstance(delta, np.ndarray):
        return list(zip(delta["k"].tolist(), delta["v"].tolist(),
                        delta["w"].tolist()))
    return delta


def _integral_rows(integral):
    keys = sorted(integral)
    out = np.empty(len(keys), dtype=ROW_DT)
    out["k"] = np.array([k for k, _ in keys], dtype=np.uint64)
    out["v"] = np.array([v for _, v in keys], dtype=np.uint64)
    out["w"] = np.array([integral[key] for key in keys], dtype=np.int64)
    return out


def _zset(rows):
    """helpers.zset for rows already checked to be distinct and non-zero."""
    return dict(zip(zip(rows["k"].tolist(), rows["v"].tolist()),
                    rows["w"].tolist()))


def run_stream(ctx, ticks, gs, rs):
    """The contract in the module docstring; returns (default stats,
    refill_all stats, model, per-tick model refill counts, per-tick model
    outputs)."""
    from dbsp_amd.engine import ArgMax
    op_d = ArgMax(ctx, gs, rs)
    op_r = ArgMax(ctx, gs, rs, refill_all=True)
    model = am.Model(gs, rs)
    acc, refills, outs, touched = {}, [], [], 0
    try:
        for i, delta in enumerate(ticks):
            rows = _rows(delta)
            got_d, got_r = op_d.step(rows), op_r.step(rows)
            assert got_d.tobytes() == got_r.tobytes(), f"tick {i}"
            _assert_consolidated(got_d)
            exp, n_refill, n_groups = model.step(_triples(delta))
            assert _zset(got_d) == exp, f"tick {i}"
            acc = am.zset_add(acc, exp)
            refills.append(n_refill)
            outs.append(exp)
            touched += n_groups
        st_d, st_r = op_d.stats(), op_r.stats()
    finally:
        op_d.close()
        op_r.close()
    assert acc == model.acc
    recomputed = ctx.argmax(_integral_rows(model.integral), gs, rs)
    _assert_consolidated(recomputed)
    assert _zset(recomputed) == acc
    assert st_d["groups_refilled"] == sum(refills)
    assert st_d["groups_seen"] == touched == st_r["groups_seen"]
    assert st_r["groups_refilled"] == touched
    assert st_d["in_rows"] == st_r["in_rows"]
    assert st_d["out_rows"] == st_r["out_rows"]
    for st in (st_d, st_r):
        assert st["in_batches"] <= 24 and st["out_batches"] <= 24
    if sum(refills) == 0:
        assert st_d["rows_gathered"] == 0
    return st_d, st_r, model, refills, outs


# ---- ties ----

@pytest.mark.parametrize("ties", [1, 2, 600])
def test_tie_sets(ctx, ties):
    """600 ties straddle 256-thread blocks in the select stage."""
    gs, rs = 20, 10
    top = (5 << gs) | (77 << rs)
    ticks = [[((5 << gs) | (3 << rs) | i, i, 1) for i in range(700)] +
             [(top | i, 9, 1) for i in range(ties)] +
             [((6 << gs) | 1, 0, 1)],
             # one row below the maximum more: nothing
             [((5 << gs) | (4 << rs), 0, 1)],
             # one tie more
             [(top | 1023, 9, 1)]]
    _, _, model, refills, outs = run_stream(ctx, ticks, gs, rs)
    assert refills == [0, 0, 0]
    assert len(outs[0]) == ties + 1 and outs[1] == {}
    assert outs[2] == {(top | 1023, 9): 1}
    assert len(model.acc) == ties + 2


def test_weights_pass_through(ctx):
    gs, rs = 8, 4
    ticks = [[(0x120, 0, 1), (0x121, 1, 3), (0x100, 0, 5)],
             [(0x120, 0, 1)],                # 1 -> 2: +1 for that row only
             [(0x121, 1, -5)],               # 3 -> -2: present, -5
             [(0x100, 0, 1)]]                # below the maximum: nothing
    _, _, _, refills, outs = run_stream(ctx, ticks, gs, rs)
    assert outs == [{(0x120, 0): 1, (0x121, 1): 3}, {(0x120, 0): 1},
                    {(0x121, 1): -5}, {}]
    assert refills == [0, 0, 0, 0]


def test_divergence_mixed_sign_ties(ctx):
    """Rows of weight +1 and -1 at the top rank are both present and stay the
    tie set (the reference's Min would skip that price)."""
    _, _, _, _, outs = run_stream(
        ctx, [[(0x100, 0, 1), (0x120, 0, 1), (0x121, 0, -1)]], 8, 4)
    assert outs == [{(0x120, 0): 1, (0x121, 0): -1}]


# ---- the verdicts ----

def test_verdict_cases(ctx):
    gs, rs = 8, 4
    fill = [[(0x100, 0, 1), (0x110, 0, 1), (0x120, 0, 1), (0x121, 5, 1),
             (0x200, 0, 1)]]
    # the maximum rises: no refill
    st, _, _, r, o = run_stream(ctx, fill + [[(0x130, 0, 1)]], gs, rs)
    assert r == [0, 0] and st["rows_gathered"] == 0
    assert o[1] == {(0x130, 0): 1, (0x120, 0): -1, (0x121, 5): -1}
    # a tie vanishes while another stays: no refill
    st, _, _, r, o = run_stream(ctx, fill + [[(0x120, 0, -1)]], gs, rs)
    assert r == [0, 0] and st["rows_gathered"] == 0
    assert o[1] == {(0x120, 0): -1}
    # all ties vanish: refill, the next rank surfaces
    st, _, _, r, o = run_stream(
        ctx, fill + [[(0x120, 0, -1), (0x121, 5, -1)]], gs, rs)
    # the group's run: 2 rows consolidated, 6 while its batches are apart
    assert r == [0, 1] and 2 <= st["rows_gathered"] <= 6
    assert o[1] == {(0x120, 0): -1, (0x121, 5): -1, (0x110, 0): 1}
    # the group empties: refill, the output is -Oc
    st, _, _, r, o = run_stream(ctx, fill + [[(0x200, 0, -1)]], gs, rs)
    assert r == [0, 1] and st["rows_gathered"] <= 2
    assert o[1] == {(0x200, 0): -1}
    # a higher row appears in the tick in which all ties vanish: no refill
    st, _, _, r, o = run_stream(
        ctx, fill + [[(0x120, 0, -1), (0x121, 5, -1), (0x1F0, 0, 2)]], gs, rs)
    assert r == [0, 0] and st["rows_gathered"] == 0
    assert o[1] == {(0x120, 0): -1, (0x121, 5): -1, (0x1F0, 0): 2}
    # ... and so does a new row at the old rank; a lower one does not help
    _, _, _, r, _ = run_stream(
        ctx, fill + [[(0x120, 0, -1), (0x121, 5, -1), (0x12F, 0, 1)]], gs, rs)
    assert r == [0, 0]
    _, _, _, r, _ = run_stream(
        ctx, fill + [[(0x120, 0, -1), (0x121, 5, -1), (0x111, 0, 1)]], gs, rs)
    assert r == [0, 1]


# ---- shift edges, group 0 and the all-ones group ----

def test_rank_shift_equals_group_shift_the_whole_group_ties(ctx):
    s = 12
    ticks = [[(0x1000 | i, i, 1 + i % 3) for i in range(300)] +
             [(0x2000, 0, 1)],
             [(0x1000 | 255, 255, -(1 + 255 % 3)), (0x1003, 9, 1)],
             [(0x2000, 0, -1)]]
    _, _, model, refills, outs = run_stream(ctx, ticks, s, s)
    assert len(outs[0]) == 301 and len(outs[1]) == 2
    assert refills == [0, 0, 1]
    assert model.acc == model.integral


def test_rank_shift_0_and_group_shift_0(ctx):
    ticks = [[(k, v, 1) for k in (0, 1, 5, ONES) for v in range(4)],
             [(5, 3, -1), (ONES, 3, -1), (0, 9, 1)],
             [(1, v, -1) for v in range(4)] + [(ONES, 0, 2)]]
    _, _, model, refills, _ = run_stream(ctx, ticks, 0, 0)
    # with shift 0 a key is its own group and all its rows tie
    assert refills == [0, 0, 1]
    assert model.acc == model.integral


def test_group_shift_63(ctx):
    hi = 1 << 63
    for rs in (0, 5, 63):
        ticks = [[(0, 0, 1), (5, 1, 1), (hi - 1, 0, 1), (hi, 0, 1),
                  (hi | 77, 0, 1), (ONES, ONES, 1)],
                 [(hi - 1, 0, -1), (ONES, ONES, -1)],
                 [(3, 3, 1), (ONES - 1, 3, 1)]]
        _, _, model, refills, _ = run_stream(ctx, ticks, 63, rs)
        assert refills == ([0, 2, 0] if rs < 63 else [0, 0, 0])
        if rs == 0:
            assert model.acc == {(5, 1): 1, (ONES - 1, 3): 1}


@pytest.mark.parametrize("gs,rs", [(8, 0), (27, 3), (59, 32)])
def test_group_0_and_the_all_ones_group(ctx, gs, rs):
    """The last group's range ends at 2^64 - 1: (g + 1) << shift would wrap
    to 0 and the range would come out empty or inverted."""
    top = ONES >> gs << gs                 # first key of the all-ones group
    ticks = [[(i, 0, 1) for i in range(5)] +
             [(top | i, 1, 1) for i in range(5)] + [(ONES, ONES, 1)],
             [(4, 0, -1), (ONES, ONES, -1), (top - 1, 0, 1)],
             [(ONES, 0, 1), (0, 0, -1)]]
    _, _, model, refills, _ = run_stream(ctx, ticks, gs, rs)
    if rs == 0:
        assert refills == [0, 2, 0]
    assert (ONES, 0) in model.acc and (top - 1, 0) in model.acc


# ---- presence ----

def test_presence_rules_across_spine_batches(ctx):
    gs, rs = 4, 0
    ticks = [[(0x10, 1, 1), (0x11, 0, 1), (0x12, 0, 1)],
             [(0x12, 0, 1)],        # 1 -> 2: +1
             [(0x12, 0, -1)],       # 2 -> 1: -1
             [(0x12, 0, -1)],       # +1 then -1 in another batch: vanish
             [(0x13, 5, -1)],       # net -1: present, at -1
             [(0x13, 5, 1)],        # -1 then +1: vanish
             [(0x21, 0, -1), (0x21, 0, 1)],     # consolidates to empty
             [],                                # n = 0
             [(0x10, 1, 2), (0x10, 1, -2)]]
    from dbsp_amd.engine import ArgMax
    op = ArgMax(ctx, gs, rs)
    outs = [zset(op.step(rows_of(t))) for t in ticks]
    st = op.stats()
    op.close()
    assert outs == [
        {(0x12, 0): 1}, {(0x12, 0): 1}, {(0x12, 0): -1},
        {(0x12, 0): -1, (0x11, 0): 1},
        {(0x13, 5): -1, (0x11, 0): -1},
        {(0x13, 5): 1, (0x11, 0): 1}, {}, {}, {}]
    assert st["groups_seen"] == 6 and st["groups_refilled"] == 2
    run_stream(ctx, ticks, gs, rs)


# ---- non-decreasing maxima read nothing ----

def test_non_decreasing_maxima_never_refill(ctx):
    """The operator's claim: an append-only stream with distinct rows, on
    which no group's maximum ever decreases, refills no group and gathers
    nothing from the input trace."""
    rng = np.random.default_rng(5)
    gs, rs = 16, 4
    seen, ticks = set(), []
    for _ in range(12):
        tick = []
        while len(tick) < 500:
            key = (int(rng.integers(0, 30)) << gs | int(rng.integers(0, 1 << gs)),
                   int(rng.integers(0, 4)))
            if key not in seen:
                seen.add(key)
                tick.append(key + (1,))
        ticks.append(tick)
    st, st_all, _, refills, _ = run_stream(ctx, ticks, gs, rs)
    assert st["groups_refilled"] == 0 and st["rows_gathered"] == 0
    assert sum(refills) == 0
    assert st_all["rows_gathered"] > st["in_rows"]   # the other route reads


# ---- sizes at the sort and merge edges ----

def _size_ticks(n):
    """Four ticks of n-row deltas over keys that are each their own group
    (shift 0, so all rows of a key tie): n keys, a slice of n rows; then
    every third key loses its only row and gains another, the rest of the n
    rows being new keys; then every key gains a row; then loses it again.
    No tick refills: a row of the old rank is always left or arrives."""
    k = np.arange(n, dtype=np.uint64) * np.uint64(3)
    t1 = np.empty(n, dtype=ROW_DT)
    t1["k"], t1["v"], t1["w"] = k, 5, 1
    third = k[::3]
    m = len(third)
    pad = n - 2 * m
    t2 = np.empty(n, dtype=ROW_DT)
    t2["k"] = np.concatenate([third, third,
                              np.arange(pad, dtype=np.uint64) * np.uint64(3)
                              + np.uint64(1)])
    t2["v"] = np.concatenate([np.full(m, 5), np.full(m, 9), np.zeros(pad)])
    t2["w"] = np.concatenate([np.full(m, -1), np.ones(m), np.ones(pad)])
    t3 = np.empty(n, dtype=ROW_DT)
    t3["k"], t3["v"], t3["w"] = k, 2, 1
    t4 = np.empty(n, dtype=ROW_DT)
    t4["k"], t4["v"], t4["w"] = k, 2, -1
    return [t1, t2[np.random.default_rng(n).permutation(n)], t3, t4]


@pytest.mark.parametrize("n", [1024, 1025, 2048, 2049, 8192, 8193, 65537])
def test_delta_and_slice_sizes(ctx, n):
    st, _, model, refills, _ = run_stream(ctx, _size_ticks(n), 0, 0)
    # with shift 0 the new row of tick 2 ties with the one that leaves
    assert refills == [0, 0, 0, 0]
    assert len(model.acc) == n + (n - 2 * len(range(0, n, 3)))


@pytest.mark.parametrize("n", [1025, 8193])
def test_refilled_slice_sizes(ctx, n):
    """n groups of two ranks lose their top row: n refills, whose runs hold n
    rows once consolidated and 3n while the batches are apart."""
    gs = 4
    k = np.arange(n, dtype=np.uint64) << np.uint64(gs)
    t1 = np.empty(2 * n, dtype=ROW_DT)
    t1["k"] = np.concatenate([k | np.uint64(1), k | np.uint64(9)])
    t1["v"], t1["w"] = 7, 2
    t2 = np.empty(n, dtype=ROW_DT)
    t2["k"], t2["v"], t2["w"] = k | np.uint64(9), 7, -2
    st, _, model, refills, _ = run_stream(ctx, [t1, t2], gs, 0)
    assert refills == [0, n] and n <= st["rows_gathered"] <= 3 * n
    assert len(model.acc) == n and set(model.acc.values()) == {2}


def test_hot_group_is_refilled(ctx):
    n, gs, rs = 20000, 20, 0
    t1 = np.empty(n + 50, dtype=ROW_DT)
    t1["k"] = np.concatenate([
        (np.uint64(7) << np.uint64(gs)) | np.arange(n, dtype=np.uint64),
        (np.uint64(8) << np.uint64(gs)) | np.arange(50, dtype=np.uint64)])
    t1["v"], t1["w"] = 3, 1
    top = (7 << gs) | (n - 1)
    ticks = [t1, [(top, 3, -1), ((8 << gs) | 5, 3, -1)]]
    st, _, model, refills, _ = run_stream(ctx, ticks, gs, rs)
    assert refills == [0, 1]
    assert ((7 << gs) | (n - 2), 3) in model.acc
    assert n - 2 <= st["rows_gathered"] <= n + 2


def test_many_single_row_ticks(ctx):
    gs, rs = 8, 0
    ticks = [[(0x100 | i, 0, 1)] for i in range(30)]
    ticks += [[(0x100 | i, 0, -1)] for i in range(29, 9, -1)]
    ticks += [[(0x300 | i, i, 1)] for i in range(10)]
    st, _, _, refills, _ = run_stream(ctx, ticks, gs, rs)
    assert len(ticks) > 2 * 24
    assert sum(refills) == 20


def test_random_stream_with_retractions(ctx):
    """120 ticks x ~200 rows over 40 groups, 30 % retractions;
    tests/test_argmax_model.py checks that this seed makes both verdicts
    occur at least 20 times each."""
    gs, rs = am.RANDOM_SHIFTS
    st, _, _, refills, _ = run_stream(
        ctx, am.random_stream(am.RANDOM_SEED), gs, rs)
    assert st["groups_refilled"] == sum(refills) >= 20


# ---- the batch primitive ----

def _np_argmax(rows, gs, rs):
    k = rows["k"]
    g = k >> np.uint64(gs)
    end = np.searchsorted(g, g, side="right")
    keep = (k[end - 1] >> np.uint64(rs)) == (k >> np.uint64(rs))
    return rows[keep].copy()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
@pytest.mark.parametrize("gs,rs", [(0, 0), (6, 2), (9, 9), (11, 1), (63, 0),
                                   (63, 62)])
def test_argmax_batch_against_numpy(ctx, n, gs, rs):
    rng = np.random.default_rng(n * 131 + gs * 7 + rs)
    # distinct sorted keys; with shift 6 / 9 / 11 a group holds up to 64 /
    # 512 / 2048 consecutive rows, so groups and tie sets straddle the
    # 256-thread blocks
    k = np.cumsum(rng.integers(1, 3, size=n)).astype(np.uint64)
    if gs == 63 and n:
        k[n // 2:] |= np.uint64(1 << 63)
    rows = np.empty(n, dtype=ROW_DT)
    rows["k"], rows["v"] = k, rng.integers(0, 1 << 40, size=n)
    rows["w"] = rng.choice(np.array([-3, -1, 1, 2]), size=n)
    got = ctx.argmax(rows, gs, rs)
    exp = _np_argmax(rows, gs, rs)
    assert got.tobytes() == exp.tobytes()


def test_argmax_batch_ties_inside_a_key(ctx):
    rows = rows_of([(ONES - 1, 0, 4)] + [(ONES, v, -1) for v in range(600)])
    got = ctx.argmax(rows, 1, 0)
    assert got["v"].tolist() == list(range(600))
    assert (got["w"] == -1).all() and (got["k"] == np.uint64(ONES)).all()


@pytest.mark.parametrize("gs,rs", [(-1, -1), (5, -1), (64, 3), (3, 5),
                                   (64, 64)])
def test_invalid_shifts_are_rejected(ctx, gs, rs):
    from dbsp_amd.engine import ArgMax
    with pytest.raises(RuntimeError):
        ArgMax(ctx, gs, rs)
    with pytest.raises(RuntimeError):
        ctx.argmax(rows_of([(1, 1, 1)]), gs, rs)


def test_unknown_flag_bits_are_rejected(ctx):
    import ctypes
    h = ctypes.c_void_p()
    for flags in (2, 3, 1 << 31):
        assert ctx._lib.dbsp_argmax_create(ctx._h, 8, 4, flags,
                                           ctypes.byref(h)) != 0
    assert ctx._lib.dbsp_argmax_create(ctx._h, 8, 4, 1, ctypes.byref(h)) == 0
    assert ctx._lib.dbsp_argmax_destroy(h) == 0
