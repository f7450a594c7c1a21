"""The incremental top-K per group operator (dbsp_topk_op) and its batch
primitive (dbsp_topk) on the GPU, against the dict model of
tests/topk_model.py.

Every operator test runs its stream through a default operator and a
refill_all one: per-tick outputs byte-equal between the two and equal to the
model, every output sorted, distinct and non-zero, the accumulated output
equal to dbsp_topk over the model's final integral, and groups_refilled equal
to the model's count of the verdict rule."""
import numpy as np
import pytest

import topk_model as tm
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


def run_stream(ctx, ticks, K, shift):
    """The contract in the module docstring; returns (default stats,
    refill_all stats, model, per-tick model refill counts)."""
    from dbsp_amd.engine import TopK
    op_d = TopK(ctx, K, shift)
    op_r = TopK(ctx, K, shift, refill_all=True)
    model = tm.Model(K, shift)
    acc, refills, touched = {}, [], 0
    try:
        for i, delta in enumerate(ticks):
            rows = _rows(delta)
            got_d, got_r = op_d.step(rows), op_r.step(rows)
            assert got_d.tobytes() == got_r.tobytes(), f"tick {i}"
            _assert_consolidated(got_d)
            exp, n_refill, n_groups = model.step(_triples(delta))
            assert _zset(got_d) == exp, f"tick {i}"
            assert set(got_d["w"].tolist()) <= {1, -1}
            acc = tm.zset_add(acc, exp)
            refills.append(n_refill)
            touched += n_groups
        st_d, st_r = op_d.stats(), op_r.stats()
    finally:
        op_d.close()
        op_r.close()
    assert acc == model.acc
    recomputed = ctx.topk(_integral_rows(model.integral), K, shift)
    _assert_consolidated(recomputed)
    assert _zset(recomputed) == acc
    assert st_d["groups_refilled"] == sum(refills)
    assert st_d["groups_seen"] == touched == st_r["groups_seen"]
    assert st_r["groups_refilled"] == touched
    assert st_d["in_rows"] == st_r["in_rows"]
    assert st_d["in_batches"] <= 24 and st_d["out_batches"] <= 24
    if sum(refills) == 0:
        assert st_d["rows_gathered"] == 0
    return st_d, st_r, model, refills


# ---- group sizes around K ----

@pytest.mark.parametrize("K", [1, 3, 10])
def test_groups_of_k_minus_1_k_and_k_plus_1(ctx, K):
    s = 8
    tick = []
    for g, size in enumerate((max(K - 1, 0), K, K + 1), start=1):
        tick += [((g << s) | i, 7, 1) for i in range(size)]
    # then each group gains one row above and loses its top row
    tick2 = [((g << s) | 200, 0, 1) for g in (1, 2, 3)]
    tick3 = [((g << s) | 200, 0, -1) for g in (1, 2, 3)]
    _, _, model, refills = run_stream(ctx, [tick, tick2, tick3], K, s)
    assert len(model.acc) == (K - 1) + K + K
    # tick 3: every group holds at least K rows by now and loses its top one
    assert refills == [0, 0, 3]


def test_k_larger_than_every_group(ctx):
    ticks = [[(g << 4 | i, i, 1) for g in range(5) for i in range(3)],
             [(g << 4 | 1, 1, -1) for g in range(5)],
             [(g << 4 | 9, 0, 2) for g in range(5)]]
    st, _, model, _ = run_stream(ctx, ticks, 65536, 4)
    assert st["groups_refilled"] == 0
    assert model.acc == {key: 1 for key in model.integral}


# ---- group_shift edges, group 0 and the all-ones group ----

def test_shift_0_every_key_its_own_group(ctx):
    ticks = [[(k, v, 1) for k in (0, 1, 5, ONES) for v in range(4)],
             [(5, 3, -1), (ONES, 3, -1), (0, 9, 1)],
             [(1, 2, -1), (ONES, 0, -1)]]
    _, _, model, refills = run_stream(ctx, ticks, 2, 0)
    assert refills == [0, 2, 1]   # tick 3: (ONES, 0) is below the threshold
    assert (ONES, 2) in model.acc and (0, 9) in model.acc


def test_shift_63_two_groups(ctx):
    hi = 1 << 63
    ticks = [[(0, 0, 1), (5, 1, 1), (hi - 1, 0, 1), (hi, 0, 1),
              (hi | 77, 0, 1), (ONES, ONES, 1)],
             [(hi - 1, 0, -1), (ONES, ONES, -1)],
             [(3, 3, 1), (hi | 3, 3, 1)]]
    _, _, model, refills = run_stream(ctx, ticks, 2, 63)
    assert refills == [0, 2, 0]
    assert set(model.acc) == {(3, 3), (5, 1), (hi | 3, 3), (hi | 77, 0)}


@pytest.mark.parametrize("shift", [8, 27])
def test_group_0_and_the_all_ones_group(ctx, shift):
    """The last group's range ends at 2^64 - 1: (g + 1) << shift would wrap
    to 0 and the range would come out empty or inverted."""
    top = ONES >> shift << shift          # first key of the all-ones group
    ticks = [[(i, 0, 1) for i in range(5)] +
             [(top | i, 1, 1) for i in range(5)] + [(ONES, ONES, 1)],
             [(4, 0, -1), (ONES, ONES, -1), (top - 1, 0, 1)],
             [(ONES, 0, 1), (0, 0, -1)]]
    _, _, model, refills = run_stream(ctx, ticks, 3, shift)
    assert refills == [0, 2, 0]
    assert (ONES, 0) in model.acc and (top - 1, 0) in model.acc


# ---- presence ----

def test_presence_rules_across_spine_batches(ctx):
    s = 4
    ticks = [[(0x10, 1, 1), (0x11, 0, 1), (0x12, 0, 1)],
             [(0x12, 0, 1)],        # 1 -> 2: no output
             [(0x12, 0, -1)],       # 2 -> 1: no output
             [(0x12, 0, -1)],       # +1 then -1 in another batch: vanish
             [(0x13, 5, -1)],       # net -1: present
             [(0x13, 5, 1)],        # -1 then +1: vanish
             [(0x21, 0, -1), (0x21, 0, 1)],     # consolidates to empty
             [],                                # n = 0
             [(0x10, 1, 2), (0x10, 1, -2)]]
    from dbsp_amd.engine import TopK
    op = TopK(ctx, 2, s)
    outs = [zset(op.step(rows_of(t))) for t in ticks]
    op.close()
    assert outs == [
        {(0x11, 0): 1, (0x12, 0): 1}, {}, {},
        {(0x12, 0): -1, (0x10, 1): 1},
        {(0x13, 5): 1, (0x10, 1): -1},
        {(0x13, 5): -1, (0x10, 1): 1}, {}, {}, {}]
    run_stream(ctx, ticks, 2, s)


# ---- the three verdict cases ----

def test_verdict_cases(ctx):
    K, s = 3, 8
    fill = [[(0x100 | i, 0, 1) for i in range(6)] +      # full group
            [(0x200 | i, 0, 1) for i in range(2)]]       # short group
    # a member of a full top-K vanishes: refill, the new member from below
    _, _, m, r = run_stream(ctx, fill + [[(0x104, 0, -1)]], K, s)
    assert r == [0, 1] and (0x102, 0) in m.acc
    # a row below the threshold of a full group vanishes: no refill
    st, _, m, r = run_stream(ctx, fill + [[(0x101, 0, -1)]], K, s)
    assert r == [0, 0] and st["rows_gathered"] == 0
    # a member of a short group vanishes: no refill
    st, _, m, r = run_stream(ctx, fill + [[(0x201, 0, -1)]], K, s)
    assert r == [0, 0] and st["rows_gathered"] == 0
    assert set(k for k in m.acc if k[0] >> s == 2) == {(0x200, 0)}
    # the refill gather reads the group's run, not the trace
    st, _, _, _ = run_stream(ctx, fill + [[(0x105, 0, -1)]], K, s)
    assert 5 <= st["rows_gathered"] <= 7


def test_appear_and_vanish_in_one_group_in_one_tick(ctx):
    K, s = 3, 8
    ticks = [[(0x100 | i, 0, 1) for i in range(6)],
             # below the threshold: out and in, the top-K stays
             [(0x100, 0, -1), (0x101, 5, 1)],
             # a member out, a higher row in, a lower row in
             [(0x104, 0, -1), (0x1F0, 0, 1), (0x100, 9, 1)],
             # every member out, two new ones in
             [(0x103, 0, -1), (0x105, 0, -1), (0x1F0, 0, -1), (0x1A0, 0, 1),
              (0x1A1, 0, 1)]]
    _, _, m, r = run_stream(ctx, ticks, K, s)
    assert r == [0, 0, 1, 1]
    assert set(m.acc) == {(0x102, 0), (0x1A0, 0), (0x1A1, 0)}


def test_append_only_never_refills(ctx):
    """The operator's claim: all weights +1, rows distinct -> no group is
    refilled and nothing is gathered from the input trace."""
    rng = np.random.default_rng(5)
    seen, ticks = set(), []
    for _ in range(12):
        tick = []
        while len(tick) < 500:
            key = (int(rng.integers(0, 30)) << 16 | int(rng.integers(0, 1 << 16)),
                   int(rng.integers(0, 4)))
            if key not in seen:
                seen.add(key)
                tick.append(key + (1,))
        ticks.append(tick)
    st, st_all, _, refills = run_stream(ctx, ticks, 10, 16)
    assert st["groups_refilled"] == 0 and st["rows_gathered"] == 0
    assert sum(refills) == 0
    assert st_all["rows_gathered"] > st["in_rows"]   # the other route reads


# ---- sizes at the sort and tree edges ----

def _size_ticks(n):
    """Three ticks whose deltas and candidate slices have n rows: n keys each
    their own group (shift 0); then every third key loses its only row and
    gains a higher one (n = 2 * ceil(n / 3) + ... rows padded to n with new
    keys); then every key gains a row."""
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
    return [t1, t2[np.random.default_rng(n).permutation(n)], t3]


@pytest.mark.parametrize("n", [1024, 1025, 2048, 2049, 8192, 8193, 65537])
def test_delta_and_slice_sizes(ctx, n):
    st, _, model, refills = run_stream(ctx, _size_ticks(n), 1, 0)
    assert refills[0] == 0 and refills[1] == len(range(0, n, 3))
    assert refills[2] == 0
    assert len(model.acc) == n + (n - 2 * len(range(0, n, 3)))


def test_hot_group_is_refilled(ctx):
    n, K, s = 20000, 10, 20
    t1 = np.empty(n + 50, dtype=ROW_DT)
    t1["k"] = np.concatenate([
        (np.uint64(7) << np.uint64(s)) | np.arange(n, dtype=np.uint64),
        (np.uint64(8) << np.uint64(s)) | np.arange(50, dtype=np.uint64)])
    t1["v"], t1["w"] = 3, 1
    top = (7 << s) | (n - 1)
    ticks = [t1, [(top, 3, -1)], [((7 << s) | (n - 5), 3, -1), (8 << s, 3, -1)]]
    st, _, model, refills = run_stream(ctx, ticks, K, s)
    assert refills == [0, 1, 1]
    assert ((7 << s) | (n - 12), 3) in model.acc
    assert 2 * (n - 2) <= st["rows_gathered"] <= 2 * (n + 2)


def test_many_single_row_ticks(ctx):
    K, s = 2, 8
    ticks = [[(0x100 | i, 0, 1)] for i in range(30)]
    ticks += [[(0x100 | i, 0, -1)] for i in range(29, 9, -1)]
    ticks += [[(0x300 | i, i, 1)] for i in range(10)]
    st, _, _, refills = run_stream(ctx, ticks, K, s)
    assert len(ticks) > 2 * 24
    assert sum(refills) == 20


def test_random_stream_with_retractions(ctx):
    """200 ticks x ~300 rows over 40 groups, 30 % retractions, K = 10;
    tests/test_topk_model.py checks that this seed makes both verdicts
    occur at least 20 times each."""
    st, _, _, refills = run_stream(ctx, tm.random_stream(tm.RANDOM_SEED), 10,
                                   20)
    assert st["groups_refilled"] == sum(refills) >= 20


# ---- the batch primitive ----

def _np_topk(rows, K, shift):
    g = rows["k"] >> np.uint64(shift)
    end = np.searchsorted(g, g, side="right")
    keep = end - np.arange(len(rows)) <= K
    out = rows[keep].copy()
    out["w"] = 1
    return out


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
@pytest.mark.parametrize("K,shift", [(1, 0), (10, 6), (300, 9), (65536, 63)])
def test_topk_batch_against_numpy(ctx, n, K, shift):
    rng = np.random.default_rng(n * 131 + K)
    # distinct sorted keys; with shift 6 / 9 a group holds up to 64 / 512
    # consecutive rows, so groups straddle the 256-thread blocks
    k = np.cumsum(rng.integers(1, 3, size=n)).astype(np.uint64)
    if shift == 63 and n:
        k[n // 2:] |= np.uint64(1 << 63)
    rows = np.empty(n, dtype=ROW_DT)
    rows["k"], rows["v"] = k, rng.integers(0, 1 << 40, size=n)
    rows["w"] = rng.choice(np.array([-3, -1, 1, 2]), size=n)
    got = ctx.topk(rows, K, shift)
    exp = _np_topk(rows, K, shift)
    assert got.tobytes() == exp.tobytes()


def test_topk_batch_ranks_by_v_inside_a_key(ctx):
    rows = rows_of([(ONES, v, -1) for v in range(600)])
    got = ctx.topk(rows, 257, 0)
    assert got["v"].tolist() == list(range(343, 600))
    assert (got["w"] == 1).all() and (got["k"] == np.uint64(ONES)).all()


@pytest.mark.parametrize("K,shift", [(0, 0), (-1, 3), (65537, 3), (5, -1),
                                     (5, 64)])
def test_invalid_k_and_shift_are_rejected(ctx, K, shift):
    from dbsp_amd.engine import TopK
    with pytest.raises(RuntimeError):
        TopK(ctx, K, shift)
    with pytest.raises(RuntimeError):
        ctx.topk(rows_of([(1, 1, 1)]), K, shift)
