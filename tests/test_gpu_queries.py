"""End-to-end GPU engine parity: Nexmark q3/q5/q8 ticked over generated event
streams, compared tick-by-tick against the CPU oracle (bit-exact Z-sets), plus
the reference's golden test vectors replayed through the engine."""
import numpy as np
import pytest

from dbsp_amd import gen, oracle
from helpers import (CITY_IDS, Intern, auction_event, bid_event, events,
                     load_golden, pack_person, person_event, rows_of,
                     state_id, zset)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dbsp_amd.engine import Ctx
    c = Ctx(0)
    yield c
    c.close()


def _tick_bounds(n, tick):
    """[lo, hi) per tick: `tick` is one size for all ticks or a list of
    sizes, one per tick."""
    if isinstance(tick, int):
        return [(lo, min(lo + tick, n)) for lo in range(0, n, tick)]
    ends = np.cumsum(tick)
    assert ends[-1] == n
    return [(int(hi - t), int(hi)) for t, hi in zip(tick, ends)]


def _run_parity(ctx, query, evs, tick, seed_note=""):
    """Tick by tick against the oracle; returns the oracle's outputs."""
    from dbsp_amd.engine import Engine
    eng = Engine(ctx, query=query)
    q = oracle.Query(query)
    eng.stage(evs)
    exps = []
    try:
        for lo, hi in _tick_bounds(len(evs), tick):
            eng.step_staged(lo, hi)
            got = eng.output()
            exp = q.step(evs[lo:hi], cap=1 << 22)
            assert zset(got) == zset(exp), (
                f"q{query}{seed_note}: tick [{lo},{hi}) diverged: "
                f"{len(got)} vs {len(exp)} rows")
            exps.append(exp)
    finally:
        # a failed tick must not leave the engine to be destroyed after the
        # module's ctx: dbsp_engine_destroy reads its ctx
        eng.close()
        q.close()
    return exps


@pytest.mark.parametrize("query", [3, 5, 8])
def test_query_parity_generated(ctx, query):
    evs = gen.generate(100_000, seed=11)
    _run_parity(ctx, query, evs, tick=10_000)


@pytest.mark.parametrize("query", [3, 5, 8])
def test_query_parity_small_ticks(ctx, query):
    # tiny ticks stress empty deltas / empty windows / single rows
    evs = gen.generate(2_000, seed=13)
    _run_parity(ctx, query, evs, tick=137)


def test_golden_q3_on_gpu(ctx):
    from dbsp_amd.engine import Engine
    g = load_golden("q3_people.json")
    intern = Intern()
    eng = Engine(ctx, query=3)
    for tick in g["ticks"]:
        evs = []
        for p in tick["persons"]:
            evs.append(person_event(p["id"], intern(p["name"]),
                                    CITY_IDS[p["city"]],
                                    state_id(p["state"], intern)))
        for a in tick["auctions"]:
            evs.append(auction_event(a["id"], a["seller"], a["category"]))
        eng.step(events(*evs))
        got = eng.output()
        expected = zset(rows_of([
            (pack_person(intern(name), CITY_IDS[city], state_id(st, intern)),
             aid, w) for name, city, st, aid, w in tick["expected"]]))
        assert zset(got) == expected
    eng.close()


def test_golden_q5_on_gpu(ctx):
    from dbsp_amd.engine import Engine
    g = load_golden("q5_hot_items.json")
    for case in g["cases"]:
        eng = Engine(ctx, query=5)
        for b1, b2, exp in zip(case["auction1_batches"],
                               case["auction2_batches"], case["expected"]):
            evs = [bid_event(1, dt) for dt in b1] + \
                  [bid_event(2, dt) for dt in b2]
            eng.step(events(*evs))
            got = eng.output()
            assert zset(got) == zset(rows_of([(a, n, w) for a, n, w in exp])), \
                case["name"]
        eng.close()


def test_golden_q8_on_gpu(ctx):
    from dbsp_amd.engine import Engine
    g = load_golden("q8_monitor_new_users.json")
    for case in g["cases"]:
        intern = Intern()
        eng = Engine(ctx, query=8)
        for pb, ab, exp in zip(case["people_batches"], case["auction_batches"],
                               case["expected"]):
            evs = [person_event(pid, intern(name), 0, 3, dt=dt)
                   for pid, name, dt in pb]
            evs += [auction_event(1, seller, 1, dt=dt) for seller, dt in ab]
            eng.step(events(*evs))
            got = eng.output()
            expected = zset(rows_of([
                (pid, (intern(name) << 32) | stime, w)
                for pid, name, stime, w in exp]))
            assert zset(got) == expected, case["name"]
        eng.close()


@pytest.mark.parametrize("query", [3, 5, 8])
def test_query_parity_with_retractions(ctx, query):
    """Streams carrying deletions: every third event of earlier ticks is
    re-issued later with weight -1 (the reference's Z-set deltas carry
    insertions AND retractions; generated streams alone only exercise w=+1)."""
    evs = gen.generate(30_000, seed=17)
    retract = evs[::3].copy()
    retract["w"] = -1
    mixed = np.concatenate([evs, retract])
    _run_parity(ctx, query, mixed, tick=6000, seed_note="+retractions")


def test_q3_duplicate_and_zero_weight_events(ctx):
    """Duplicate events (weights accumulate) and exact cancellations inside
    one tick (weight-zero elimination end to end)."""
    evs = gen.generate(5_000, seed=19)
    dup = evs[:2000].copy()
    neg = evs[:1000].copy()
    neg["w"] = -2
    mixed = np.concatenate([evs, dup, neg])
    _run_parity(ctx, 3, mixed, tick=1000, seed_note="+dups")


@pytest.mark.parametrize("query", [3, 5, 8])
def test_query_parity_at_scale(ctx, query):
    """2M events (50 reference-sized ticks): traces reach hundreds of
    thousands of rows, exercising spine cascades, the medium sort path and
    multi-batch probes end to end."""
    evs = gen.generate(2_000_000, seed=29)
    _run_parity(ctx, query, evs, tick=40_000)


def test_q0_host_path(ctx):
    """q0 runs the host plumbing path (BASELINE configs[0]: CPU, 1 worker)."""
    from dbsp_amd.engine import Engine
    evs = gen.generate(10_000, seed=3)
    eng = Engine(ctx, query=0)
    eng.stage(evs)
    eng.step_staged(0, 10_000)
    got = eng.output_events()
    exp = oracle.q0_step(evs)
    assert np.array_equal(got, exp)
    eng.close()


@pytest.mark.parametrize("query", [3, 5, 8])
def test_query_parity_oversized_deltas(ctx, query):
    """Ticks whose per-stream deltas exceed the fused-sort capacity (8192
    rows) and whose key boxes are too wide for the dense-range path: the
    chained single-rank tick loses its speculation (the sort kernels write
    the -1 sentinels) and must recover through the sized sort paths with
    the lengths read back at the tick sync."""
    from helpers import events
    rng = np.random.default_rng(53)
    evs = []
    for i in range(12_000):
        dt = 10_000_000 + i
        evs.append(person_event(int(rng.integers(0, 1 << 40)),
                                i % 997, i % 15, i % 6, dt=dt))
        evs.append(auction_event(int(rng.integers(0, 1 << 40)),
                                 int(rng.integers(0, 1 << 40)), 10 + i % 5,
                                 dt=dt))
        # wide auction ids reject the dense-range consolidate too
        evs.append(bid_event(int(rng.integers(0, 1 << 40)), dt))
    _run_parity(ctx, query, events(*evs), tick=30_000,
                seed_note="+oversized")


def _q8_one_big_stream(big):
    """Six q8 ticks, tick t with event times in [10_000_000 + 10_000 t,
    +9_100), so the window moves on every tick and tick t's output is tick
    t-2's join (entering) and tick t-3's (leaving).  Ticks 0, 1 and 5 hold 200
    rows of the `big` stream, ticks 2-4 hold 8200 (above the fused sort's 8192
    rows); the other stream holds 16 rows in every tick.  Returns the events
    and the tick sizes."""
    from dbsp_amd import EVENT_DT, KIND_AUCTION, KIND_PERSON
    ticks, sizes = [], []
    for t in range(6):
        nbig = 8200 if t in (2, 3, 4) else 200
        npers, nauc = (nbig, 16) if big == "persons" else (16, nbig)
        base = 10_000_000 + 10_000 * t
        p = np.zeros(npers, dtype=EVENT_DT)
        i = np.arange(npers, dtype=np.uint64)
        p["kind"], p["f0"], p["f1"] = KIND_PERSON, 100_000 * t + i, i % 997
        p["f2"], p["f3"], p["w"] = i % 10, i % 6, 1
        p["f4"] = base + i * 9_100 // npers
        a = np.zeros(nauc, dtype=EVENT_DT)
        j = np.arange(nauc, dtype=np.uint64)
        a["kind"], a["f0"] = KIND_AUCTION, 100_000 * t + j
        a["f1"] = 100_000 * t + 7 * j % min(npers, 200)
        a["f2"], a["f4"], a["w"] = 10 + j % 5, 2000, 1
        a["f3"] = base + j * 9_100 // nauc
        ticks += [p, a]
        sizes.append(npers + nauc)
    return np.concatenate(ticks), sizes


@pytest.mark.parametrize("big", ["persons", "auctions"])
def test_q8_parity_one_oversized_delta(ctx, big):
    """Only ONE of q8's two deltas overflows the fused sort, on ticks with a
    previous window and a moving one: the tick loses its speculation with
    the other delta's sort (and, persons big, the watermark update behind the
    auction delta) already good.  The oversized ticks' outputs carry both
    insertions and retractions."""
    evs, sizes = _q8_one_big_stream(big)
    exps = _run_parity(ctx, 8, evs, sizes, seed_note=f"+{big} big")
    assert all(len(zset(exp)) > 0 for exp in exps[2:5])


def test_q8_one_oversized_delta_run_staged(ctx):
    """The same persons-big stream through run_staged, so ticks 3 and 4 take
    a pipelined front and then lose its speculation."""
    from dbsp_amd.engine import Engine
    evs, sizes = _q8_one_big_stream("persons")
    q = oracle.Query(8)
    for lo, hi in _tick_bounds(len(evs), sizes):
        exp = q.step(evs[lo:hi], cap=1 << 22)
    q.close()
    eng = Engine(ctx, query=8)
    eng.stage(evs)
    lo = 0
    # one call per run of equal ticks: a call's ticks are of one size
    for first, count in ((0, 2), (2, 3), (5, 1)):
        assert sizes[first:first + count] == [sizes[first]] * count
        eng.run_staged(lo, lo + count * sizes[first], sizes[first])
        lo += count * sizes[first]
    assert lo == len(evs)
    got = eng.output()
    eng.close()
    assert len(zset(exp)) > 0
    assert zset(got) == zset(exp)


@pytest.mark.parametrize("query", [5, 8])
def test_query_parity_window_slides(ctx, query):
    """Accelerated event time: 200k events spanning 20s of event time, so the
    q5/q8 tumbling windows slide on ~every tick (the generated parity streams
    at the 10M/s rate never cross a 2s tumble inside 100k events). Exercises
    the 3-region retract/insert path and the device watermark end to end."""
    evs = gen.generate(200_000, seed=37)
    dt = (10_000_000 + np.arange(len(evs)) // 10).astype(np.uint64)
    person = evs["kind"] == 0
    bid_or_auction = ~person
    evs["f4"] = np.where(person, dt, evs["f4"])     # person dt
    evs["f3"] = np.where(bid_or_auction, dt, evs["f3"])  # auction/bid dt
    _run_parity(ctx, query, evs, tick=20_000, seed_note="+slides")


@pytest.mark.parametrize("query", [3, 5, 8])
def test_run_staged_matches_step_staged(ctx, query):
    """dbsp_engine_run_staged (the benchmark loop) pipelines consecutive
    ticks — the next tick's front half launches during this tick's tail and
    is consumed via the engine's front state. Per-tick step_staged never
    exercises that path, so run the same stream both ways and require the
    final outputs and a full-trace probe to agree (plus the oracle)."""
    from dbsp_amd.engine import Engine
    evs = gen.generate(200_000, seed=61)
    tick = 20_000
    eng_a = Engine(ctx, query=query)
    eng_a.stage(evs)
    for lo in range(0, len(evs), tick):
        eng_a.step_staged(lo, min(lo + tick, len(evs)))
    out_a = eng_a.output()
    eng_a.close()
    eng_b = Engine(ctx, query=query)
    eng_b.stage(evs)
    eng_b.run_staged(0, len(evs), tick)
    out_b = eng_b.output()
    eng_b.close()
    assert zset(out_a) == zset(out_b)
    q = oracle.Query(query)
    exp = None
    for lo in range(0, len(evs), tick):
        exp = q.step(evs[lo:min(lo + tick, len(evs))], cap=1 << 22)
    q.close()
    assert zset(out_b) == zset(exp)


@pytest.mark.parametrize("seed", [101, 211, 307])
@pytest.mark.parametrize("query", [3, 5, 8])
def test_query_parity_fuzz_seeds(ctx, query, seed):
    """Seed sweep at an irregular tick size: different generator seeds shift
    the person/auction/bid id interleavings, hot-key draws and timestamp
    boundaries that the sized sort/dense/window routing keys off."""
    evs = gen.generate(60_000, seed=seed)
    _run_parity(ctx, query, evs, tick=7_777, seed_note=f"+fuzz{seed}")


def test_query_parity_generated_q4(ctx):
    evs = gen.generate(100_000, seed=11)
    _run_parity(ctx, 4, evs, tick=10_000)


def test_query_parity_small_ticks_q4(ctx):
    evs = gen.generate(2_000, seed=13)
    _run_parity(ctx, 4, evs, tick=137)


def test_golden_q4_on_gpu(ctx):
    """The reference's q4 test (queries/q4.rs:94-239) through the engine."""
    import sys
    from dbsp_amd.engine import Engine
    from test_oracle import _q4_golden_events
    g = load_golden("q4_category_avg.json")
    eng = Engine(ctx, query=4)
    for t, tick in enumerate(g["ticks"]):
        evs = _q4_golden_events(tick)
        eng.step(evs)
        got = zset(eng.output())
        exp = {(int(k), int(v)): int(w) for k, v, w in tick["expected"]}
        assert got == exp, f"tick {t}: {got} != {exp}"
    eng.close()


def test_query_parity_generated_q6(ctx):
    evs = gen.generate(100_000, seed=11)
    _run_parity(ctx, 6, evs, tick=10_000)


def test_golden_q6_on_gpu(ctx):
    """The reference's q6 tests (queries/q6.rs) through the engine."""
    from dbsp_amd.engine import Engine
    from test_oracle import _q6_golden_events
    g = load_golden("q6_seller_avg.json")
    for case in g["cases"]:
        eng = Engine(ctx, query=6)
        for t, tick in enumerate(case["ticks"]):
            eng.step(_q6_golden_events(tick))
            got = zset(eng.output())
            exp = {(int(k), int(v)): int(w) for k, v, w in tick["expected"]}
            assert got == exp, f'{case["name"]} tick {t}: {got} != {exp}'
        eng.close()
