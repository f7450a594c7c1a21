#!/usr/bin/env python3
"""bench.py — Nexmark events/s on the MI355X-native DBSP engine.

A "step" is one clock tick of the flagship query (default q3, the workload
BASELINE.json's metric is quoted on for one GPU: "Nexmark q3 stream-table
join, 10M synthetic events, i64 keys, 1 MI355X") over one tick_events-sized
batch of synthetic events — the reference feeds 40k-event batches per tick
(crates/nexmark/src/config.rs:108-109).  All (warmup+steps) ticks' events are
generated up front and staged to HBM before the timed region; the tick
pipeline (flat_map build, sort+consolidate, trace merges, joins, output
consolidate) runs entirely on-GPU inside the timed region.

Single GPU:   python bench.py --steps 250 --warmup 10
Multi GPU:    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
                  --master-addr 127.0.0.1 bench.py --gpus N ...
(one rank per GPU; deltas are key-sharded across ranks with an RCCL
all-to-all-v over xGMI; weak scaling: each rank processes tick_events per
tick, so the whole job covers tick_events*N events per step).

A plain run does only what the headline figure needs: generate + stage the
events, warm up, time --steps ticks, print the line.  --full adds the
cpu_baseline and roofline legs (each a run of its own).  --dump-outputs DIR
writes the output delta of the last timed tick as DIR/<column>.npy.

Rank 0 prints ONE JSON line (driver contract).
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "database-stream-processor_amd" / "python"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# Reference's published q3 number (9,936,407 events/s on an
# unnamed 16-core CPU — the only published figure for this metric).
PUBLISHED = {3: 9_936_407.0, 4: 9_768_487.0, 5: 9_906_875.0, 6: 9_829_942.0,
             8: 9_380_863.0, 0: 9_926_544.0}


def generate_events(total, seed=1):
    from dbsp_amd import gen
    return gen.generate(total, seed=seed)


def generate_rank_slices(n_ticks, tick, world, rank, seed=1):
    """Each rank keeps only its own tick-sized slice of the global stream
    (tick t covers global events [t*tick*world, (t+1)*tick*world); rank r owns
    the r-th tick-sized slice).  Generation itself is sequential and cheap;
    storing the full stream at N=8 would cost ~5 GB/rank."""
    import numpy as np
    from dbsp_amd import gen
    if world == 1:
        return gen.generate(n_ticks * tick, seed=seed)
    st = gen.Stream(seed=seed)
    out = []
    for _ in range(n_ticks):
        chunk = st.next(tick * world)
        out.append(chunk[rank * tick:(rank + 1) * tick].copy())
    st.close()
    return np.concatenate(out)


DUMP_MAX_BYTES = 64 << 20  # --dump-outputs budget over all files


def _exact_f64(name, col):
    """An 8-byte integer column as float64 array(s) without losing bits:
    one array while every value is within +-2^53, else the 32-bit halves of
    the two's-complement pattern as <name>_hi / <name>_lo."""
    import numpy as np
    lim = 1 << 53
    if col.dtype == np.uint64:
        exact = bool((col <= lim).all())
    else:
        exact = bool(((col >= -lim) & (col <= lim)).all())
    if exact:
        return {name: col.astype(np.float64)}
    u = col.view(np.uint64)
    return {name + "_hi": (u >> np.uint64(32)).astype(np.float64),
            name + "_lo": (u & np.uint64(0xFFFFFFFF)).astype(np.float64)}


def dump_outputs(out_dir, rows, f64_cols=()):
    """Write what the timed path's last tick handed its caller (the output
    delta Z-set, or q0's event Z-set) as one float64 .npy per column.  A Z-set
    is unordered, so rows go out in canonical column-lexicographic order;
    columns named in f64_cols hold f64 bit patterns and are written as those
    doubles.  Past DUMP_MAX_BYTES a fixed seeded row sample (of the ordered
    rows) is written instead, with its row indices in sample_index.npy."""
    import numpy as np
    names = rows.dtype.names
    rows = rows[np.lexsort([rows[n] for n in reversed(names)])]
    cols = {}
    for n in names:
        col = np.ascontiguousarray(rows[n])
        if n in f64_cols:
            cols[n] = col.view(np.float64)
        else:
            cols.update(_exact_f64(n, col))
    max_rows = DUMP_MAX_BYTES // (8 * (len(cols) + 1))
    if len(rows) > max_rows:
        idx = np.sort(np.random.default_rng(0).choice(
            len(rows), size=max_rows, replace=False))
        cols = {n: c[idx] for n, c in cols.items()}
        cols["sample_index"] = idx.astype(np.float64)
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    for n, c in cols.items():
        np.save(out_dir / f"{n}.npy", c)


def _dump_dir(args, rank, world):
    """--dump-outputs target of this rank (one sub-directory per rank when
    the job is sharded), or None."""
    if args.dump_outputs is None:
        return None
    d = Path(args.dump_outputs)
    return d if world == 1 else d / f"rank{rank}"


def run_engine(ctx_dev, query, events, n_ticks, tick, world, rank, nccl_id,
               timed_ticks, dist=None):
    """Stage events; run warmup then timed ticks; return (elapsed_s, engine)."""
    import torch
    from dbsp_amd.engine import Ctx, Engine

    ctx = Ctx(ctx_dev)
    if world > 1 or os.environ.get("DBSP_FORCE_SHARD") == "1":
        import ctypes
        import numpy as np
        if nccl_id is None:  # forced single-rank sharding (self-exchange)
            nccl_id = np.zeros(128, dtype=np.uint8)
            ctx._lib.dbsp_comm_unique_id.restype = ctypes.c_int32
            assert ctx._lib.dbsp_comm_unique_id(
                nccl_id.ctypes.data_as(ctypes.c_void_p)) == 0
        ctx._lib.dbsp_comm_init.restype = ctypes.c_int32
        st = ctx._lib.dbsp_comm_init(ctx._h, rank, world,
                                     nccl_id.ctypes.data_as(ctypes.c_void_p))
        assert st == 0, "dbsp_comm_init failed"
    eng = Engine(ctx, query=query, rank=rank, world=world)
    eng.stage(events)

    warmup_ticks = n_ticks - timed_ticks
    eng.run_staged(0, warmup_ticks * tick, tick)
    ctx.sync()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    eng.run_staged(warmup_ticks * tick, n_ticks * tick, tick)
    ctx.sync()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
    return elapsed, eng, ctx


def _shard_filter(evs, query, world, rank):
    """Key-shard an event stream for one oracle worker, at the same points
    the reference calls shard() (communication/shard.rs:88; join/aggregate
    inputs are single-key, so per-shard sub-circuits union to the global
    result — the reference's own multi-worker argument, shard.rs:35-60).
    Partition is key%world (any deterministic partition is result-invariant;
    xxh3 only matters for per-rank comparability)."""
    import numpy as np
    kind = evs["kind"]
    if query == 3:
        # persons by id (f0), auctions by seller (f1); bids are dropped by
        # q3's flat_map anyway (queries/q3.rs:39-52)
        keep = ((kind == 0) & (evs["f0"] % world == rank)) | \
               ((kind == 1) & (evs["f1"] % world == rank))
    elif query in (4, 6):
        # auctions and bids both by auction id (queries/q4.rs:45-56,
        # q6.rs:46-57)
        keep = ((kind == 1) | (kind == 2)) & (evs["f0"] % world == rank)
    elif query == 5:
        # bids by auction id (queries/q5.rs:67-88)
        keep = (kind == 2) & (evs["f0"] % world == rank)
    elif query == 8:
        keep = ((kind == 0) & (evs["f0"] % world == rank)) | \
               ((kind == 1) & (evs["f1"] % world == rank))
    else:
        keep = np.ones(len(evs), dtype=bool)
    return evs[keep]


_BASE_EVS = None  # fork-shared (COW) event stream for baseline workers


def _baseline_worker(args):
    """One oracle worker: scan the full stream (the shard filter is the
    worker's share of the flat_map+partition work), run its key-shard."""
    import time as _t
    from dbsp_amd import oracle
    query, tick, world, rank, n_ticks = args
    evs = _BASE_EVS
    q = oracle.Query(query)
    t0 = _t.perf_counter()
    for t in range(n_ticks):
        sl = _shard_filter(evs[t * tick:(t + 1) * tick], query, world, rank)
        q.step(sl, cap=1 << 22)
    dt = _t.perf_counter() - t0
    q.close()
    return dt


def cpu_baseline_leg(query, tick, budget_s=30.0):
    """Time the CPU oracle (the restatement of the crates/dbsp algorithms —
    kind 'port') on a bounded sample of the same workload: the same 10M-event
    stream the GPU runs.  Two legs: single-core, and all host cores as N
    key-sharded worker processes (the reference's multi-worker model,
    one circuit per worker, shard.rs:35-60; per-query watermark/window state
    is per-worker).  Reported, not the optimisation target."""
    import multiprocessing as mp
    import os as _os
    global _BASE_EVS
    from dbsp_amd import oracle
    sample_events = 250 * tick  # the full default workload (10M events)
    evs = generate_events(sample_events, seed=1)
    q = oracle.Query(query)
    t0 = time.perf_counter()
    done = 0
    for lo in range(0, sample_events, tick):
        q.step(evs[lo:lo + tick], cap=1 << 22)
        done = lo + tick
        if time.perf_counter() - t0 > budget_s:
            break
    dt = time.perf_counter() - t0
    q.close()
    one_core = done / dt
    # all-cores leg: N forked workers, each runs its key-shard sub-circuit
    # over the same global prefix; whole-job rate = events / max-over-workers.
    # Worker count is capped: each worker's shard filter scans the full
    # stream (its share of the flat_map+partition work), so beyond ~32
    # workers the duplicated scans saturate host memory bandwidth and the
    # figure REGRESSES (measured: 256 workers ran 5x slower than 1 core).
    hw_cores = _os.cpu_count() or 1
    cores = min(hw_cores, 32)
    n_ticks = done // tick
    _BASE_EVS = evs
    try:
        ctx = mp.get_context("fork")
        with ctx.Pool(cores) as pool:
            worker_s = pool.map(
                _baseline_worker,
                [(query, tick, cores, r, n_ticks) for r in range(cores)])
        allcores = n_ticks * tick / max(worker_s)
    finally:
        _BASE_EVS = None
    return {
        "value": round(max(allcores, one_core), 1),
        "unit": "events/s",
        "cores": cores if allcores >= one_core else 1,
        "hw_cores": hw_cores,
        "kind": "port",
        "one_core_value": round(one_core, 1),
        "all_cores_value": round(allcores, 1),
        "sample": f"oracle q{query} over {n_ticks * tick} events; "
                  f"{cores} key-sharded worker processes of {hw_cores} "
                  f"hw cores (max-over-workers {max(worker_s):.2f}s; "
                  f"per-worker full-stream shard filter is memory-bound "
                  f"beyond ~32 workers); 1-core leg {done} events in "
                  f"{dt:.2f}s (C++ restatement of the crates/dbsp operators)",
    }


def roofline_leg(query, events, n_ticks, tick):
    """Re-run the same workload with DBSP_PROFILE=1 (hipEvent timing per
    kernel class on the engine stream) and derive achieved algorithmic GB/s of
    the dominant kernel class (trace merge)."""
    os.environ["DBSP_PROFILE"] = "1"
    elapsed, eng, ctx = run_engine(0, query, events, n_ticks, tick, 1, 0, None,
                                   timed_ticks=n_ticks)
    classes = {0: "sort_consolidate", 1: "merge", 2: "join", 3: "aggregate",
               4: "window"}
    stats = {name: eng.kernel_stats(k) for k, name in classes.items()}
    eng.close()
    ctx.close()
    os.environ.pop("DBSP_PROFILE", None)
    # dominant class by device ms
    dom = max(stats.items(), key=lambda kv: kv[1][0])
    name, (ms, by, ln) = dom
    achieved = (by / 1e9) / (ms / 1e3) if ms > 0 else 0.0
    return {
        "bound": "hbm",
        "kernel_class": name,
        "achieved": round(achieved, 2),
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4),
        "traffic": None,  # PMC pass collected separately (profiles/)
        "regime": "latency-bound (40k-event ticks: per-launch batches are "
                  "thousands of rows; the HBM-bound regime is the trace "
                  "merge at C5/kbench scale — see profiles/r02_merge_pmc.txt "
                  "and the c5 workload's roofline)",
        "detail": {k: {"ms": round(v[0], 2), "algo_GB": round(v[1] / 1e9, 3),
                       "launches": v[2]} for k, v in stats.items()},
    }


def c5_cpu_baseline(n_trace, n_delta, seed, budget_s=25.0):
    """CPU oracle leg for C5 (kind 'port'): the same trace (numpy
    regeneration of the device generator) probed by a bounded slice of the
    first delta through the same join -> weigh -> consolidate -> aggregate
    pipeline, scaled to delta rows/s.  Falls back to a smaller trace if the
    host can't hold n_trace rows (24 GB at 1B)."""
    import numpy as np
    sys.path.insert(0, str(ROOT / "tests"))
    from test_gpu_c5 import c5_gen, c5_oracle_tick
    from dbsp_amd import ROW_DT
    nt = n_trace
    while True:
        try:
            trace = c5_gen(nt, 5, 4, seed, 0)
            break
        except MemoryError:
            nt //= 4
    stride = max(3, (5 * n_trace) // n_delta)
    dseed = (seed + 0x9E3779B97F4A7C15) % (1 << 64)
    # bounded sample: slices of the first tick's delta until ~budget_s
    wint = np.empty(0, dtype=ROW_DT)
    out_trace = np.empty(0, dtype=ROW_DT)
    slice_rows = 1_000_000
    done = 0
    t0 = time.perf_counter()
    full = c5_gen(n_delta, stride, stride - 1, dseed, 1)
    while done < n_delta and time.perf_counter() - t0 < budget_s:
        sl = full[done:done + slice_rows]
        wint, out_trace, _ = c5_oracle_tick(trace, wint, out_trace, sl)
        done += len(sl)
    dt = time.perf_counter() - t0
    return {
        "value": done / dt,
        "unit": "delta rows/s",
        "cores": 1,
        "kind": "port",
        "sample": f"oracle C5 pipeline: {done} delta rows vs a {nt}-row "
                  f"trace in {dt:.1f}s (single-threaded C++ restatement"
                  + ("" if nt == n_trace else f"; trace cut to {nt} rows "
                     "for host RAM") + ")",
    }


def run_c5(args, rank, world, local_rank, dist):
    """Config C5 (BASELINE configs[4]) as an engine workload: a step = one
    n_delta-row device-generated delta joined incrementally against the
    n_trace-row trace with the f64 sum aggregate + upsert.  N>1 = weak
    scaling over key-disjoint shard replicas (rank-salted seeds; the path
    partitions with no data-path collective)."""
    import torch
    from dbsp_amd.engine import Ctx, Engine
    n_ticks = args.warmup + args.steps
    nd = args.tick

    def one_run(warm, timed, dump_dir=None):
        ctx = Ctx(local_rank)
        eng = Engine(ctx, query=100, rank=rank, world=world)
        eng.c5_init(args.c5_trace, nd, seed=args.seed + rank * 7919)
        eng.run_staged(0, warm * nd, nd)
        ctx.sync()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        t0 = time.perf_counter()
        eng.run_staged(warm * nd, (warm + timed) * nd, nd)
        ctx.sync()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        el = time.perf_counter() - t0
        st = {name: eng.kernel_stats(k) for k, name in
              {0: "sort_consolidate", 1: "merge", 2: "join",
               3: "aggregate"}.items()}
        if dump_dir is not None:
            # (key, f64 sum bits, weight) rows: per touched key at most one
            # insertion and one retraction of the previous sum
            dump_outputs(dump_dir, eng.output(cap=2 * nd + 1024),
                         f64_cols=("v",))
        eng.close()
        ctx.close()
        return el, st

    elapsed, _ = one_run(args.warmup, args.steps, _dump_dir(args, rank, world))
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    stats = None
    if args.full and world == 1:
        # per-kernel-class hipEvent timing needs DBSP_PROFILE=1 at ctx
        # creation: collect it from a short separate run
        os.environ["DBSP_PROFILE"] = "1"
        _, stats = one_run(1, min(args.steps, 5))
        os.environ.pop("DBSP_PROFILE", None)
    if rank != 0:
        return
    timed_rows = args.steps * nd * world
    value = timed_rows / elapsed
    if stats:
        # dominant class among those with an algorithmic-byte model (the
        # aggregate class times its probe kernels but carries no byte figure)
        dom = max(stats.items(), key=lambda kv: kv[1][1])
        name, (ms, by, ln) = dom
        achieved = (by / 1e9) / (ms / 1e3) if ms > 0 else 0.0
    else:
        name, achieved, stats = "unprofiled", 0.0, {}
    result = {
        "metric": "C5 delta rows/s",
        "value": round(value, 1),
        "unit": "delta rows/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1000, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": "c5-incremental-join-f64-sum",
            "trace_rows": args.c5_trace,
            "delta_rows": nd,
            "parallelism": f"keyshard{world}" if world > 1 else "single",
        },
        "roofline": {
            "bound": "hbm",
            "kernel_class": name,
            "achieved": round(achieved, 2),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": None,
            "detail": {k: {"ms": round(v[0], 2),
                           "algo_GB": round(v[1] / 1e9, 3),
                           "launches": v[2]} for k, v in stats.items()},
        },
    }
    if args.full and world == 1:
        result["cpu_baseline"] = c5_cpu_baseline(args.c5_trace, nd, args.seed)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed ticks (default 250; c5: 20)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--query", default="3",
                    choices=["0", "3", "4", "5", "6", "8", "c5"])
    ap.add_argument("--tick", type=int, default=None,
                    help="events (c5: delta rows) per tick "
                         "(default 40000; c5: 10M)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--c5-trace", type=int, default=1_000_000_000,
                    help="C5 trace rows (configs[4]: 1B)")
    ap.add_argument("--full", action="store_true",
                    help="also run the cpu_baseline and roofline legs")
    ap.add_argument("--no-extras", action="store_true",
                    help="accepted for old command lines; the extra legs "
                         "only run with --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed tick's output as DIR/*.npy")
    args = ap.parse_args()
    if args.steps is not None and args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", str(args.gpus)))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    # configs[4] (c5): a step = one 10M-row delta; --tick keeps its meaning as
    # rows per step, defaulting to the config's 10M (not the Nexmark 40k)
    c5 = args.query == "c5"
    if args.tick is None:
        args.tick = 10_000_000 if c5 else 40_000
    if args.steps is None:
        args.steps = 20 if c5 else 250
    if not c5:
        args.query = int(args.query)

    cpu_baseline = None
    if args.full and world == 1 and not c5 and args.query != 0:
        # first, while this process has not opened the GPU: the all-cores
        # leg forks its workers, and they would inherit the open device
        cpu_baseline = cpu_baseline_leg(args.query, args.tick)

    import torch
    if torch.cuda.is_available():
        # keep torch's notion of the current device aligned with the rank's
        # GPU, so the bracketing torch.cuda.synchronize() syncs the right one
        torch.cuda.set_device(local_rank)

    dist = None
    nccl_id = None
    if world > 1:
        import numpy as np
        import torch.distributed as tdist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        tdist.init_process_group("gloo")
        dist = tdist
        import ctypes
        from dbsp_amd.engine import _L
        buf = np.zeros(128, dtype=np.uint8)
        if rank == 0:
            L = _L()
            L.dbsp_comm_unique_id.restype = ctypes.c_int32
            assert L.dbsp_comm_unique_id(
                buf.ctypes.data_as(ctypes.c_void_p)) == 0
        import torch
        t = torch.from_numpy(buf)
        tdist.broadcast(t, src=0)
        nccl_id = t.numpy()

    if c5:
        run_c5(args, rank, world, local_rank, dist)
        return

    n_ticks = args.warmup + args.steps
    events = generate_rank_slices(n_ticks, args.tick, world, rank,
                                  seed=args.seed)

    elapsed, eng, ctx = run_engine(local_rank, args.query, events, n_ticks,
                                   args.tick, world, rank, nccl_id,
                                   timed_ticks=args.steps, dist=dist)
    # MAX over ranks
    if dist is not None:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    dump_dir = _dump_dir(args, rank, world)
    if dump_dir is not None:
        dump_outputs(dump_dir, eng.output_events(cap=args.tick + 16)
                     if args.query == 0 else eng.output())
    eng.close()
    ctx.close()

    if rank != 0:
        return

    timed_events = args.steps * args.tick * world
    value = timed_events / elapsed
    result = {
        "metric": "Nexmark events/s",
        "value": round(value, 1),
        "unit": "events/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1000, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": round(value / PUBLISHED[args.query], 3),
        "dtype": "int64",
        "data": "synthetic",
        "config": {
            "workload": f"nexmark-q{args.query}",
            "events_timed": timed_events,
            "tick_events": args.tick,
            "parallelism": f"keyshard{world}" if world > 1 else "single",
        },
    }
    if cpu_baseline is not None:
        result["cpu_baseline"] = cpu_baseline
        result["roofline"] = roofline_leg(args.query, events, n_ticks, args.tick)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
