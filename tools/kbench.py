#!/usr/bin/env python3
"""Kernel-scale roofline bench: drives the C-ABI primitives at the C5-class
sizes (1B-row trace, 10M-row delta) where the merge-path and
join kernels are HBM-bound, and reports achieved algorithmic GB/s against the
8 TB/s HBM3E peak.  torch is used only to materialize device operands
(sorted-unique keys via cumsum of positive gaps — no host staging).

Usage (on a GPU box):  python tools/kbench.py [--rows 500000000]
                       python tools/kbench.py --only rolling [--roll-rows N]
                       python tools/kbench.py --only rolling_wm
                       python tools/kbench.py --only rolling_minmax [--roll-rows N]
                       python tools/kbench.py --only topk [--topk-rows N ...]
                       python tools/kbench.py --only antijoin [--anti-rows N ...]
                       python tools/kbench.py --only argmax [--argmax-rows N ...]
Prints one JSON line per primitive.
"""
import argparse
import ctypes
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "database-stream-processor_amd" / "python"))

import torch  # noqa: E402

from dbsp_amd.engine import Ctx, BatchStruct, _L  # noqa: E402

HBM_PEAK_GBS = 8000.0


def sorted_unique_batch(n, seed, max_gap=8):
    g = torch.Generator(device="cuda").manual_seed(seed)
    gaps = torch.randint(1, max_gap, (n,), generator=g, dtype=torch.int64,
                         device="cuda")
    k = torch.cumsum(gaps, 0)
    v = torch.zeros(n, dtype=torch.int64, device="cuda")
    w = torch.where(
        torch.rand(n, generator=g, device="cuda") < 0.5,
        torch.tensor(1, dtype=torch.int64, device="cuda"),
        torch.tensor(-1, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    return k, v, w


def as_batch(k, v, w):
    b = BatchStruct()
    b.k = ctypes.c_void_p(k.data_ptr())
    b.v = ctypes.c_void_p(v.data_ptr())
    b.w = ctypes.c_void_p(w.data_ptr())
    b.len = len(k)
    return b


def bench_merge(ctx, L, n_per_side, reps=3):
    reps = int(os.environ.get("KB_REPS", reps))
    ka, va, wa = sorted_unique_batch(n_per_side, 1)
    kb, vb, wb = sorted_unique_batch(n_per_side, 2)
    a, b = as_batch(ka, va, wa), as_batch(kb, vb, wb)
    times = []
    n_out = 0
    for _ in range(reps):
        out = BatchStruct()
        ctx.sync()
        t0 = time.perf_counter()
        assert L.dbsp_merge(ctx._h, ctypes.byref(a), ctypes.byref(b),
                            ctypes.byref(out)) == 0
        ctx.sync()
        times.append(time.perf_counter() - t0)
        n_out = out.len
        ctx.free_batch(out)
    dt = min(times)
    algo_gb = 24.0 * (2 * n_per_side + n_out) / 1e9
    return {
        "primitive": "dbsp_merge (merge-path trace merge)",
        "rep_ms": [round(t * 1e3, 1) for t in times],
        "rows_in": 2 * n_per_side, "rows_out": n_out,
        "ms": round(dt * 1e3, 2), "algo_GB": round(algo_gb, 2),
        "achieved_GBs": round(algo_gb / dt, 1),
        "frac_of_peak": round(algo_gb / dt / HBM_PEAK_GBS, 4),
    }


def bench_join(ctx, L, n_trace, n_delta, reps=3):
    kt, vt, wt = sorted_unique_batch(n_trace, 3)
    kd, vd, wd = sorted_unique_batch(n_delta, 4,
                                     max_gap=max(2, (6 * n_trace) // n_delta))
    t, d = as_batch(kt, vt, wt), as_batch(kd, vd, wd)
    times = []
    n_out = 0
    for _ in range(reps):
        out = BatchStruct()
        ctx.sync()
        t0 = time.perf_counter()
        assert L.dbsp_join(ctx._h, ctypes.byref(d), ctypes.byref(t), 0, 0,
                           ctypes.byref(out)) == 0
        ctx.sync()
        times.append(time.perf_counter() - t0)
        n_out = out.len
        ctx.free_batch(out)
    dt = min(times)
    # probe model: ~2 effective cache lines per binary-search
    # probe chain per delta row + emitted rows
    algo_gb = (n_delta * 2 * 128 + n_out * 40.0) / 1e9
    return {
        "primitive": "dbsp_join (delta x 1B-row trace probe)",
        "trace_rows": n_trace, "delta_rows": n_delta, "rows_out": n_out,
        "ms": round(dt * 1e3, 2), "algo_GB": round(algo_gb, 2),
        "achieved_GBs": round(algo_gb / dt, 1),
        "frac_of_peak": round(algo_gb / dt / HBM_PEAK_GBS, 4),
    }


def bench_sort(ctx, L, n, reps=3):
    g = torch.Generator(device="cuda").manual_seed(9)
    k = torch.randint(0, 1 << 40, (n,), generator=g, dtype=torch.int64, device="cuda")
    v = torch.randint(0, 1 << 20, (n,), generator=g, dtype=torch.int64, device="cuda")
    w = torch.ones(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    b = as_batch(k, v, w)
    times = []
    n_out = 0
    for _ in range(reps):
        out = BatchStruct()
        ctx.sync()
        t0 = time.perf_counter()
        assert L.dbsp_sort_consolidate(ctx._h, b.k, b.v, b.w, n,
                                       ctypes.byref(out)) == 0
        ctx.sync()
        times.append(time.perf_counter() - t0)
        n_out = out.len
        ctx.free_batch(out)
    dt = min(times)
    # LSD radix: passes * (read+write 24B/row); 40+20 significant bits = 8 byte passes
    algo_gb = 8 * 48.0 * n / 1e9
    return {
        "primitive": "dbsp_sort_consolidate (radix, 60-bit keys)",
        "rows": n, "rows_out": n_out, "ms": round(dt * 1e3, 2),
        "algo_GB": round(algo_gb, 2), "achieved_GBs": round(algo_gb / dt, 1),
        "frac_of_peak": round(algo_gb / dt / HBM_PEAK_GBS, 4),
    }


def bench_incremental(ctx, L, n_trace, n_delta, steps=12):
    """C5-class incremental loop (SURVEY.md §8 config 5, i64-weight variant;
    the f64 sum aggregate is a named next step): per step, a 10M-row sorted
    delta joins against the 1B-row trace spine (join is linear: one probe per
    spine batch) and is then merged into the spine under the power-of-two
    leveling — the steady-state trace-maintenance loop at HBM scale."""
    kt, vt, wt = sorted_unique_batch(n_trace, 7)
    wt.fill_(1)  # trace weights +1 so delta inserts never fully cancel
    spine = [(as_batch(kt, vt, wt), None)]  # (batch, dbsp-owned BatchStruct?)
    keep_alive = [(kt, vt, wt)]
    gap = max(2, (9 * n_trace) // (2 * n_delta))
    step_ms = []
    joined_total = 0
    for it in range(steps):
        kd, vd, wd = sorted_unique_batch(n_delta, 100 + it, max_gap=gap)
        wd.fill_(1)
        keep_alive.append((kd, vd, wd))
        d = as_batch(kd, vd, wd)
        ctx.sync()
        t0 = time.perf_counter()
        # join delta against every spine batch (linear in the trace)
        outs = []
        for b, _ in spine:
            o = BatchStruct()
            assert L.dbsp_join(ctx._h, ctypes.byref(d), ctypes.byref(b), 0, 0,
                               ctypes.byref(o)) == 0
            outs.append(o)
        joined = sum(o.len for o in outs)
        for o in outs:
            ctx.free_batch(o)
        # insert the delta into the spine (power-of-two leveling)
        spine.append((d, None))
        while len(spine) >= 2 and spine[-1][0].len * 2 >= spine[-2][0].len:
            (b_top, own_top) = spine.pop()
            (b_below, own_below) = spine.pop()
            m = BatchStruct()
            assert L.dbsp_merge(ctx._h, ctypes.byref(b_below),
                                ctypes.byref(b_top), ctypes.byref(m)) == 0
            for bb, own in ((b_top, own_top), (b_below, own_below)):
                if own is not None:
                    ctx.free_batch(bb)
            spine.append((m, True))
        ctx.sync()
        step_ms.append((time.perf_counter() - t0) * 1e3)
        joined_total += joined
    trace_rows = sum(b.len for b, _ in spine)
    for b, own in spine:
        if own is not None:
            ctx.free_batch(b)
    avg = sum(step_ms[1:]) / max(1, len(step_ms) - 1)
    return {
        "primitive": "incremental join + spine maintenance (C5-class, i64)",
        "trace_rows_initial": n_trace, "delta_rows": n_delta, "steps": steps,
        "trace_rows_final": trace_rows, "join_matches_total": joined_total,
        "ms_per_step": [round(x, 2) for x in step_ms],
        "avg_ms_per_step": round(avg, 2),
        "delta_rows_per_s": round(n_delta / (avg / 1e3), 0),
    }


def bench_c5(ctx, L, n_trace, n_delta, steps=10):
    """Config C5 end-to-end: 1B-row indexed trace
    (1 val/key, f64 vals) x 10M-row delta incremental join, f64 vals weighed
    (f(k,v)=v) into f64 weights, consolidated deterministically, and
    sum-aggregated per key with upsert against the running output trace.
    i64 structural weights bit-exact; f64 sums within 2 ulp * depth."""
    g = torch.Generator(device="cuda").manual_seed(41)
    gaps = torch.randint(1, 8, (n_trace,), generator=g, dtype=torch.int64,
                         device="cuda")
    kt = torch.cumsum(gaps, 0)
    vt = torch.rand(n_trace, generator=g, dtype=torch.float64,
                    device="cuda").view(torch.int64)
    wt = torch.ones(n_trace, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    spine = [(as_batch(kt, vt, wt), None)]
    kmax = int(kt[-1].item())
    wb = None        # f64-weighted integral (auction-sum input trace)
    out_tr = None    # aggregate output trace (k -> f64 bits, i64 weights)
    step_ms = []
    gap = max(2, (9 * n_trace) // (2 * n_delta))
    for it in range(steps):
        gd = torch.Generator(device="cuda").manual_seed(500 + it)
        kd = torch.cumsum(torch.randint(1, gap, (n_delta,), generator=gd,
                                        dtype=torch.int64, device="cuda"), 0)
        vd = torch.zeros(n_delta, dtype=torch.int64, device="cuda")
        wd = torch.ones(n_delta, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        d = as_batch(kd, vd, wd)
        ctx.sync()
        t0 = time.perf_counter()
        # join vs every spine batch (proj (k, v2): carry the f64 val)
        outs = []
        for b, _ in spine:
            o = BatchStruct()
            assert L.dbsp_join(ctx._h, ctypes.byref(d), ctypes.byref(b), 8, 0,
                               ctypes.byref(o)) == 0
            outs.append(o)
        # weigh + consolidate each join output, fold into the f64 integral
        for o in outs:
            if o.len > 0:
                wre = BatchStruct()
                assert L.dbsp_weigh_f64(ctx._h, ctypes.byref(o),
                                        ctypes.byref(wre)) == 0
                dwb = BatchStruct()
                assert L.dbsp_sort_consolidate_f64(ctx._h, wre.k, wre.v, wre.w,
                                                   wre.len,
                                                   ctypes.byref(dwb)) == 0
                ctx.free_batch(wre)
                if wb is None:
                    wb = dwb
                else:
                    m = BatchStruct()
                    assert L.dbsp_merge_f64(ctx._h, ctypes.byref(wb),
                                            ctypes.byref(dwb),
                                            ctypes.byref(m)) == 0
                    ctx.free_batch(wb)
                    ctx.free_batch(dwb)
                    wb = m
            ctx.free_batch(o)
        # aggregate affected keys + upsert
        if wb is not None and wb.len > 0:
            keys = ctypes.c_void_p()
            nk = ctypes.c_int64()
            assert L.dbsp_unique_keys(ctx._h, ctypes.byref(wb),
                                      ctypes.byref(keys),
                                      ctypes.byref(nk)) == 0
            empty = BatchStruct()
            upd = BatchStruct()
            assert L.dbsp_agg_linear_upsert_f64(
                ctx._h, keys, nk.value, ctypes.byref(wb),
                ctypes.byref(out_tr if out_tr else empty),
                ctypes.byref(upd)) == 0
            L.dbsp_dev_free(ctx._h, keys)
            cons = BatchStruct()
            assert L.dbsp_sort_consolidate(ctx._h, upd.k, upd.v, upd.w,
                                           upd.len, ctypes.byref(cons)) == 0
            ctx.free_batch(upd)
            if out_tr is None:
                out_tr = cons
            else:
                m = BatchStruct()
                assert L.dbsp_merge(ctx._h, ctypes.byref(out_tr),
                                    ctypes.byref(cons), ctypes.byref(m)) == 0
                ctx.free_batch(out_tr)
                ctx.free_batch(cons)
                out_tr = m
        # insert the delta into the join trace spine
        spine.append((d, None))
        while len(spine) >= 2 and spine[-1][0].len * 2 >= spine[-2][0].len:
            (b_top, own_top) = spine.pop()
            (b_below, own_below) = spine.pop()
            m = BatchStruct()
            assert L.dbsp_merge(ctx._h, ctypes.byref(b_below),
                                ctypes.byref(b_top), ctypes.byref(m)) == 0
            for bb, own in ((b_top, own_top), (b_below, own_below)):
                if own is not None:
                    ctx.free_batch(bb)
            spine.append((m, True))
        ctx.sync()
        step_ms.append((time.perf_counter() - t0) * 1e3)
    res = {
        "primitive": "C5 end-to-end: 1B trace x 10M delta incremental join "
                     "+ f64 weigh/consolidate/sum-aggregate (i64 join, f64 agg)",
        "trace_rows": n_trace, "delta_rows": n_delta, "steps": steps,
        "agg_out_rows": out_tr.len if out_tr else 0,
        "wb_rows": wb.len if wb else 0,
        "ms_per_step": [round(x, 2) for x in step_ms],
        "avg_ms_per_step": round(sum(step_ms[1:]) / max(1, len(step_ms) - 1), 2),
    }
    for b, own in spine:
        if own is not None:
            ctx.free_batch(b)
    if wb is not None:
        ctx.free_batch(wb)
    if out_tr is not None:
        ctx.free_batch(out_tr)
    return res


def _rolling_deltas(n_per, parts, n_delta, late_frac, ticks, span, seed):
    """Per tick: n_delta raw rows (partition, ts, +1), ts near each
    partition's time frontier (2 * n_per, advancing `span` per tick), and a
    late_frac share drawn uniformly from the whole past."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    n_late = int(n_delta * late_frac)
    for t in range(ticks):
        k = torch.randint(0, parts, (n_delta,), generator=g,
                          dtype=torch.int64, device="cuda")
        v = 2 * n_per + t * span + torch.randint(
            0, span, (n_delta,), generator=g, dtype=torch.int64,
            device="cuda")
        if n_late:
            v[:n_late] = torch.randint(0, 2 * n_per, (n_late,), generator=g,
                                       dtype=torch.int64, device="cuda")
        w = torch.ones(n_delta, dtype=torch.int64, device="cuda")
        out.append((k, v, w))
    torch.cuda.synchronize()
    return out


def _with_values(ts, g, vmax=1 << 20):
    """(partition, ts) rows -> v = ts << 32 | val, val uniform below vmax."""
    val = torch.randint(0, vmax, ts.shape, generator=g, dtype=torch.int64,
                        device="cuda")
    return (ts << 32) | val


def bench_rolling(ctx, L, n_trace, parts, n_delta, late_frac, before, after,
                  ticks=12, warm=2, span=64, agg="sum"):
    """Incremental partitioned rolling aggregate (dbsp_rolling_step) against
    the only route the batch primitive offers: merge the tick's delta into
    ONE consolidated integral and run dbsp_rolling_agg over all of it (the
    diff against the previous result, which that route also needs, is NOT
    included: the comparison leg is a lower bound of its cost).  Both legs
    consume the same raw deltas; `warm` leading ticks are excluded.  Times
    are host-clock around calls that end in a stream synchronise; with
    DBSP_PROFILE=1 the operator body's hipEvent time (kernel_stats class 3)
    is reported too.

    agg "max" / "min": the same stream with a value column (rows
    (partition, ts << 32 | val, w), val uniform below 2^20) through a Max /
    Min operator, against merge + dbsp_rolling_minmax over the trace."""
    from dbsp_amd.engine import Engine, roll_agg_code
    n_per = max(1, n_trace // parts)
    n_trace = n_per * parts
    g = torch.Generator(device="cuda").manual_seed(17)
    tk = torch.arange(parts, dtype=torch.int64,
                      device="cuda").repeat_interleave(n_per)
    tv = (2 * torch.arange(n_per, dtype=torch.int64, device="cuda")).repeat(parts)
    tw = torch.randint(1, 4, (n_trace,), generator=g, dtype=torch.int64,
                       device="cuda")
    deltas = _rolling_deltas(n_per, parts, n_delta, late_frac, warm + ticks,
                             span, 23)
    if agg != "sum":
        gv = torch.Generator(device="cuda").manual_seed(29)
        tv = _with_values(tv, gv)
        deltas = [(k, _with_values(v, gv), w) for k, v, w in deltas]
        torch.cuda.synchronize()
    probe = Engine(ctx, query=101)   # reads the context's hipEvent counters

    # ---- incremental operator ----
    op = ctx.rolling_create(before, after, agg=agg)
    out = BatchStruct()
    t0 = time.perf_counter()
    assert L.dbsp_rolling_step(op._h, tk.data_ptr(), tv.data_ptr(),
                               tw.data_ptr(), n_trace, ctypes.byref(out)) == 0
    load_ms = (time.perf_counter() - t0) * 1e3
    ctx.free_batch(out)
    inc_ms, inc_ev_ms, rows_out = [], [], []
    for i, (k, v, w) in enumerate(deltas):
        ev0 = probe.kernel_stats(3)[0]
        out = BatchStruct()
        ctx.sync()
        t0 = time.perf_counter()
        assert L.dbsp_rolling_step(op._h, k.data_ptr(), v.data_ptr(),
                                   w.data_ptr(), n_delta,
                                   ctypes.byref(out)) == 0
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            inc_ms.append(dt)
            inc_ev_ms.append(probe.kernel_stats(3)[0] - ev0)
            rows_out.append(out.len)
        ctx.free_batch(out)
    stats = op.stats()
    op.close()

    # ---- comparison leg: consolidated integral + batch primitive ----
    integral = as_batch(tk, tv, tw)
    owned = False
    full_ms = []
    for i, (k, v, w) in enumerate(deltas):
        ctx.sync()
        t0 = time.perf_counter()
        d = BatchStruct()
        assert L.dbsp_sort_consolidate(ctx._h, k.data_ptr(), v.data_ptr(),
                                       w.data_ptr(), n_delta,
                                       ctypes.byref(d)) == 0
        m = BatchStruct()
        assert L.dbsp_merge(ctx._h, ctypes.byref(integral), ctypes.byref(d),
                            ctypes.byref(m)) == 0
        res = BatchStruct()
        if agg == "sum":
            assert after == 0, "dbsp_rolling_agg covers [ts - width, ts] only"
            assert L.dbsp_rolling_agg(ctx._h, ctypes.byref(m), before,
                                      ctypes.byref(res)) == 0
        else:
            assert L.dbsp_rolling_minmax(ctx._h, ctypes.byref(m),
                                         roll_agg_code(agg), before, after,
                                         ctypes.byref(res)) == 0
        ctx.sync()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            full_ms.append(dt)
        ctx.free_batch(d)
        ctx.free_batch(res)
        if owned:
            ctx.free_batch(integral)
        integral, owned = m, True
    if owned:
        ctx.free_batch(integral)
    probe.close()

    def med(x):
        s = sorted(x)
        return s[len(s) // 2]
    return {
        "primitive": "dbsp_rolling_step (incremental partitioned rolling "
                     "aggregate) vs merge + dbsp_rolling_agg over the trace"
                     if agg == "sum" else
                     f"dbsp_rolling_step on a {agg} operator vs merge + "
                     "dbsp_rolling_minmax over the trace",
        "agg": agg, "trace_rows": n_trace, "partitions": parts, "delta_rows": n_delta,
        "late_frac": late_frac, "before": before, "after": after,
        "ticks": ticks, "warmup_ticks": warm, "load_ms": round(load_ms, 2),
        "in_rows": stats[0], "in_batches": stats[1],
        "out_rows": stats[2], "out_batches": stats[3],
        "rows_out_per_tick": rows_out,
        "incremental_ms_per_step": [round(x, 3) for x in inc_ms],
        "incremental_ms_median": round(med(inc_ms), 3),
        "incremental_op_hipevent_ms": [round(x, 3) for x in inc_ev_ms],
        "full_recompute_ms_per_step": [round(x, 3) for x in full_ms],
        "full_recompute_ms_median": round(med(full_ms), 3),
        "full_recompute_excludes": "diff against the previous result",
    }


def _med(x):
    s = sorted(x)
    return s[len(s) // 2]


def bench_rolling_wm_operator(ctx, L, parts, n_delta, late_frac, before,
                              after, ticks, span, lateness, every):
    """Watermark-bounded operator (dbsp_rolling_step_wm) against the
    unbounded one (dbsp_rolling_step) of the same build on one frontier
    stream: tick t draws its times from [t*span, (t+1)*span) past a base of
    `lateness` and passes the watermark (t+1)*span - 1 (the largest time the
    tick can hold minus the lateness, so no readback); a late_frac share of
    its rows is drawn from between that watermark and the tick's frontier
    instead (late, but inside the lateness: no row is dropped).
    Host clock around calls that end in a stream synchronise."""
    assert lateness > span
    g = torch.Generator(device="cuda").manual_seed(29)
    n_late = int(n_delta * late_frac)
    deltas = []
    for t in range(ticks):
        k = torch.randint(0, parts, (n_delta,), generator=g,
                          dtype=torch.int64, device="cuda")
        v = lateness + t * span + torch.randint(
            0, span, (n_delta,), generator=g, dtype=torch.int64,
            device="cuda")
        wm = (t + 1) * span - 1
        if n_late:
            v[:n_late] = wm + torch.randint(
                0, lateness - span + 1, (n_late,), generator=g,
                dtype=torch.int64, device="cuda")
        w = torch.ones(n_delta, dtype=torch.int64, device="cuda")
        deltas.append((k, v, w, wm))
    torch.cuda.synchronize()
    legs = {}
    for name in ("bounded", "unbounded"):
        op = ctx.rolling_create(before, after)
        ms, rows, rows_out, peak = [], [], 0, [0, 0]
        for t, (k, v, w, wm) in enumerate(deltas):
            out = BatchStruct()
            ctx.sync()
            t0 = time.perf_counter()
            if name == "bounded":
                st = L.dbsp_rolling_step_wm(op._h, k.data_ptr(), v.data_ptr(),
                                            w.data_ptr(), n_delta, wm,
                                            ctypes.byref(out))
            else:
                st = L.dbsp_rolling_step(op._h, k.data_ptr(), v.data_ptr(),
                                         w.data_ptr(), n_delta,
                                         ctypes.byref(out))
            ms.append((time.perf_counter() - t0) * 1e3)
            assert st == 0
            rows_out += out.len
            ctx.free_batch(out)
            s = op.stats()
            peak = [max(peak[0], s[0]), max(peak[1], s[2])]
            if (t + 1) % every == 0:
                rows.append({"tick": t + 1, "in_rows": s[0], "out_rows": s[2]})
        q = max(1, ticks // 4)
        wm, lb, late, sweeps = op.wm_stats()
        legs[name] = {
            "rows_every_%d_ticks" % every: rows,
            "in_rows_max": peak[0], "out_rows_max": peak[1],
            "ms_median_first_quarter": round(_med(ms[:q]), 3),
            "ms_median_last_quarter": round(_med(ms[-q:]), 3),
            "ms_max": round(max(ms), 3),
            "rows_out_total": rows_out, "watermark": wm, "lower_bound": lb,
            "late_rows": late, "sweeps": sweeps,
        }
        op.close()
    assert legs["bounded"]["rows_out_total"] == \
        legs["unbounded"]["rows_out_total"]
    return {
        "primitive": "dbsp_rolling_step_wm (watermark-bounded state) vs "
                     "dbsp_rolling_step on one frontier stream",
        "partitions": parts, "delta_rows": n_delta, "late_frac": late_frac,
        "before": before, "after": after, "ticks": ticks, "span": span,
        "lateness": lateness, **legs,
    }


def bench_truncate(ctx, L, n, reps=5, run=64):
    """dbsp_truncate_below (mode 0) on n consolidated rows (p, ts, +-1) in
    partitions of `run` rows with the first half of every partition below the
    bound, against device-to-device hipMemcpyAsync calls over the same
    buffers whose sizes add up to 24n + 24*kept bytes (the three input
    columns and the three output columns, each copied into scratch).  A copy
    of B bytes reads B and writes B; the kernel's own model is 8n (count
    pass) + 24n (emit reads) + 24*kept (emit writes).  One untimed warm-up
    call each; host clock around calls that end in a synchronise."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_size_t, ctypes.c_int,
                                   ctypes.c_void_p]
    reps = int(os.environ.get("KB_REPS", reps))
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    k, v = i // run, i % run
    w = torch.where(i % 3 == 0, -1, 1).to(torch.int64)
    del i
    scratch = torch.empty(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    b = as_batch(k, v, w)
    times, kept, out = [], 0, None
    for r in range(reps + 1):
        if out is not None:
            ctx.free_batch(out)
        out = BatchStruct()
        ctx.sync()
        t0 = time.perf_counter()
        assert L.dbsp_truncate_below(ctx._h, ctypes.byref(b), 0, run // 2,
                                     ctypes.byref(out)) == 0
        dt = time.perf_counter() - t0
        if r:
            times.append(dt)
        kept = out.len
    pieces = [(k.data_ptr(), 8 * n), (v.data_ptr(), 8 * n),
              (w.data_ptr(), 8 * n), (out.k, 8 * kept), (out.v, 8 * kept),
              (out.w, 8 * kept)]
    ctimes = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for src, nbytes in pieces:
            assert hip.hipMemcpyAsync(scratch.data_ptr(), src, nbytes, 3,
                                      None) == 0       # 3 = device to device
        torch.cuda.synchronize()
        if r:
            ctimes.append(time.perf_counter() - t0)
    ctx.free_batch(out)
    algo = 8.0 * n + 24.0 * n + 24.0 * kept
    copy_bytes = 24.0 * n + 24.0 * kept
    return {
        "primitive": "dbsp_truncate_below (order-preserving spine "
                     "truncation) vs device-to-device hipMemcpyAsync",
        "rows": n, "kept": kept, "partition_rows": run,
        "rep_ms": [round(t * 1e3, 3) for t in times],
        "ms_min": round(min(times) * 1e3, 3),
        "ms_median": round(_med(times) * 1e3, 3),
        "algo_GB": round(algo / 1e9, 3),
        "achieved_GBs": round(algo / min(times) / 1e9, 1),
        "frac_of_peak": round(algo / min(times) / 1e9 / HBM_PEAK_GBS, 4),
        "copy_bytes": int(copy_bytes),
        "copy_rep_ms": [round(t * 1e3, 3) for t in ctimes],
        "copy_ms_min": round(min(ctimes) * 1e3, 3),
        "copy_ms_median": round(_med(ctimes) * 1e3, 3),
        "copy_moved_GBs": round(2 * copy_bytes / min(ctimes) / 1e9, 1),
    }


TOPK_SHIFT = 40


def _topk_stream(n_per, groups, n_delta, ticks, retract_frac, seed):
    """Per-tick raw deltas over a trace of `groups` groups x n_per rows at the
    even ranks (k = group << 40 | 2 * i, v = 0, w = +1).  Appends are distinct
    new rows at odd ranks (v = tick + 1 keeps them distinct across ticks).
    With retract_frac, that share of a tick takes back, for as many distinct
    groups, the group's highest trace row not yet taken back: a member of its
    current top-K unless appended rows have crowded it out."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n_ret = int(n_delta * retract_frac)
    assert n_ret <= groups
    taken = torch.zeros(groups, dtype=torch.int64, device="cuda")
    out = []
    for t in range(ticks):
        n_app = n_delta - n_ret
        pos = torch.randperm(n_per * groups, generator=g,
                             device="cuda")[:n_app]
        k = ((pos // n_per) << TOPK_SHIFT) | (2 * (pos % n_per) + 1)
        v = torch.full((n_app,), t + 1, dtype=torch.int64, device="cuda")
        w = torch.ones(n_app, dtype=torch.int64, device="cuda")
        if n_ret:
            gr = torch.randperm(groups, generator=g, device="cuda")[:n_ret]
            rk = (gr << TOPK_SHIFT) | (2 * (n_per - 1 - taken[gr]))
            taken[gr] += 1
            k = torch.cat([k, rk])
            v = torch.cat([v, torch.zeros(n_ret, dtype=torch.int64,
                                          device="cuda")])
            w = torch.cat([w, -torch.ones(n_ret, dtype=torch.int64,
                                          device="cuda")])
        out.append((k.contiguous(), v.contiguous(), w.contiguous()))
    torch.cuda.synchronize()
    return out


def bench_topk(ctx, L, n_trace, groups=1024, K=10, n_delta=40_000, ticks=12,
               warm=2, retract_frac=0.01):
    """Incremental top-K per group (dbsp_topk_step) on a trace of n_trace rows
    in `groups` groups: (a) an append-only stream, (b) the same stream with
    DBSP_TOPK_REFILL_ALL, (c) the recompute route: sort the delta, merge it
    into ONE consolidated integral and run dbsp_topk over all of it (the diff
    against the previous result, which that route also needs, is NOT
    included: a lower bound), (d) a second stream where retract_frac of each
    delta takes back a current top-K member.  Host clock around calls that end
    in a stream synchronise; `warm` leading ticks are excluded."""
    from dbsp_amd.engine import TopK
    n_per = max(K + ticks + warm + 1, n_trace // groups)
    n_trace = n_per * groups
    tk = ((torch.arange(groups, dtype=torch.int64, device="cuda")
           << TOPK_SHIFT).repeat_interleave(n_per)
          | (2 * torch.arange(n_per, dtype=torch.int64,
                              device="cuda")).repeat(groups))
    tv = torch.zeros(n_trace, dtype=torch.int64, device="cuda")
    tw = torch.ones(n_trace, dtype=torch.int64, device="cuda")
    appends = _topk_stream(n_per, groups, n_delta, warm + ticks, 0.0, 23)
    mixed = _topk_stream(n_per, groups, n_delta, warm + ticks, retract_frac, 29)

    def run_op(stream, refill_all):
        op = TopK(ctx, K, TOPK_SHIFT, refill_all=refill_all)
        out = BatchStruct()
        t0 = time.perf_counter()
        assert L.dbsp_topk_step(op._h, tk.data_ptr(), tv.data_ptr(),
                                tw.data_ptr(), n_trace, ctypes.byref(out)) == 0
        load_ms = (time.perf_counter() - t0) * 1e3
        assert out.len == K * groups
        ctx.free_batch(out)
        ms, rows_out, refilled, gathered = [], [], [], []
        prev = op.stats()
        for i, (k, v, w) in enumerate(stream):
            out = BatchStruct()
            ctx.sync()
            t0 = time.perf_counter()
            assert L.dbsp_topk_step(op._h, k.data_ptr(), v.data_ptr(),
                                    w.data_ptr(), len(k),
                                    ctypes.byref(out)) == 0
            dt = (time.perf_counter() - t0) * 1e3
            st = op.stats()
            if i >= warm:
                ms.append(dt)
                rows_out.append(out.len)
                refilled.append(st["groups_refilled"] - prev["groups_refilled"])
                gathered.append(st["rows_gathered"] - prev["rows_gathered"])
            prev = st
            ctx.free_batch(out)
        op.close()
        return {"load_ms": round(load_ms, 2),
                "ms_per_step": [round(x, 3) for x in ms],
                "ms_median": round(_med(ms), 3),
                "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                "rows_out_per_tick": rows_out,
                "groups_refilled_per_tick": refilled,
                "rows_gathered_per_tick": gathered,
                "in_rows": prev["in_rows"], "in_batches": prev["in_batches"],
                "out_rows": prev["out_rows"],
                "out_batches": prev["out_batches"]}

    a = run_op(appends, False)
    b = run_op(appends, True)
    d = run_op(mixed, False)

    # ---- (c) recompute: consolidated integral + batch primitive ----
    integral = as_batch(tk, tv, tw)
    owned = False
    full_ms = []
    for i, (k, v, w) in enumerate(appends):
        ctx.sync()
        t0 = time.perf_counter()
        dl = BatchStruct()
        assert L.dbsp_sort_consolidate(ctx._h, k.data_ptr(), v.data_ptr(),
                                       w.data_ptr(), len(k),
                                       ctypes.byref(dl)) == 0
        m = BatchStruct()
        assert L.dbsp_merge(ctx._h, ctypes.byref(integral), ctypes.byref(dl),
                            ctypes.byref(m)) == 0
        res = BatchStruct()
        assert L.dbsp_topk(ctx._h, ctypes.byref(m), K, TOPK_SHIFT,
                           ctypes.byref(res)) == 0
        ctx.sync()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            full_ms.append(dt)
        ctx.free_batch(dl)
        ctx.free_batch(res)
        if owned:
            ctx.free_batch(integral)
        integral, owned = m, True
    if owned:
        ctx.free_batch(integral)
    return {
        "primitive": "dbsp_topk_step (incremental top-K per group) vs "
                     "refill_all vs merge + dbsp_topk over the trace",
        "trace_rows": n_trace, "groups": groups, "k": K,
        "delta_rows": n_delta, "ticks": ticks, "warmup_ticks": warm,
        "retract_frac": retract_frac,
        "a_append_only": a, "b_append_only_refill_all": b,
        "c_recompute_ms_per_step": [round(x, 3) for x in full_ms],
        "c_recompute_ms_median": round(_med(full_ms), 3),
        "c_recompute_ms_min": round(min(full_ms), 3),
        "c_recompute_ms_max": round(max(full_ms), 3),
        "c_recompute_excludes": "diff against the previous result",
        "d_with_retractions": d,
    }


def bench_argmax(ctx, L, n_trace, groups=1024, n_delta=40_000, ticks=12,
                 warm=2):
    """Incremental arg-max per group (dbsp_argmax_step, group_shift 40,
    rank_shift 0) on a trace of n_trace rows in `groups` groups: (a) an
    append-only stream, on which no group's maximum ever decreases, (b) the
    same stream with DBSP_ARGMAX_REFILL_ALL, (c) the recompute route: sort the
    delta, merge it into ONE consolidated integral and run dbsp_argmax over
    all of it (the diff against the previous result, which that route also
    needs, is NOT included: a lower bound), (d) the append-only stream kept
    out of group 0, which instead loses its top row every tick: one refill of
    a group of n_trace / groups rows per tick.  Host clock around calls that
    end in a stream synchronise; `warm` leading ticks are excluded."""
    from dbsp_amd.engine import ArgMax
    n_per = max(ticks + warm + 2, n_trace // groups)
    n_trace = n_per * groups
    tk = ((torch.arange(groups, dtype=torch.int64, device="cuda")
           << TOPK_SHIFT).repeat_interleave(n_per)
          | (2 * torch.arange(n_per, dtype=torch.int64,
                              device="cuda")).repeat(groups))
    tv = torch.zeros(n_trace, dtype=torch.int64, device="cuda")
    tw = torch.ones(n_trace, dtype=torch.int64, device="cuda")
    appends = _topk_stream(n_per, groups, n_delta, warm + ticks, 0.0, 23)
    hot = []
    for t, (k, v, w) in enumerate(appends):
        keep = (k >> TOPK_SHIFT) != 0
        top = torch.tensor([2 * (n_per - 1 - t)], dtype=torch.int64,
                           device="cuda")
        hot.append((torch.cat([k[keep], top]).contiguous(),
                    torch.cat([v[keep], torch.zeros_like(top)]).contiguous(),
                    torch.cat([w[keep], -torch.ones_like(top)]).contiguous()))
    torch.cuda.synchronize()

    def run_op(stream, refill_all):
        op = ArgMax(ctx, TOPK_SHIFT, 0, refill_all=refill_all)
        out = BatchStruct()
        t0 = time.perf_counter()
        assert L.dbsp_argmax_step(op._h, tk.data_ptr(), tv.data_ptr(),
                                  tw.data_ptr(), n_trace,
                                  ctypes.byref(out)) == 0
        load_ms = (time.perf_counter() - t0) * 1e3
        assert out.len == groups
        ctx.free_batch(out)
        ms, rows_out, refilled, gathered = [], [], [], []
        prev = op.stats()
        for i, (k, v, w) in enumerate(stream):
            out = BatchStruct()
            ctx.sync()
            t0 = time.perf_counter()
            assert L.dbsp_argmax_step(op._h, k.data_ptr(), v.data_ptr(),
                                      w.data_ptr(), len(k),
                                      ctypes.byref(out)) == 0
            dt = (time.perf_counter() - t0) * 1e3
            st = op.stats()
            if i >= warm:
                ms.append(dt)
                rows_out.append(out.len)
                refilled.append(st["groups_refilled"] - prev["groups_refilled"])
                gathered.append(st["rows_gathered"] - prev["rows_gathered"])
            prev = st
            ctx.free_batch(out)
        op.close()
        return {"load_ms": round(load_ms, 2),
                "ms_per_step": [round(x, 3) for x in ms],
                "ms_median": round(_med(ms), 3),
                "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                "rows_out_per_tick": rows_out,
                "groups_refilled_per_tick": refilled,
                "rows_gathered_per_tick": gathered,
                "in_rows": prev["in_rows"], "in_batches": prev["in_batches"],
                "out_rows": prev["out_rows"],
                "out_batches": prev["out_batches"]}

    a = run_op(appends, False)
    assert sum(a["groups_refilled_per_tick"]) == 0
    assert sum(a["rows_gathered_per_tick"]) == 0
    b = run_op(appends, True)
    d = run_op(hot, False)
    assert d["groups_refilled_per_tick"] == [1] * ticks

    # ---- (c) recompute: consolidated integral + batch primitive ----
    integral = as_batch(tk, tv, tw)
    owned = False
    full_ms = []
    for i, (k, v, w) in enumerate(appends):
        ctx.sync()
        t0 = time.perf_counter()
        dl = BatchStruct()
        assert L.dbsp_sort_consolidate(ctx._h, k.data_ptr(), v.data_ptr(),
                                       w.data_ptr(), len(k),
                                       ctypes.byref(dl)) == 0
        m = BatchStruct()
        assert L.dbsp_merge(ctx._h, ctypes.byref(integral), ctypes.byref(dl),
                            ctypes.byref(m)) == 0
        res = BatchStruct()
        assert L.dbsp_argmax(ctx._h, ctypes.byref(m), TOPK_SHIFT, 0,
                             ctypes.byref(res)) == 0
        ctx.sync()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            full_ms.append(dt)
        ctx.free_batch(dl)
        ctx.free_batch(res)
        if owned:
            ctx.free_batch(integral)
        integral, owned = m, True
    if owned:
        ctx.free_batch(integral)
    return {
        "primitive": "dbsp_argmax_step (incremental arg-max per group, ties "
                     "kept) vs refill_all vs merge + dbsp_argmax over the "
                     "trace",
        "trace_rows": n_trace, "groups": groups, "group_rows": n_per,
        "delta_rows": n_delta, "ticks": ticks, "warmup_ticks": warm,
        "a_append_only": a, "b_append_only_refill_all": b,
        "c_recompute_ms_per_step": [round(x, 3) for x in full_ms],
        "c_recompute_ms_median": round(_med(full_ms), 3),
        "c_recompute_ms_min": round(min(full_ms), 3),
        "c_recompute_ms_max": round(max(full_ms), 3),
        "c_recompute_excludes": "diff against the previous result",
        "d_hot_group_refilled_every_tick": d,
    }


def bench_antijoin(ctx, L, n_trace, per_key=64, n_delta=40_000, n_flip=256,
                   ticks=12, warm=2):
    """Incremental antijoin (dbsp_antijoin_step) over a row trace of n_trace
    rows, per_key values per key (k = key index, v = 0..per_key-1, w = +1),
    with the even keys present in the key trace.  Every tick sends n_delta new
    rows over uniform keys plus n_flip distinct keys whose presence flips
    (-1 if present, +1 if absent), so about n_flip * per_key trace rows are
    re-emitted.  Beside it the recompute route: sort both deltas, merge them
    into ONE consolidated integral each and run dbsp_antijoin over all of it
    (the diff against the previous result, which that route also needs, is
    NOT included: a lower bound).  Host clock around calls that end in a
    stream synchronise; `warm` leading ticks are excluded."""
    from dbsp_amd.engine import AntiJoin, ANTIJOIN
    nkeys = max(2 * n_flip, n_trace // per_key)
    n_trace = nkeys * per_key
    i64 = dict(dtype=torch.int64, device="cuda")
    tk = torch.arange(nkeys, **i64).repeat_interleave(per_key)
    tv = torch.arange(per_key, **i64).repeat(nkeys)
    tw = torch.ones(n_trace, **i64)
    bk = torch.arange(0, nkeys, 2, **i64)
    bw = torch.ones(len(bk), **i64)
    g = torch.Generator(device="cuda").manual_seed(31)
    present = torch.zeros(nkeys, dtype=torch.bool, device="cuda")
    present[bk] = True
    stream = []
    for t in range(warm + ticks):
        ak = torch.randint(0, nkeys, (n_delta,), generator=g, **i64)
        av = per_key + t * n_delta + torch.arange(n_delta, **i64)
        aw = torch.ones(n_delta, **i64)
        fk = torch.randperm(nkeys, generator=g, device="cuda")[:n_flip]
        fw = torch.where(present[fk], -1, 1).to(torch.int64)
        present[fk] = ~present[fk]
        stream.append((ak, av, aw, fk.contiguous(), fw.contiguous()))
    torch.cuda.synchronize()

    op = AntiJoin(ctx, ANTIJOIN)
    out = BatchStruct()
    t0 = time.perf_counter()
    assert L.dbsp_antijoin_step(op._h, tk.data_ptr(), tv.data_ptr(),
                                tw.data_ptr(), n_trace, bk.data_ptr(),
                                bw.data_ptr(), len(bk),
                                ctypes.byref(out)) == 0
    load_ms = (time.perf_counter() - t0) * 1e3
    assert out.len == (nkeys - len(bk)) * per_key
    ctx.free_batch(out)
    ms, rows_out, flipped, gathered, filtered = [], [], [], [], []
    prev = op.stats()
    for i, (ak, av, aw, fk, fw) in enumerate(stream):
        out = BatchStruct()
        ctx.sync()
        t0 = time.perf_counter()
        assert L.dbsp_antijoin_step(op._h, ak.data_ptr(), av.data_ptr(),
                                    aw.data_ptr(), len(ak), fk.data_ptr(),
                                    fw.data_ptr(), len(fk),
                                    ctypes.byref(out)) == 0
        dt = (time.perf_counter() - t0) * 1e3
        st = op.stats()
        if i >= warm:
            ms.append(dt)
            rows_out.append(out.len)
            flipped.append(st["keys_flipped"] - prev["keys_flipped"])
            gathered.append(st["rows_gathered"] - prev["rows_gathered"])
            filtered.append(st["rows_filtered"] - prev["rows_filtered"])
        prev = st
        ctx.free_batch(out)
    op.close()
    inc = {"load_ms": round(load_ms, 2),
           "ms_per_step": [round(x, 3) for x in ms],
           "ms_median": round(_med(ms), 3),
           "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
           "rows_out_per_tick": rows_out, "keys_flipped_per_tick": flipped,
           "rows_gathered_per_tick": gathered,
           "rows_filtered_per_tick": filtered,
           "a_rows": prev["a_rows"], "a_batches": prev["a_batches"],
           "b_rows": prev["b_rows"], "b_batches": prev["b_batches"]}

    # ---- recompute: consolidated integrals + the batch primitive ----
    ia, ib = as_batch(tk, tv, tw), as_batch(bk, torch.zeros_like(bk), bw)
    owned = False
    full_ms = []
    for i, (ak, av, aw, fk, fw) in enumerate(stream):
        fz = torch.zeros_like(fk)
        ctx.sync()
        t0 = time.perf_counter()
        da, db, ma, mb, res = (BatchStruct() for _ in range(5))
        assert L.dbsp_sort_consolidate(ctx._h, ak.data_ptr(), av.data_ptr(),
                                       aw.data_ptr(), len(ak),
                                       ctypes.byref(da)) == 0
        assert L.dbsp_sort_consolidate(ctx._h, fk.data_ptr(), fz.data_ptr(),
                                       fw.data_ptr(), len(fk),
                                       ctypes.byref(db)) == 0
        assert L.dbsp_merge(ctx._h, ctypes.byref(ia), ctypes.byref(da),
                            ctypes.byref(ma)) == 0
        assert L.dbsp_merge(ctx._h, ctypes.byref(ib), ctypes.byref(db),
                            ctypes.byref(mb)) == 0
        assert L.dbsp_antijoin(ctx._h, ctypes.byref(ma), mb.k, mb.w, mb.len,
                               ANTIJOIN, ctypes.byref(res)) == 0
        ctx.sync()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            full_ms.append(dt)
        for b in (da, db, res):
            ctx.free_batch(b)
        if owned:
            ctx.free_batch(ia)
            ctx.free_batch(ib)
        ia, ib, owned = ma, mb, True
    if owned:
        ctx.free_batch(ia)
        ctx.free_batch(ib)
    return {
        "primitive": "dbsp_antijoin_step (incremental antijoin) vs merge + "
                     "dbsp_antijoin over the traces",
        "trace_rows": n_trace, "keys": nkeys, "values_per_key": per_key,
        "delta_rows": n_delta, "keys_flipped": n_flip, "ticks": ticks,
        "warmup_ticks": warm,
        "incremental": inc,
        "recompute_ms_per_step": [round(x, 3) for x in full_ms],
        "recompute_ms_median": round(_med(full_ms), 3),
        "recompute_ms_min": round(min(full_ms), 3),
        "recompute_ms_max": round(max(full_ms), 3),
        "recompute_excludes": "diff against the previous result",
    }


def bench_rolling_wm(ctx, L, args):
    yield bench_rolling_wm_operator(ctx, L, args.roll_parts, args.roll_delta,
                                    args.roll_late, args.roll_before,
                                    args.roll_after, args.wm_ticks, 64,
                                    args.wm_lateness, args.wm_every)
    for n in args.trunc_rows:
        yield bench_truncate(ctx, L, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000_000,
                    help="rows per merge side (trace = 2x this)")
    ap.add_argument("--delta", type=int, default=10_000_000)
    ap.add_argument("--sort-rows", type=int, default=50_000_000)
    ap.add_argument("--only", default=None,
                    choices=["merge", "join", "sort", "incremental", "c5",
                             "rolling", "rolling_wm", "rolling_minmax",
                             "topk", "antijoin", "argmax"])
    ap.add_argument("--argmax-rows", type=int, nargs="*",
                    default=[4_000_000, 16_000_000, 64_000_000],
                    help="argmax leg: trace rows")
    ap.add_argument("--anti-rows", type=int, nargs="*",
                    default=[4_000_000, 16_000_000, 64_000_000],
                    help="antijoin leg: row-trace rows")
    ap.add_argument("--topk-rows", type=int, nargs="*",
                    default=[4_000_000, 16_000_000, 64_000_000],
                    help="topk leg: trace rows")
    ap.add_argument("--wm-ticks", type=int, default=200,
                    help="rolling_wm leg: ticks of the frontier stream")
    ap.add_argument("--wm-lateness", type=int, default=1024)
    ap.add_argument("--wm-every", type=int, default=25,
                    help="rolling_wm leg: record trace rows every N ticks")
    ap.add_argument("--trunc-rows", type=int, nargs="*",
                    default=[4_000_000, 16_000_000, 64_000_000],
                    help="rolling_wm leg: dbsp_truncate_below sizes")
    ap.add_argument("--roll-rows", type=int, default=4_000_000,
                    help="rolling leg: trace rows")
    ap.add_argument("--roll-parts", type=int, default=1024)
    ap.add_argument("--roll-delta", type=int, default=40_000)
    ap.add_argument("--roll-late", type=float, default=0.01)
    ap.add_argument("--roll-before", type=int, default=200)
    ap.add_argument("--roll-after", type=int, default=0)
    ap.add_argument("--roll-ticks", type=int, default=12)
    args = ap.parse_args()
    ctx = Ctx(0)
    L = _L()
    legs = {
        "merge": lambda: bench_merge(ctx, L, args.rows),
        "join": lambda: bench_join(ctx, L, 2 * args.rows, args.delta),
        "sort": lambda: bench_sort(ctx, L, args.sort_rows),
        "incremental": lambda: bench_incremental(ctx, L, 2 * args.rows,
                                                 args.delta),
        "c5": lambda: bench_c5(ctx, L, 2 * args.rows, args.delta),
        "rolling": lambda: bench_rolling(ctx, L, args.roll_rows,
                                         args.roll_parts, args.roll_delta,
                                         args.roll_late, args.roll_before,
                                         args.roll_after, args.roll_ticks),
    }
    for name, leg in legs.items():
        # the rolling leg runs on request only: a bare run keeps its legs
        if args.only == name or (args.only is None and name != "rolling"):
            print(json.dumps(leg()))
    if args.only == "rolling_minmax":   # on request only: the rolling leg's
        for agg in ("sum", "max"):      # stream through both operators
            print(json.dumps(bench_rolling(
                ctx, L, args.roll_rows, args.roll_parts, args.roll_delta,
                args.roll_late, args.roll_before, args.roll_after,
                args.roll_ticks, agg=agg)), flush=True)
    if args.only == "topk":             # on request only, as the rolling leg
        for n in args.topk_rows:
            print(json.dumps(bench_topk(ctx, L, n)), flush=True)
    if args.only == "antijoin":         # on request only, as the rolling leg
        for n in args.anti_rows:
            print(json.dumps(bench_antijoin(ctx, L, n)), flush=True)
    if args.only == "argmax":           # on request only, as the rolling leg
        for n in args.argmax_rows:
            print(json.dumps(bench_argmax(ctx, L, n)), flush=True)
    if args.only == "rolling_wm":       # on request only, as the rolling leg
        for res in bench_rolling_wm(ctx, L, args):
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
