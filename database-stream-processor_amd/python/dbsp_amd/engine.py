"""GPU engine bindings (the PRODUCT path).

ctypes layer over libdbsp_hip.so — the C-ABI of include/dbsp_hip.h.  Requires
a real GPU: dbsp_ctx_create fails with DBSP_ERR_NOGPU otherwise (no CPU
fallback, by design).  torch is used only as plumbing for tests that need
device arrays; the engine itself manages its own HBM.
"""
import ctypes

import numpy as np

from . import (EVENT_DT, ROLL_MAX, ROLL_MIN, ROLL_SUM, ROW_DT,
               load_hip_lib)

_lib = None


class BatchStruct(ctypes.Structure):
    _fields_ = [("k", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("w", ctypes.c_void_p), ("len", ctypes.c_int64)]


class JoinPlanStruct(ctypes.Structure):
    _fields_ = [("delta", BatchStruct), ("nd", ctypes.c_int64),
                ("trace_batches", ctypes.POINTER(BatchStruct)),
                ("n_batches", ctypes.c_int), ("proj", ctypes.c_int),
                ("fresh", ctypes.c_int), ("tn", ctypes.c_int64)]


class WindowChainStruct(ctypes.Structure):
    _fields_ = [("state", ctypes.c_uint64 * 4), ("wm_n", ctypes.c_int64),
                ("bn", ctypes.c_int64), ("width", ctypes.c_uint64),
                ("tumble", ctypes.c_uint64), ("lag", ctypes.c_uint64)]


WM_SOURCES = {"host_n": 0, "dev_n": 1, "gmax": 2}  # dbsp_wm_source


def _L():
    global _lib
    if _lib is None:
        _lib = load_hip_lib()
        L = _lib
        i64, u64, vp, i32 = (ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p,
                             ctypes.c_int32)
        L.dbsp_ctx_create.restype = i32
        L.dbsp_ctx_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
        L.dbsp_ctx_destroy.argtypes = [vp]
        L.dbsp_ctx_sync.restype = i32
        L.dbsp_ctx_sync.argtypes = [vp]
        L.dbsp_dev_alloc.restype = i32
        L.dbsp_dev_alloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.dbsp_dev_free.restype = i32
        L.dbsp_dev_free.argtypes = [vp, vp]
        L.dbsp_h2d.restype = i32
        L.dbsp_h2d.argtypes = [vp, vp, vp, ctypes.c_size_t]
        L.dbsp_d2h.restype = i32
        L.dbsp_d2h.argtypes = [vp, vp, vp, ctypes.c_size_t]
        L.dbsp_sort_consolidate.restype = i32
        L.dbsp_sort_consolidate.argtypes = [vp, vp, vp, vp, i64,
                                            ctypes.POINTER(BatchStruct)]
        L.dbsp_merge.restype = i32
        L.dbsp_merge.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                 ctypes.POINTER(BatchStruct),
                                 ctypes.POINTER(BatchStruct)]
        L.dbsp_join.restype = i32
        L.dbsp_join.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                ctypes.POINTER(BatchStruct), ctypes.c_int, u64,
                                ctypes.POINTER(BatchStruct)]
        L.dbsp_join_spine.restype = i32
        L.dbsp_join_spine.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                      ctypes.POINTER(BatchStruct),
                                      ctypes.c_int, ctypes.c_int, u64,
                                      ctypes.c_int,
                                      ctypes.POINTER(BatchStruct)]
        L.dbsp_join_tail.restype = i32
        L.dbsp_join_tail.argtypes = [vp, ctypes.POINTER(JoinPlanStruct),
                                     ctypes.c_int, i64, ctypes.POINTER(i64),
                                     ctypes.POINTER(vp),
                                     ctypes.POINTER(BatchStruct)]
        L.dbsp_agg_linear_upsert.restype = i32
        L.dbsp_agg_linear_upsert.argtypes = [vp, vp, i64,
                                             ctypes.POINTER(BatchStruct),
                                             ctypes.POINTER(BatchStruct),
                                             ctypes.POINTER(BatchStruct)]
        L.dbsp_agg_max_upsert.restype = i32
        L.dbsp_agg_max_upsert.argtypes = L.dbsp_agg_linear_upsert.argtypes
        L.dbsp_agg_last10_upsert.restype = i32
        L.dbsp_agg_last10_upsert.argtypes = L.dbsp_agg_linear_upsert.argtypes
        L.dbsp_agg_sum_spine.restype = i32
        L.dbsp_agg_sum_spine.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                         ctypes.POINTER(BatchStruct),
                                         ctypes.c_int, ctypes.POINTER(vp),
                                         ctypes.POINTER(i64),
                                         ctypes.POINTER(BatchStruct)]
        L.dbsp_wm_update.restype = i32
        L.dbsp_wm_update.argtypes = [vp, ctypes.POINTER(u64),
                                     ctypes.POINTER(u64), ctypes.c_int, vp,
                                     i64, i64, u64, u64, u64, u64]
        L.dbsp_window_spine.restype = i32
        L.dbsp_window_spine.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                        ctypes.c_int,
                                        ctypes.POINTER(BatchStruct),
                                        ctypes.c_int, ctypes.POINTER(u64),
                                        ctypes.POINTER(WindowChainStruct),
                                        ctypes.POINTER(i64),
                                        ctypes.POINTER(i64),
                                        ctypes.POINTER(BatchStruct)]
        L.dbsp_window.restype = i32
        L.dbsp_window.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                  ctypes.POINTER(BatchStruct), ctypes.c_int,
                                  u64, u64, u64, u64,
                                  ctypes.POINTER(BatchStruct)]
        L.dbsp_shard_partition.restype = i32
        L.dbsp_shard_partition.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                           ctypes.c_int,
                                           ctypes.POINTER(BatchStruct), vp]
        L.dbsp_xxh3_u64.restype = u64
        L.dbsp_xxh3_u64.argtypes = [u64, u64]
        L.dbsp_acc_fold.restype = i32
        L.dbsp_acc_fold.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                    ctypes.POINTER(BatchStruct),
                                    ctypes.POINTER(BatchStruct)]
        L.dbsp_sort_consolidate_f64.restype = i32
        L.dbsp_sort_consolidate_f64.argtypes = [vp, vp, vp, vp, i64,
                                                ctypes.POINTER(BatchStruct)]
        L.dbsp_merge_f64.restype = i32
        L.dbsp_merge_f64.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                     ctypes.POINTER(BatchStruct),
                                     ctypes.POINTER(BatchStruct)]
        L.dbsp_weigh_f64.restype = i32
        L.dbsp_weigh_f64.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                     ctypes.POINTER(BatchStruct)]
        L.dbsp_agg_linear_upsert_f64.restype = i32
        L.dbsp_agg_linear_upsert_f64.argtypes = [vp, vp, i64,
                                                 ctypes.POINTER(BatchStruct),
                                                 ctypes.POINTER(BatchStruct),
                                                 ctypes.POINTER(BatchStruct)]
        L.dbsp_distinct_inc.restype = i32
        L.dbsp_distinct_inc.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                        ctypes.POINTER(BatchStruct),
                                        ctypes.c_int,
                                        ctypes.POINTER(BatchStruct)]
        L.dbsp_unique_keys.restype = i32
        L.dbsp_unique_keys.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                       ctypes.POINTER(vp),
                                       ctypes.POINTER(i64)]
        L.dbsp_comm_unique_id.restype = i32
        L.dbsp_comm_unique_id.argtypes = [vp]
        L.dbsp_comm_init.restype = i32
        L.dbsp_comm_init.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
        L.dbsp_engine_create.restype = i32
        L.dbsp_engine_create.argtypes = [ctypes.POINTER(vp), vp, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int]
        L.dbsp_engine_destroy.argtypes = [vp]
        L.dbsp_engine_step.restype = i32
        L.dbsp_engine_step.argtypes = [vp, vp, i64]
        L.dbsp_engine_stage_events.restype = i32
        L.dbsp_engine_stage_events.argtypes = [vp, vp, i64]
        L.dbsp_engine_step_staged.restype = i32
        L.dbsp_engine_step_staged.argtypes = [vp, i64, i64]
        L.dbsp_engine_run_staged.restype = i32
        L.dbsp_engine_run_staged.argtypes = [vp, i64, i64, i64]
        L.dbsp_engine_output.restype = i32
        L.dbsp_engine_output.argtypes = [vp, vp, i64, ctypes.POINTER(i64)]
        L.dbsp_engine_output_events.restype = i32
        L.dbsp_engine_output_events.argtypes = [vp, vp, i64, ctypes.POINTER(i64)]
        L.dbsp_rolling_agg.restype = i32
        L.dbsp_rolling_agg.argtypes = [vp, ctypes.POINTER(BatchStruct), u64,
                                       ctypes.POINTER(BatchStruct)]
        L.dbsp_rolling_create.restype = i32
        L.dbsp_rolling_create.argtypes = [vp, u64, u64, ctypes.POINTER(vp)]
        L.dbsp_rolling_create_agg.restype = i32
        L.dbsp_rolling_create_agg.argtypes = [vp, i32, u64, u64,
                                              ctypes.POINTER(vp)]
        L.dbsp_rolling_minmax.restype = i32
        L.dbsp_rolling_minmax.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                          i32, u64, u64,
                                          ctypes.POINTER(BatchStruct)]
        L.dbsp_engine_rolling_agg.restype = i32
        L.dbsp_engine_rolling_agg.argtypes = [vp, i32]
        L.dbsp_rolling_step.restype = i32
        L.dbsp_rolling_step.argtypes = [vp, vp, vp, vp, i64,
                                        ctypes.POINTER(BatchStruct)]
        L.dbsp_rolling_stats.restype = i32
        L.dbsp_rolling_stats.argtypes = [vp, ctypes.POINTER(i64),
                                         ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(i64),
                                         ctypes.POINTER(ctypes.c_int)]
        L.dbsp_rolling_destroy.restype = i32
        L.dbsp_rolling_destroy.argtypes = [vp]
        L.dbsp_rolling_step_wm.restype = i32
        L.dbsp_rolling_step_wm.argtypes = [vp, vp, vp, vp, i64, u64,
                                           ctypes.POINTER(BatchStruct)]
        L.dbsp_rolling_compact.restype = i32
        L.dbsp_rolling_compact.argtypes = [vp]
        L.dbsp_rolling_wm_stats.restype = i32
        L.dbsp_rolling_wm_stats.argtypes = [vp, ctypes.POINTER(u64),
                                            ctypes.POINTER(u64),
                                            ctypes.POINTER(i64),
                                            ctypes.POINTER(i64)]
        L.dbsp_truncate_below.restype = i32
        L.dbsp_truncate_below.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                          ctypes.c_int, u64,
                                          ctypes.POINTER(BatchStruct)]
        L.dbsp_engine_rolling_init.restype = i32
        L.dbsp_engine_rolling_init.argtypes = [vp, u64, u64]
        L.dbsp_engine_rolling_lateness.restype = i32
        L.dbsp_engine_rolling_lateness.argtypes = [vp, u64]
        L.dbsp_engine_rolling_stats.restype = i32
        L.dbsp_engine_rolling_stats.argtypes = [vp, ctypes.POINTER(i64),
                                                ctypes.POINTER(i64),
                                                ctypes.POINTER(i64),
                                                ctypes.POINTER(i64)]
        L.dbsp_topk.restype = i32
        L.dbsp_topk.argtypes = [vp, ctypes.POINTER(BatchStruct), i64,
                                ctypes.c_int, ctypes.POINTER(BatchStruct)]
        L.dbsp_topk_create.restype = i32
        L.dbsp_topk_create.argtypes = [vp, i64, ctypes.c_int, ctypes.c_uint32,
                                       ctypes.POINTER(vp)]
        L.dbsp_topk_step.restype = i32
        L.dbsp_topk_step.argtypes = [vp, vp, vp, vp, i64,
                                     ctypes.POINTER(BatchStruct)]
        L.dbsp_topk_stats.restype = i32
        L.dbsp_topk_stats.argtypes = [vp, ctypes.POINTER(i64),
                                      ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(i64),
                                      ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(i64),
                                      ctypes.POINTER(i64),
                                      ctypes.POINTER(i64)]
        L.dbsp_topk_destroy.restype = i32
        L.dbsp_topk_destroy.argtypes = [vp]
        L.dbsp_engine_topk_init.restype = i32
        L.dbsp_engine_topk_init.argtypes = [vp, i64]
        L.dbsp_engine_topk_stats.restype = i32
        L.dbsp_engine_topk_stats.argtypes = [vp] + [ctypes.POINTER(i64)] * 5
        L.dbsp_antijoin.restype = i32
        L.dbsp_antijoin.argtypes = [vp, ctypes.POINTER(BatchStruct), vp, vp,
                                    i64, ctypes.c_int,
                                    ctypes.POINTER(BatchStruct)]
        L.dbsp_antijoin_create.restype = i32
        L.dbsp_antijoin_create.argtypes = [vp, ctypes.c_int,
                                           ctypes.POINTER(vp)]
        L.dbsp_antijoin_step.restype = i32
        L.dbsp_antijoin_step.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64,
                                         ctypes.POINTER(BatchStruct)]
        L.dbsp_antijoin_stats.restype = i32
        L.dbsp_antijoin_stats.argtypes = [vp, ctypes.POINTER(i64),
                                          ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(i64),
                                          ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(i64),
                                          ctypes.POINTER(i64),
                                          ctypes.POINTER(i64)]
        L.dbsp_antijoin_destroy.restype = i32
        L.dbsp_antijoin_destroy.argtypes = [vp]
        L.dbsp_engine_antijoin_stats.restype = i32
        L.dbsp_engine_antijoin_stats.argtypes = (
            [vp] + [ctypes.POINTER(i64)] * 5)
        L.dbsp_argmax.restype = i32
        L.dbsp_argmax.argtypes = [vp, ctypes.POINTER(BatchStruct),
                                  ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(BatchStruct)]
        L.dbsp_argmax_create.restype = i32
        L.dbsp_argmax_create.argtypes = [vp, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_uint32, ctypes.POINTER(vp)]
        L.dbsp_argmax_step.restype = i32
        L.dbsp_argmax_step.argtypes = [vp, vp, vp, vp, i64,
                                       ctypes.POINTER(BatchStruct)]
        L.dbsp_argmax_stats.restype = i32
        L.dbsp_argmax_stats.argtypes = [vp, ctypes.POINTER(i64),
                                        ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(i64),
                                        ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(i64),
                                        ctypes.POINTER(i64),
                                        ctypes.POINTER(i64)]
        L.dbsp_argmax_destroy.restype = i32
        L.dbsp_argmax_destroy.argtypes = [vp]
        L.dbsp_engine_argmax_stats.restype = i32
        L.dbsp_engine_argmax_stats.argtypes = [vp] + [ctypes.POINTER(i64)] * 5
        L.dbsp_engine_c5_init.restype = i32
        L.dbsp_engine_c5_init.argtypes = [vp, i64, i64, u64]
        L.dbsp_engine_kernel_stats.restype = i32
        L.dbsp_engine_kernel_stats.argtypes = [vp, ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(i64)]
    return _lib


def _check(status, what):
    if status != 0:
        raise RuntimeError(f"dbsp {what} failed with status {status}")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Ctx:
    """Per-device context (stream + arena).  Raises without a GPU."""

    def __init__(self, device=0):
        self._lib = _L()
        h = ctypes.c_void_p()
        _check(self._lib.dbsp_ctx_create(ctypes.byref(h), device), "ctx_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dbsp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def sync(self):
        _check(self._lib.dbsp_ctx_sync(self._h), "sync")

    # ---- host<->device row helpers (test plumbing) ----
    def upload_rows(self, rows: np.ndarray) -> BatchStruct:
        rows = np.ascontiguousarray(rows, dtype=ROW_DT)
        n = len(rows)
        b = BatchStruct()
        k = np.ascontiguousarray(rows["k"])
        v = np.ascontiguousarray(rows["v"])
        w = np.ascontiguousarray(rows["w"])
        for name, host in (("k", k), ("v", v), ("w", w)):
            d = ctypes.c_void_p()
            _check(self._lib.dbsp_dev_alloc(self._h, max(n, 1) * 8,
                                            ctypes.byref(d)), "alloc")
            if n:
                _check(self._lib.dbsp_h2d(self._h, d, _p(host), n * 8), "h2d")
            setattr(b, name, d)
        b.len = n
        self.sync()
        return b

    def download_rows(self, b: BatchStruct) -> np.ndarray:
        n = b.len
        out = np.empty(n, dtype=ROW_DT)
        if n:
            for name in ("k", "v", "w"):
                host = np.empty(n, dtype=np.uint64)
                _check(self._lib.dbsp_d2h(self._h, _p(host),
                                          getattr(b, name), n * 8), "d2h")
                out[name] = host.view(ROW_DT[name])
        return out

    def free_batch(self, b: BatchStruct):
        for name in ("k", "v", "w"):
            ptr = getattr(b, name)
            if ptr:
                self._lib.dbsp_dev_free(self._h, ptr)
                setattr(b, name, None)

    # ---- kernel primitives (GPU parity tests) ----
    def sort_consolidate(self, rows: np.ndarray) -> np.ndarray:
        raw = self.upload_rows(rows)
        out = BatchStruct()
        _check(self._lib.dbsp_sort_consolidate(self._h, raw.k, raw.v, raw.w,
                                               raw.len, ctypes.byref(out)),
               "sort_consolidate")
        self.sync()
        res = self.download_rows(out)
        self.free_batch(raw)
        self.free_batch(out)
        return res

    def merge(self, a_rows, b_rows) -> np.ndarray:
        a = self.upload_rows(a_rows)
        b = self.upload_rows(b_rows)
        out = BatchStruct()
        _check(self._lib.dbsp_merge(self._h, ctypes.byref(a), ctypes.byref(b),
                                    ctypes.byref(out)), "merge")
        res = self.download_rows(out)
        for x in (a, b, out):
            self.free_batch(x)
        return res

    def acc_fold(self, a_rows, b_rows, b_len=None) -> np.ndarray:
        """Fold the small delta b into the accumulator a (both consolidated).
        b_len overrides the delta length handed to the kernel (the poison
        test passes -1)."""
        a = self.upload_rows(a_rows)
        b = self.upload_rows(b_rows)
        if b_len is not None:
            b.len = b_len
        out = BatchStruct()
        try:
            _check(self._lib.dbsp_acc_fold(self._h, ctypes.byref(a),
                                           ctypes.byref(b),
                                           ctypes.byref(out)), "acc_fold")
            res = self.download_rows(out)
        finally:
            for x in (a, b, out):
                self.free_batch(x)
        return res

    def join(self, delta_rows, trace_rows, proj, param=0) -> np.ndarray:
        d = self.upload_rows(delta_rows)
        t = self.upload_rows(trace_rows)
        out = BatchStruct()
        _check(self._lib.dbsp_join(self._h, ctypes.byref(d), ctypes.byref(t),
                                   proj, param, ctypes.byref(out)), "join")
        self.sync()
        res = self.download_rows(out)
        for x in (d, t, out):
            self.free_batch(x)
        return res

    def join_spine(self, delta_rows, batches, proj, param=0,
                   path=1) -> np.ndarray:
        """delta x spine, the raw rows in the order the kernel wrote them.
        `batches` (at most 24, each sorted by (k, v)) reach the kernels
        verbatim, empty ones included.  path 1: the sized count / scan / emit
        route; path 2: the small route (probe, one-workgroup scan, emit over
        prepared counts), at most 8192 delta rows."""
        d = self.upload_rows(delta_rows)
        ups = [self.upload_rows(b) for b in batches]
        arr = (BatchStruct * max(len(ups), 1))(*ups)
        out = BatchStruct()
        try:
            _check(self._lib.dbsp_join_spine(self._h, ctypes.byref(d), arr,
                                             len(ups), proj, param, path,
                                             ctypes.byref(out)), "join_spine")
            res = self.download_rows(out)
        finally:
            for x in [d, out] + ups:
                self.free_batch(x)
        return res

    def join_tail(self, plans, cap=32768) -> dict:
        """The chained tick's probe + join tail over 1..3 plans.  A plan is a
        dict: "delta" (rows), "batches" (list of rows), "proj", and optionally
        "nd" (the delta length handed to the kernels in place of
        len(delta); negative and oversized ones are passed on), "fresh"
        (the one-batch trace is a tick-fresh delta) and "tn" (its length as
        the kernels see it).  Returns the verdicts "totals", "d_total",
        "d_flag", "d_final", "offsets" (per plan: the plan-local exclusive
        offsets, None where the total is negative), "store" (the output
        store's rows when d_final >= 0, else None) and "capbuf" (the capacity
        buffer's rows when only they are valid, else None)."""
        np_ = len(plans)
        arr = (JoinPlanStruct * max(np_, 1))()
        keep, offs = [], []
        for p, pl in enumerate(plans):
            d = self.upload_rows(pl["delta"])
            ups = [self.upload_rows(b) for b in pl["batches"]]
            tb = (BatchStruct * max(len(ups), 1))(*ups)
            keep.append((d, ups, tb))
            nd = pl.get("nd")
            arr[p].delta = d
            arr[p].nd = d.len if nd is None else nd
            arr[p].trace_batches = tb
            arr[p].n_batches = len(ups)
            arr[p].proj = pl["proj"]
            arr[p].fresh = 1 if pl.get("fresh") else 0
            tn = pl.get("tn")
            arr[p].tn = (ups[0].len if ups else 0) if tn is None else tn
            offs.append(np.zeros(max(d.len, 1), dtype=np.uint64))
        optr = (ctypes.c_void_p * max(np_, 1))(*[_p(o) for o in offs])
        verdict = (ctypes.c_int64 * 6)()
        out = BatchStruct()
        try:
            _check(self._lib.dbsp_join_tail(self._h, arr, np_, cap, verdict,
                                            optr, ctypes.byref(out)),
                   "join_tail")
            rows = self.download_rows(out)
        finally:
            for d, ups, _ in keep:
                for x in [d] + ups:
                    self.free_batch(x)
            self.free_batch(out)
        totals = [int(verdict[p]) for p in range(np_)]
        d_total, d_flag, d_final = (int(verdict[i]) for i in (3, 4, 5))
        return {
            "totals": totals, "d_total": d_total, "d_flag": d_flag,
            "d_final": d_final,
            "offsets": [offs[p][:max(int(arr[p].nd), 0)].copy()
                        if totals[p] >= 0 else None for p in range(np_)],
            "store": rows if d_final >= 0 else None,
            "capbuf": rows if d_final < 0 and d_flag == 0 and d_total >= 0
            else None,
        }

    def _agg_upsert(self, fn, what, keys, in_rows, out_rows) -> np.ndarray:
        """Upload the keys and both traces, run one dbsp_agg_*_upsert entry
        point (`fn`), download its rows; the device buffers go back even when
        the call raises."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        dk = ctypes.c_void_p()
        _check(self._lib.dbsp_dev_alloc(self._h, max(len(keys), 1) * 8,
                                        ctypes.byref(dk)), "alloc")
        if len(keys):
            _check(self._lib.dbsp_h2d(self._h, dk, _p(keys), len(keys) * 8), "h2d")
        it = self.upload_rows(in_rows)
        ot = self.upload_rows(out_rows)
        out = BatchStruct()
        try:
            _check(fn(self._h, dk, len(keys), ctypes.byref(it),
                      ctypes.byref(ot), ctypes.byref(out)), what)
            self.sync()
            res = self.download_rows(out)
        finally:
            self._lib.dbsp_dev_free(self._h, dk)
            for x in (it, ot, out):
                self.free_batch(x)
        return res

    def agg_linear_upsert(self, keys, in_rows, out_rows) -> np.ndarray:
        return self._agg_upsert(self._lib.dbsp_agg_linear_upsert, "agg",
                                keys, in_rows, out_rows)

    def agg_max_upsert(self, keys, in_rows, out_rows) -> np.ndarray:
        return self._agg_upsert(self._lib.dbsp_agg_max_upsert, "aggmax",
                                keys, in_rows, out_rows)

    def agg_last10_upsert(self, keys, in_rows, out_rows) -> np.ndarray:
        """q6's fold + upsert: per key the floor average of the last <= 10
        prices (low 27 bits of v) of its run in in_rows, then the key's
        out_rows negated; raw rows in kernel order."""
        return self._agg_upsert(self._lib.dbsp_agg_last10_upsert, "agglast10",
                                keys, in_rows, out_rows)

    def agg_sum_spine(self, delta_rows, batches):
        """(unique keys of the consolidated delta, emitted rows): per-key
        weight sums over `batches` (at most 24, passed verbatim), one row
        (key, sum, +1) per non-zero sum, in ticket order."""
        d = self.upload_rows(delta_rows)
        ups = [self.upload_rows(b) for b in batches]
        arr = (BatchStruct * max(len(ups), 1))(*ups)
        out = BatchStruct()
        dk = ctypes.c_void_p()
        nk = ctypes.c_int64()
        try:
            _check(self._lib.dbsp_agg_sum_spine(self._h, ctypes.byref(d), arr,
                                                len(ups), ctypes.byref(dk),
                                                ctypes.byref(nk),
                                                ctypes.byref(out)),
                   "agg_sum_spine")
            keys = np.empty(nk.value, dtype=np.uint64)
            if nk.value:
                _check(self._lib.dbsp_d2h(self._h, _p(keys), dk,
                                          nk.value * 8), "d2h")
            res = self.download_rows(out)
        finally:
            if dk:
                self._lib.dbsp_dev_free(self._h, dk)
            for x in [d, out] + ups:
                self.free_batch(x)
        return keys, res

    def wm_update(self, state, source, keys=(), n=None, gmax=0, width=1,
                  tumble=1, lag=0, bounds=None):
        """One k_wm_update step on scratch words.  state: {wm, s0, e0,
        have_prev}; source: "host_n", "dev_n" or "gmax"; keys: the sorted time
        keys uploaded, n the length the kernel sees (default len(keys));
        bounds: the 6 words the kernel finds (default zeros).  Returns
        (state after, bounds after) as lists of ints."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        st = (ctypes.c_uint64 * 4)(*[int(x) for x in state])
        bd = (ctypes.c_uint64 * 6)(*[int(x) for x in (bounds or [0] * 6)])
        dk = ctypes.c_void_p()
        _check(self._lib.dbsp_dev_alloc(self._h, max(len(keys), 1) * 8,
                                        ctypes.byref(dk)), "alloc")
        try:
            if len(keys):
                _check(self._lib.dbsp_h2d(self._h, dk, _p(keys),
                                          len(keys) * 8), "h2d")
            _check(self._lib.dbsp_wm_update(
                self._h, st, bd, WM_SOURCES[source], dk, len(keys),
                len(keys) if n is None else n, gmax, width, tumble, lag),
                "wm_update")
        finally:
            self._lib.dbsp_dev_free(self._h, dk)
        return [int(x) for x in st], [int(x) for x in bd]

    def window_spine(self, batches, tick_rows, bounds=None, chain=None):
        """The window stage over a spine (at most 24 batches, passed
        verbatim).  Route 1: bounds = (s0, e0, s1, e1, have_prev), handed to
        the ranges kernel by value.  Route 2: chain = dict(state, width,
        tumble, lag, and optionally wm_n / bn: the tick batch's length as the
        watermark / the ranges kernel reads it from the device, default
        len(tick_rows)); the bounds come from k_wm_update on the device.
        Returns dict(total, table (nreg x 5 int64, None for a -1 total), rows
        (kernel order), bounds (6 words) and, on route 2, state)."""
        ups = [self.upload_rows(b) for b in batches]
        tick = self.upload_rows(tick_rows)
        arr = (BatchStruct * max(len(ups), 1))(*ups)
        nreg = 3 * len(ups) + 1
        table = np.zeros((nreg, 5), dtype=np.int64)
        bd = (ctypes.c_uint64 * 6)()
        total = ctypes.c_int64()
        out = BatchStruct()
        ch = None
        if chain is None:
            for i, x in enumerate(bounds):
                bd[i] = int(x)
        else:
            ch = WindowChainStruct()
            for i, x in enumerate(chain["state"]):
                ch.state[i] = int(x)
            ch.wm_n = chain.get("wm_n", tick.len)
            ch.bn = chain.get("bn", tick.len)
            ch.width, ch.tumble, ch.lag = (chain["width"], chain["tumble"],
                                           chain["lag"])
        try:
            _check(self._lib.dbsp_window_spine(
                self._h, arr, len(ups), ctypes.byref(tick),
                1 if chain is None else 2, bd,
                None if ch is None else ctypes.byref(ch),
                ctypes.byref(total),
                table.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                ctypes.byref(out)), "window_spine")
            rows = self.download_rows(out)
        finally:
            for x in [tick, out] + ups:
                self.free_batch(x)
        res = {"total": total.value,
               "table": table if total.value >= 0 else None,
               "rows": rows, "bounds": [int(x) for x in bd]}
        if ch is not None:
            res["state"] = [int(x) for x in ch.state]
        return res

    def window(self, trace_rows, batch_rows, have_prev, s0, e0, s1, e1):
        t = self.upload_rows(trace_rows)
        b = self.upload_rows(batch_rows)
        out = BatchStruct()
        _check(self._lib.dbsp_window(self._h, ctypes.byref(t), ctypes.byref(b),
                                     1 if have_prev else 0, s0, e0, s1, e1,
                                     ctypes.byref(out)), "window")
        self.sync()
        res = self.download_rows(out)
        for x in (t, b, out):
            self.free_batch(x)
        return res

    def sort_consolidate_f64(self, rows: np.ndarray) -> np.ndarray:
        raw = self.upload_rows(rows)
        out = BatchStruct()
        _check(self._lib.dbsp_sort_consolidate_f64(self._h, raw.k, raw.v, raw.w,
                                                   raw.len, ctypes.byref(out)),
               "sort_consolidate_f64")
        self.sync()
        res = self.download_rows(out)
        self.free_batch(raw)
        self.free_batch(out)
        return res

    def merge_f64(self, a_rows, b_rows) -> np.ndarray:
        a = self.upload_rows(a_rows)
        b = self.upload_rows(b_rows)
        out = BatchStruct()
        _check(self._lib.dbsp_merge_f64(self._h, ctypes.byref(a),
                                        ctypes.byref(b), ctypes.byref(out)),
               "merge_f64")
        res = self.download_rows(out)
        for x in (a, b, out):
            self.free_batch(x)
        return res

    def weigh_f64(self, rows) -> np.ndarray:
        inp = self.upload_rows(rows)
        out = BatchStruct()
        _check(self._lib.dbsp_weigh_f64(self._h, ctypes.byref(inp),
                                        ctypes.byref(out)), "weigh_f64")
        self.sync()
        res = self.download_rows(out)
        for x in (inp, out):
            self.free_batch(x)
        return res

    def agg_linear_upsert_f64(self, keys, in_rows, out_rows) -> np.ndarray:
        return self._agg_upsert(self._lib.dbsp_agg_linear_upsert_f64, "aggf64",
                                keys, in_rows, out_rows)

    def distinct_inc(self, delta_rows, trace_batch_rows_list):
        d = self.upload_rows(delta_rows)
        batches = [self.upload_rows(b) for b in trace_batch_rows_list]
        arr = (BatchStruct * max(len(batches), 1))(*batches)
        out = BatchStruct()
        _check(self._lib.dbsp_distinct_inc(self._h, ctypes.byref(d), arr,
                                           len(batches), ctypes.byref(out)),
               "distinct")
        self.sync()
        res = self.download_rows(out)
        self.free_batch(d)
        for b in batches:
            self.free_batch(b)
        self.free_batch(out)
        return res

    def rolling_agg(self, rows, width):
        inp = self.upload_rows(rows)
        out = BatchStruct()
        _check(self._lib.dbsp_rolling_agg(self._h, ctypes.byref(inp), width,
                                          ctypes.byref(out)), "rolling")
        self.sync()
        res = self.download_rows(out)
        for x in (inp, out):
            self.free_batch(x)
        return res

    def rolling_minmax(self, rows, agg, before, after):
        """Per row (partition, ts << 32 | val, w) of a consolidated batch:
        (k, v, M) with M the "max" or "min" of val over the partition's rows
        with time in [ts - before, ts + after]."""
        code = roll_agg_code(agg)
        inp = self.upload_rows(rows)
        out = BatchStruct()
        st = self._lib.dbsp_rolling_minmax(self._h, ctypes.byref(inp), code,
                                           before, after, ctypes.byref(out))
        if st == 0:
            self.sync()
        res = self.download_rows(out) if st == 0 else None
        for x in (inp, out):
            self.free_batch(x)
        _check(st, "rolling_minmax")
        return res

    def truncate_below(self, rows, mode, bound):
        """Rows whose time is >= bound, in order.  mode 0: time = v (rows
        (partition, ts, w)); mode 1: time = k & 0xffffffff; mode 2: time =
        v >> 32 (rows (partition, ts << 32 | val, w))."""
        inp = self.upload_rows(rows)
        out = BatchStruct()
        st = self._lib.dbsp_truncate_below(self._h, ctypes.byref(inp), mode,
                                           bound, ctypes.byref(out))
        self.free_batch(inp)
        _check(st, "truncate_below")
        res = self.download_rows(out)
        self.free_batch(out)
        return res

    def rolling_create(self, before, after, agg="sum"):
        """Incremental partitioned rolling aggregate over
        [ts - before, ts + after] (see `Rolling`)."""
        return Rolling(self, before, after, agg=agg)

    def topk(self, rows, k, group_shift):
        """The last <= k rows of every group (key >> group_shift) of a
        consolidated batch, each at weight +1, in order: the recompute route
        of `TopK`."""
        inp = self.upload_rows(rows)
        out = BatchStruct()
        st = self._lib.dbsp_topk(self._h, ctypes.byref(inp), k, group_shift,
                                 ctypes.byref(out))
        self.free_batch(inp)
        _check(st, "topk")
        res = self.download_rows(out)
        self.free_batch(out)
        return res

    def antijoin(self, a_rows, b_keys, mode=0):
        """The rows of a consolidated batch whose key is absent from
        (ANTIJOIN) or present in (SEMIJOIN) a key set, in order: the
        recompute route of `AntiJoin`.  b_keys: rows (k, ignored, w) of
        sorted distinct keys with non-zero weights; a key is present iff its
        weight is > 0."""
        inp = self.upload_rows(a_rows)
        keys = self.upload_rows(b_keys)
        out = BatchStruct()
        st = self._lib.dbsp_antijoin(self._h, ctypes.byref(inp), keys.k,
                                     keys.w, keys.len, mode,
                                     ctypes.byref(out))
        self.free_batch(inp)
        self.free_batch(keys)
        _check(st, "antijoin")
        res = self.download_rows(out)
        self.free_batch(out)
        return res

    def argmax(self, rows, group_shift, rank_shift):
        """The rows of a consolidated batch whose rank (key >> rank_shift) is
        the largest of their group (key >> group_shift), weights unchanged,
        in order: the recompute route of `ArgMax`."""
        inp = self.upload_rows(rows)
        out = BatchStruct()
        st = self._lib.dbsp_argmax(self._h, ctypes.byref(inp), group_shift,
                                   rank_shift, ctypes.byref(out))
        self.free_batch(inp)
        _check(st, "argmax")
        res = self.download_rows(out)
        self.free_batch(out)
        return res

    def shard_partition(self, rows, nshards):
        inp = self.upload_rows(rows)
        out = BatchStruct()
        offs = np.zeros(nshards + 1, dtype=np.int64)
        _check(self._lib.dbsp_shard_partition(self._h, ctypes.byref(inp),
                                              nshards, ctypes.byref(out),
                                              _p(offs)), "shard")
        self.sync()
        res = self.download_rows(out)
        for x in (inp, out):
            self.free_batch(x)
        return res, offs


ROLL_AGGS = {"sum": ROLL_SUM, "max": ROLL_MAX, "min": ROLL_MIN}


def roll_agg_code(agg):
    try:
        return ROLL_AGGS[agg]
    except KeyError:
        raise ValueError(f"unknown rolling aggregator {agg!r}; "
                         f"one of {sorted(ROLL_AGGS)}") from None


class Rolling:
    """Stateful incremental partitioned rolling aggregate.

    agg="sum" (mirror of Stream::partitioned_rolling_aggregate_linear): input
    rows are (k = partition, v = ts, w) with partition, ts < 2^32; each step
    returns the tick's consolidated output delta (partition<<32 | ts, sum,
    +-1).

    agg="max" / "min" (Stream::partitioned_rolling_aggregate with Max / Min):
    input rows are (k = partition, v = ts << 32 | val, w) with partition
    < 2^32; one output (partition<<32 | ts, M, +-1) per time that holds a row
    of positive weight, M the extreme val of any non-zero weight over the
    range."""

    def __init__(self, ctx: Ctx, before: int, after: int, agg="sum"):
        self._ctx = ctx
        self._lib = ctx._lib
        self.agg = agg
        h = ctypes.c_void_p()
        _check(self._lib.dbsp_rolling_create_agg(ctx._h, roll_agg_code(agg),
                                                 before, after,
                                                 ctypes.byref(h)),
               "rolling_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._ctx, "_h", None):
                self._lib.dbsp_rolling_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def step(self, rows: np.ndarray, watermark=None) -> np.ndarray:
        """One tick: raw (unsorted, unconsolidated) delta rows in, output
        delta out.  Raises (state unchanged) on a partition or ts >= 2^32.

        With a watermark the operator first raises its own to
        max(current, watermark), drops and counts the rows below it, and
        afterwards may delete trace rows below watermark - (before + after)
        (see `wm_stats`, `compact`).  None leaves the watermark where it is."""
        raw = self._ctx.upload_rows(rows)
        out = BatchStruct()
        if watermark is None:
            st = self._lib.dbsp_rolling_step(self._h, raw.k, raw.v, raw.w,
                                             raw.len, ctypes.byref(out))
        else:
            st = self._lib.dbsp_rolling_step_wm(self._h, raw.k, raw.v, raw.w,
                                                raw.len, watermark,
                                                ctypes.byref(out))
        self._ctx.free_batch(raw)
        _check(st, "rolling_step")
        res = self._ctx.download_rows(out)
        self._ctx.free_batch(out)
        return res

    def compact(self):
        """Delete the trace rows below the current bound now."""
        _check(self._lib.dbsp_rolling_compact(self._h), "rolling_compact")

    def wm_stats(self):
        """(watermark, lower_bound, late_rows, sweeps)."""
        wm, lb = ctypes.c_uint64(), ctypes.c_uint64()
        late, sw = ctypes.c_int64(), ctypes.c_int64()
        _check(self._lib.dbsp_rolling_wm_stats(self._h, ctypes.byref(wm),
                                               ctypes.byref(lb),
                                               ctypes.byref(late),
                                               ctypes.byref(sw)),
               "rolling_wm_stats")
        return wm.value, lb.value, late.value, sw.value

    def stats(self):
        """(in_rows, in_batches, out_rows, out_batches) of the two traces."""
        ir, orr = ctypes.c_int64(), ctypes.c_int64()
        ib, ob = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.dbsp_rolling_stats(self._h, ctypes.byref(ir),
                                            ctypes.byref(ib),
                                            ctypes.byref(orr),
                                            ctypes.byref(ob)),
               "rolling_stats")
        return ir.value, ib.value, orr.value, ob.value


TOPK_REFILL_ALL = 1  # DBSP_TOPK_REFILL_ALL


class TopK:
    """Stateful incremental top-K per group (the aggregate(Fold) + flat_map
    of Nexmark q19).  Input rows are (k, v, w); a row's group is
    k >> group_shift and (k, v) order ranks the rows inside it.  The operator
    keeps, per group, the last min(k, present rows) rows whose total weight is
    non-zero, each at weight +1; each step returns the tick's consolidated
    change of that relation.  refill_all recomputes every affected group from
    its whole run (a diagnostic: outputs are the same)."""

    def __init__(self, ctx: Ctx, k: int, group_shift: int, refill_all=False):
        self._ctx = ctx
        self._lib = ctx._lib
        h = ctypes.c_void_p()
        _check(self._lib.dbsp_topk_create(
            ctx._h, k, group_shift, TOPK_REFILL_ALL if refill_all else 0,
            ctypes.byref(h)), "topk_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._ctx, "_h", None):
                self._lib.dbsp_topk_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def step(self, rows: np.ndarray) -> np.ndarray:
        """One tick: raw (unsorted, unconsolidated) delta rows in, the
        consolidated output delta (k, v, +-1) out."""
        raw = self._ctx.upload_rows(rows)
        out = BatchStruct()
        st = self._lib.dbsp_topk_step(self._h, raw.k, raw.v, raw.w, raw.len,
                                      ctypes.byref(out))
        self._ctx.free_batch(raw)
        _check(st, "topk_step")
        res = self._ctx.download_rows(out)
        self._ctx.free_batch(out)
        return res

    def stats(self) -> dict:
        """in_rows / in_batches / out_rows / out_batches of the two traces
        and the cumulative groups_seen, groups_refilled, rows_gathered."""
        ir, orr = ctypes.c_int64(), ctypes.c_int64()
        ib, ob = ctypes.c_int(), ctypes.c_int()
        gs, gr, rg = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(self._lib.dbsp_topk_stats(
            self._h, ctypes.byref(ir), ctypes.byref(ib), ctypes.byref(orr),
            ctypes.byref(ob), ctypes.byref(gs), ctypes.byref(gr),
            ctypes.byref(rg)), "topk_stats")
        return {"in_rows": ir.value, "in_batches": ib.value,
                "out_rows": orr.value, "out_batches": ob.value,
                "groups_seen": gs.value, "groups_refilled": gr.value,
                "rows_gathered": rg.value}


ANTIJOIN, SEMIJOIN = 0, 1  # DBSP_ANTIJOIN, DBSP_SEMIJOIN


class AntiJoin:
    """Stateful incremental antijoin (Stream::antijoin) or semijoin.  Left
    rows are (k, v, w); the right side is a key set, rows (k, ignored, w).
    A key is present iff its total weight in the right side's integral is
    > 0.  The maintained relation is the left integral restricted to the
    absent (ANTIJOIN) or present (SEMIJOIN) keys; each step returns the
    tick's consolidated change of it.  The semijoin keeps a left row's own
    weight: it is A joined with distinct(B), not the reference's per-batch
    semijoin_stream."""

    def __init__(self, ctx: Ctx, mode=ANTIJOIN):
        self._ctx = ctx
        self._lib = ctx._lib
        h = ctypes.c_void_p()
        _check(self._lib.dbsp_antijoin_create(ctx._h, mode, ctypes.byref(h)),
               "antijoin_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._ctx, "_h", None):
                self._lib.dbsp_antijoin_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def step(self, a_rows: np.ndarray, b_keys: np.ndarray) -> np.ndarray:
        """One tick: raw (unsorted, unconsolidated) left rows and right keys
        in, either possibly empty; the consolidated output delta out."""
        a = self._ctx.upload_rows(a_rows)
        b = self._ctx.upload_rows(b_keys)
        out = BatchStruct()
        st = self._lib.dbsp_antijoin_step(self._h, a.k, a.v, a.w, a.len, b.k,
                                          b.w, b.len, ctypes.byref(out))
        self._ctx.free_batch(a)
        self._ctx.free_batch(b)
        _check(st, "antijoin_step")
        res = self._ctx.download_rows(out)
        self._ctx.free_batch(out)
        return res

    def stats(self) -> dict:
        """a_rows / a_batches / b_rows / b_batches of the two traces and the
        cumulative keys_flipped, rows_gathered, rows_filtered."""
        ar, br = ctypes.c_int64(), ctypes.c_int64()
        ab, bb = ctypes.c_int(), ctypes.c_int()
        kf, rg, rf = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(self._lib.dbsp_antijoin_stats(
            self._h, ctypes.byref(ar), ctypes.byref(ab), ctypes.byref(br),
            ctypes.byref(bb), ctypes.byref(kf), ctypes.byref(rg),
            ctypes.byref(rf)), "antijoin_stats")
        return {"a_rows": ar.value, "a_batches": ab.value,
                "b_rows": br.value, "b_batches": bb.value,
                "keys_flipped": kf.value, "rows_gathered": rg.value,
                "rows_filtered": rf.value}


ARGMAX_REFILL_ALL = 1  # DBSP_ARGMAX_REFILL_ALL


class ArgMax:
    """Stateful incremental arg-max per group with ties (the tail of Nexmark
    q7).  Input rows are (k, v, w); a row's group is k >> group_shift and its
    rank k >> rank_shift, rank_shift <= group_shift.  The operator keeps, per
    group, every row of non-zero total weight whose rank is the group's
    largest, at that total weight; each step returns the tick's consolidated
    change of that relation.  refill_all recomputes every affected group from
    its whole run (a diagnostic: outputs are the same)."""

    def __init__(self, ctx: Ctx, group_shift: int, rank_shift: int,
                 refill_all=False):
        self._ctx = ctx
        self._lib = ctx._lib
        h = ctypes.c_void_p()
        _check(self._lib.dbsp_argmax_create(
            ctx._h, group_shift, rank_shift,
            ARGMAX_REFILL_ALL if refill_all else 0, ctypes.byref(h)),
            "argmax_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._ctx, "_h", None):
                self._lib.dbsp_argmax_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def step(self, rows: np.ndarray) -> np.ndarray:
        """One tick: raw (unsorted, unconsolidated) delta rows in, the
        consolidated output delta out."""
        raw = self._ctx.upload_rows(rows)
        out = BatchStruct()
        st = self._lib.dbsp_argmax_step(self._h, raw.k, raw.v, raw.w, raw.len,
                                        ctypes.byref(out))
        self._ctx.free_batch(raw)
        _check(st, "argmax_step")
        res = self._ctx.download_rows(out)
        self._ctx.free_batch(out)
        return res

    def stats(self) -> dict:
        """in_rows / in_batches / out_rows / out_batches of the two traces
        and the cumulative groups_seen, groups_refilled, rows_gathered."""
        ir, orr = ctypes.c_int64(), ctypes.c_int64()
        ib, ob = ctypes.c_int(), ctypes.c_int()
        gs, gr, rg = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(self._lib.dbsp_argmax_stats(
            self._h, ctypes.byref(ir), ctypes.byref(ib), ctypes.byref(orr),
            ctypes.byref(ob), ctypes.byref(gs), ctypes.byref(gr),
            ctypes.byref(rg)), "argmax_stats")
        return {"in_rows": ir.value, "in_batches": ib.value,
                "out_rows": orr.value, "out_batches": ob.value,
                "groups_seen": gs.value, "groups_refilled": gr.value,
                "rows_gathered": rg.value}


def xxh3_u64(key, seed=0x7F95EF85BE33C337):
    return _L().dbsp_xxh3_u64(key, seed)


class Engine:
    """One Nexmark query circuit on one GPU (mirror of Runtime::init_circuit +
    DBSPHandle::step)."""

    def __init__(self, ctx: Ctx, query: int, rank=0, world=1):
        self._ctx = ctx
        self._lib = ctx._lib
        h = ctypes.c_void_p()
        _check(self._lib.dbsp_engine_create(ctypes.byref(h), ctx._h, query,
                                            rank, world), "engine_create")
        self._h = h
        self.query = query

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dbsp_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def stage(self, events: np.ndarray):
        events = np.ascontiguousarray(events, dtype=EVENT_DT)
        _check(self._lib.dbsp_engine_stage_events(self._h, _p(events),
                                                  len(events)), "stage")
        self._staged = events  # keep alive

    def c5_init(self, n_trace, n_delta, seed=41):
        """Config C5 (query 100): device-generate the n_trace-row indexed
        trace and fix the per-tick delta size; step ranges then index delta
        rows (run_staged(0, steps*n_delta, n_delta) = `steps` ticks)."""
        _check(self._lib.dbsp_engine_c5_init(self._h, n_trace, n_delta, seed),
               "c5_init")

    def rolling_init(self, before, after):
        """Query 101 / 102: the rolling range [date_time - before, date_time +
        after] in ms (defaults 10000 / 0); rejected after the first step."""
        _check(self._lib.dbsp_engine_rolling_init(self._h, before, after),
               "rolling_init")

    def rolling_agg(self, agg):
        """Query 102: "max" (the default) or "min"; rejected after the first
        step."""
        _check(self._lib.dbsp_engine_rolling_agg(self._h, roll_agg_code(agg)),
               "rolling_agg")

    def rolling_lateness(self, ms):
        """Query 101 / 102: bound the operator's state by the watermark
        max(bid date_time so far) - ms; rejected after the first step."""
        _check(self._lib.dbsp_engine_rolling_lateness(self._h, ms),
               "rolling_lateness")

    def rolling_stats(self):
        """Query 101 / 102: (in_rows, out_rows, late_rows, sweeps)."""
        vals = [ctypes.c_int64() for _ in range(4)]
        _check(self._lib.dbsp_engine_rolling_stats(
            self._h, *[ctypes.byref(x) for x in vals]), "rolling_stats")
        return tuple(x.value for x in vals)

    def topk_init(self, k):
        """Query 19: how many bids per auction to keep (default 10);
        rejected after the first step."""
        _check(self._lib.dbsp_engine_topk_init(self._h, k), "topk_init")

    def topk_stats(self) -> dict:
        """Query 19: in_rows, out_rows and the cumulative groups_seen,
        groups_refilled, rows_gathered."""
        vals = [ctypes.c_int64() for _ in range(5)]
        _check(self._lib.dbsp_engine_topk_stats(
            self._h, *[ctypes.byref(x) for x in vals]), "topk_stats")
        return dict(zip(("in_rows", "out_rows", "groups_seen",
                         "groups_refilled", "rows_gathered"),
                        (x.value for x in vals)))

    def antijoin_stats(self) -> dict:
        """Query 103: a_rows, b_rows and the cumulative keys_flipped,
        rows_gathered, rows_filtered."""
        vals = [ctypes.c_int64() for _ in range(5)]
        _check(self._lib.dbsp_engine_antijoin_stats(
            self._h, *[ctypes.byref(x) for x in vals]), "antijoin_stats")
        return dict(zip(("a_rows", "b_rows", "keys_flipped", "rows_gathered",
                         "rows_filtered"), (x.value for x in vals)))

    def argmax_stats(self) -> dict:
        """Query 7: in_rows, out_rows and the cumulative groups_seen,
        groups_refilled, rows_gathered."""
        vals = [ctypes.c_int64() for _ in range(5)]
        _check(self._lib.dbsp_engine_argmax_stats(
            self._h, *[ctypes.byref(x) for x in vals]), "argmax_stats")
        return dict(zip(("in_rows", "out_rows", "groups_seen",
                         "groups_refilled", "rows_gathered"),
                        (x.value for x in vals)))

    def step_staged(self, lo, hi):
        _check(self._lib.dbsp_engine_step_staged(self._h, lo, hi), "step")

    def run_staged(self, lo, hi, tick):
        """Tick loop inside the C side (the benchmark hot path)."""
        _check(self._lib.dbsp_engine_run_staged(self._h, lo, hi, tick), "run")

    def step(self, events: np.ndarray):
        events = np.ascontiguousarray(events, dtype=EVENT_DT)
        _check(self._lib.dbsp_engine_step(self._h, _p(events), len(events)),
               "step")

    def output(self, cap=1 << 22) -> np.ndarray:
        out = np.empty(cap, dtype=ROW_DT)
        n = ctypes.c_int64()
        _check(self._lib.dbsp_engine_output(self._h, _p(out), cap,
                                            ctypes.byref(n)), "output")
        return out[:n.value].copy()

    def output_events(self, cap=1 << 22) -> np.ndarray:
        out = np.empty(cap, dtype=EVENT_DT)
        n = ctypes.c_int64()
        _check(self._lib.dbsp_engine_output_events(self._h, _p(out), cap,
                                                   ctypes.byref(n)), "output")
        return out[:n.value].copy()

    def kernel_stats(self, kind):
        ms = ctypes.c_double()
        by = ctypes.c_double()
        ln = ctypes.c_int64()
        _check(self._lib.dbsp_engine_kernel_stats(self._h, kind,
                                                  ctypes.byref(ms),
                                                  ctypes.byref(by),
                                                  ctypes.byref(ln)), "stats")
        return ms.value, by.value, ln.value
