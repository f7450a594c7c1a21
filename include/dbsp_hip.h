/* dbsp_hip.h — C-ABI boundary of the MI355X-native DBSP hot path.
 *
 * This is the FFI line that sits beneath operator `eval` in the reference's
 * Circuit/Stream API (reference: crates/dbsp/src/circuit/operator_traits.rs:18-430,
 * registered via circuit_builder.rs:626-900).  The reference is pure Rust with no
 * FFI; its hot-path subsystems (trace merge, consolidation, join, aggregate,
 * sharding) are re-implemented here as CDNA4 HIP kernels behind these extern "C"
 * entry points.  A Rust host (the north-star configuration) would bind exactly
 * these symbols; see INTEGRATION.md for the bindgen/extern-"C" stub a
 * crates/dbsp maintainer would add.  In this environment (no Rust toolchain)
 * the host-side mirror of the Stream/Circuit API is C++
 * (database-stream-processor_amd/csrc/engine.cpp) and calls the same symbols.
 *
 * Data model: a Z-set / indexed-Z-set batch is a struct-of-arrays of rows
 *   (key: u64, val: u64, weight: i64), sorted lexicographically by (key, val),
 * resident in device HBM.  This is the MI355X-native restatement of
 *   - ColumnLayer{keys,diffs}             (trace/layers/column_layer/mod.rs:31-36)
 *   - OrderedLayer{keys,offs,vals}        (trace/layers/ordered/mod.rs:32-44)
 *   - OrdZSet / OrdIndexedZSet            (trace/ord/zset_batch.rs:28,
 *                                          trace/ord/indexed_zset_batch.rs:27-41)
 * The CSR `offs` index of the reference is not materialised: kernels locate a
 * key's value range by binary search over the sorted (key,val) rows; this trades
 * the offs array for two log2(n) probes and keeps batches a single layout.
 *
 * All calls are asynchronous on the caller's hipStream_t and ordered by it
 * (the reference's per-worker scheduler thread maps to one HIP stream).
 * Output sizes are data-dependent (zero-weight elimination); calls take a
 * caller-owned device scratch arena and return lengths via device or host
 * pointers as documented per entry point.
 */
#ifndef DBSP_HIP_H
#define DBSP_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
typedef int32_t dbsp_status;
#define DBSP_OK                0
#define DBSP_ERR_NOGPU        -1  /* no HIP device: the product path fails loudly, never falls back */
#define DBSP_ERR_OOM          -2
#define DBSP_ERR_INVALID      -3
#define DBSP_ERR_OVERFLOW     -4  /* output exceeded provided capacity */
#define DBSP_ERR_INTERNAL     -5

/* ---- event row (Nexmark ingress; model: crates/nexmark/src/model.rs:14-69) ----
 * kind: 0 = Person, 1 = Auction, 2 = Bid.
 * Person : f0=id, f1=name_id, f2=city_id, f3=state_id, f4=date_time
 * Auction: f0=id, f1=seller,  f2=category, f3=date_time, f4=expires
 * Bid    : f0=auction, f1=bidder, f2=price, f3=date_time, f4=0
 * Strings are carried as dictionary ids end-to-end (SURVEY.md §7 hard part (b));
 * egress would map ids back through the dictionary. */
typedef struct {
    uint64_t kind;
    uint64_t f0, f1, f2, f3, f4;
    int64_t  w;
} dbsp_event;

/* ---- Z-set row ---- */
typedef struct {
    uint64_t k;
    uint64_t v;
    int64_t  w;
} dbsp_row;

/* ---- batch descriptor: SoA device pointers, rows sorted lex by (k,v) ---- */
typedef struct {
    uint64_t *k;     /* device */
    uint64_t *v;     /* device */
    int64_t  *w;     /* device */
    int64_t   len;
} dbsp_batch;

/* ---- join output projections ----
 * The reference's join takes a per-query `join_func` closure
 * (operator/join.rs:180,217: Fn(&K,&V1,&V2)->Z::Key).  Kernels monomorphise the
 * projections the Nexmark hot path needs (the same move the reference makes for
 * its typed, non-JIT path).  Each mode maps (k, v1, v2) -> output (hi, lo). */
typedef enum {
    DBSP_PROJ_HI_V2_LO_V1    = 0, /* q3: delta=auction_by_seller, trace=person_by_id */
    DBSP_PROJ_HI_V1_LO_V2    = 1, /* q3 swapped side */
    DBSP_PROJ_HI_K_LO_V1V2   = 2, /* generic pair join (reference join.rs:886 tests):
                                     lo = v1<<32 | (v2 & lo32); vals are 32-bit */
    DBSP_PROJ_HI_K_LO_V1RND  = 3, /* q8: lo = (v1 & hi32) | round_down(v1 & lo32, param) */
    DBSP_PROJ_HI_K_LO_V2RND  = 4, /* q8 swapped side */
    DBSP_PROJ_HI_V2_LO_K     = 5, /* q5 final join */
    DBSP_PROJ_HI_V1_LO_K     = 6, /* q5 final join swapped side */
    DBSP_PROJ_HI_K_LO_V2V1   = 7, /* generic pair join, swapped side:
                                     lo = v2<<32 | (v1 & lo32) */
    DBSP_PROJ_HI_K_LO_V2     = 8, /* (k, v2): keeps the join key, takes the trace val
                                     (full 64-bit; the C5 join -> f64-sum pipeline) */
    DBSP_PROJ_Q4_BID_X_AUC   = 9, /* q4.rs:58-68 join_func: delta=bid
                                     (v=bid_dt<<27|price), trace=auction
                                     (v=a_dt<<28|(expires-a_dt)<<4|(cat&0xF)):
                                     emit ((auction<<4)|cat, price) iff
                                     a_dt <= bid_dt <= expires, else weight 0
                                     (dropped by the consolidate).  Fields:
                                     price 27 bits, expires-a_dt 24, cat 4;
                                     auction<<4 keeps its low 64 bits */
    DBSP_PROJ_Q4_AUC_X_BID   = 10, /* q4 swapped side */
    DBSP_PROJ_Q6_BID_X_AUC   = 11, /* q6.rs:60-80: delta=bid, trace=auction
                                      (v=a_dt<<36|(expires-a_dt)<<20|seller):
                                      emit ((auction<<20)|seller, price) in
                                      the validity window, else weight 0.
                                      Fields: expires-a_dt 16 bits, seller 20;
                                      the bid packs as for q4 */
    DBSP_PROJ_Q6_AUC_X_BID   = 12, /* q6 swapped side */
} dbsp_proj;

/* ======================================================================
 * Kernel-level entry points (each replaces a reference hot-path routine)
 * ====================================================================== */

/* Opaque per-device context: owns the HIP stream, scratch arena, RCCL comm. */
typedef struct dbsp_ctx dbsp_ctx;

dbsp_status dbsp_ctx_create(dbsp_ctx **out, int device);
dbsp_status dbsp_ctx_destroy(dbsp_ctx *ctx);
/* Blocks until all queued work on the context stream is complete. */
dbsp_status dbsp_ctx_sync(dbsp_ctx *ctx);

/* Device memory management (HBM arena; 288 GB per GPU). */
dbsp_status dbsp_dev_alloc(dbsp_ctx *ctx, size_t bytes, void **out);
dbsp_status dbsp_dev_free(dbsp_ctx *ctx, void *p);
dbsp_status dbsp_h2d(dbsp_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
dbsp_status dbsp_d2h(dbsp_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* Sort + consolidate unsorted rows into a batch.
 * Replaces consolidate_slice / consolidate_paired_slices
 * (trace/consolidation/mod.rs:91-110,212-231 — "the hottest code within the
 * entirety of the program") and the MergeBatcher seal path
 * (trace/ord/merge_batcher/mod.rs:22-197).
 * In : rows_in (device, len n, unsorted, arbitrary weights)
 * Out: batch `out` (device arrays allocated by the context arena), out->len set
 *      (host-visible after dbsp_ctx_sync). */
dbsp_status dbsp_sort_consolidate(dbsp_ctx *ctx,
                                  const uint64_t *k_in, const uint64_t *v_in,
                                  const int64_t *w_in, int64_t n,
                                  dbsp_batch *out);

/* Merge two sorted batches, summing weights of equal (k,v), dropping zeros.
 * Replaces ColumnLayerBuilder::push_merge (trace/layers/column_layer/builders.rs:98-169),
 * OrderedBuilder::merge_step (trace/layers/ordered/mod.rs:344-396) and the
 * fueled variants (ordered/mod.rs:493-575): a 2-level CSR merge over
 * OrdIndexedZSet is exactly a 1-level merge over (key,val) composite rows.
 * Merge-path (diagonal) partitioned; two-phase count+emit. */
dbsp_status dbsp_merge(dbsp_ctx *ctx, const dbsp_batch *a, const dbsp_batch *b,
                       dbsp_batch *out);

/* Fold a small consolidated delta (at most 8192 rows) into a consolidated
 * accumulator: the same result as dbsp_merge(acc, delta), by the kernel the
 * pipelined q3 tick uses for its in-train accumulator merge.  The delta's
 * length reaches the kernel through a device length slot, verbatim, as it
 * does there; a negative length is that path's poison and comes back as
 * DBSP_ERR_INTERNAL with `out` untouched.  Synchronous: out->len is final on
 * return. */
dbsp_status dbsp_acc_fold(dbsp_ctx *ctx, const dbsp_batch *acc,
                          const dbsp_batch *delta, dbsp_batch *out);

/* Delta x trace join with projection.
 * Replaces Join::eval (operator/join.rs:436-473) and the JoinTrace::eval inner
 * loop (operator/join.rs:732-787) at root scope (Time = (), time/mod.rs:223-235).
 * For every delta row (k,v1,w1) and every trace row (k,v2,w2) with equal k,
 * emits proj(k,v1,v2) with weight w1*w2.  Output is RAW (unconsolidated);
 * callers consolidate once per tick as the reference's output batcher does
 * (join.rs:792-850 degenerates to a single consolidate at Time=()).
 * The trace side may be a spine of several batches: join is linear in the
 * trace, so callers loop batches and concatenate. */
dbsp_status dbsp_join(dbsp_ctx *ctx, const dbsp_batch *delta,
                      const dbsp_batch *trace, dbsp_proj proj, uint64_t param,
                      dbsp_batch *out_raw);

/* dbsp_join against a whole spine, by the kernels the engine's ticks run.
 * trace_batches: n_batches (0..24) batches, each sorted by (k, v); they reach
 * the kernels verbatim, an empty batch keeping its slot.  path 1: the sized
 * count / scan / emit route (any delta length).  path 2: the small route, a
 * block probe, a one-workgroup scan and the emit over prepared counts, as the
 * linear aggregate's retractions chain them; a delta above 8192 rows is
 * DBSP_ERR_INVALID.  out_raw holds the raw rows in the order the emit wrote
 * them: delta row major, then batch, then trace position; an invalid q4 / q6
 * pair keeps its slot with weight 0.  Synchronous. */
dbsp_status dbsp_join_spine(dbsp_ctx *ctx, const dbsp_batch *delta,
                            const dbsp_batch *trace_batches, int n_batches,
                            dbsp_proj proj, uint64_t param, int path,
                            dbsp_batch *out_raw);

/* One plan of the chained join tail: delta x trace under proj (param 0).
 * delta.len is the rows its columns hold (the capacity); nd is the length
 * handed to the kernels through a device length slot, verbatim, so a negative
 * one or one above 8192 is passed on (a length in 0..8192 above delta.len is
 * DBSP_ERR_INVALID: it would be read).  fresh != 0 marks a one-batch trace
 * that is itself a tick-fresh delta: its length tn then travels through a
 * device slot too (tn above trace_batches[0].len is DBSP_ERR_INVALID). */
typedef struct {
    dbsp_batch delta;
    int64_t nd;
    const dbsp_batch *trace_batches;
    int n_batches;  /* 1..24 */
    dbsp_proj proj;
    int fresh;
    int64_t tn;
} dbsp_join_plan;

/* The chained tick's join tail over 1..3 plans: the probe that keeps the run
 * starts, then the one-workgroup tail (scan, capacity check, emit into a
 * capacity buffer of cap >= 8192 rows, sort + consolidate through an
 * 8192-row scratch into an 8192-row output store).  Synchronous.
 * verdict (host, 6 words): totals[0..2] (-1: that plan read a poisoned
 * length; unused plans 0), then d_total, d_flag, d_final as the kernel left
 * them.  offsets_host[p] (host, plans[p].nd words) receives plan p's
 * plan-local exclusive offsets when totals[p] >= 0.  out (device, caller
 * frees): the output store's first d_final rows when d_final >= 0; else the
 * capacity buffer's first d_total rows when d_flag == 0 and d_total >= 0;
 * else empty. */
dbsp_status dbsp_join_tail(dbsp_ctx *ctx, const dbsp_join_plan *plans, int np,
                           int64_t cap, int64_t *verdict,
                           uint64_t *const *offsets_host, dbsp_batch *out);

/* Linear aggregate + upsert for the aggregate_linear path.
 * Replaces AggregateIncremental::eval_key with the WeightedCount aggregator
 * (operator/aggregate/mod.rs:129-156,479-547) followed by Upsert::eval
 * (operator/upsert.rs:161-208).
 * In : delta_keys (device, nd distinct sorted keys = keys of this tick's delta),
 *      input trace (integral of the weighed stream, incl. this tick),
 *      output trace (integral of this operator's own output, excl. this tick).
 * Out: raw update rows: for each key with new aggregate s != 0 emit (key, s, +1);
 *      for each existing (key, v, w_sum != 0) in the output trace emit (key, v, -w_sum).
 *      Caller consolidates. */
/* Radix-tree rolling aggregate (operator/time_series/radix_tree/mod.rs:1-75
 * + rolling_aggregate.rs:235-280): per row (partition, ts, w)
 * of a consolidated batch, the weight sum over the partition rows with time
 * in [ts-width, ts] (RelRange::range_of, range.rs:93-110).  Implemented as a
 * flat radix-16 prefix-aggregate tree over the sorted rows (O(log) query). */
dbsp_status dbsp_rolling_agg(dbsp_ctx *ctx, const dbsp_batch *in,
                             uint64_t width, dbsp_batch *out);

/* Incremental partitioned rolling aggregate, linear weight-sum aggregator:
 * the stateful operator over the primitive above.  Replaces
 * PartitionedRollingAggregate::eval (operator/time_series/
 * rolling_aggregate.rs:487-604) and its two traces (the input trace and the
 * output trace, rolling_aggregate.rs:286-359).
 * Input deltas are rows (k = partition, v = ts, w); a value to be summed is
 * weighed into w beforehand (aggregate/mod.rs:297-323).  partition and ts
 * must be < 2^32.  range_of(ts) = [sat_sub(ts, before), ts + after], closed
 * (RelRange::new(Before(before), After(after)), range.rs:93-104); any u64
 * before/after, the upper end clamped to 2^32-1.
 * Output deltas are rows (k = partition<<32 | ts, v = sum as i64 bits,
 * w = +-1): per tick, every previous output at a time the delta can affect
 * is retracted and every such time whose total input weight is > 0
 * (!weight.le0(), rolling_aggregate.rs:574) is re-emitted with its new sum,
 * so a late row updates the aggregates at later times.  Work per tick
 * follows the affected rows, not the trace. */
typedef struct dbsp_rolling dbsp_rolling;
/* rolling_aggregate.rs:286-359 (circuit construction: the operator, its
 * input trace and the delayed output-trace feedback) */
dbsp_status dbsp_rolling_create(dbsp_ctx *ctx, uint64_t before, uint64_t after,
                                dbsp_rolling **out);
/* The operator's aggregator (the Agg of partitioned_rolling_aggregate<TS, V,
 * Agg>, rolling_aggregate.rs:235-321; its eval, :487-604, combines tree nodes
 * with Agg::Semigroup).  DBSP_ROLL_SUM is the linear aggregator above.
 * DBSP_ROLL_MAX / DBSP_ROLL_MIN are aggregate/max.rs:36-55 / min.rs:38-57:
 * Input deltas are rows (k = partition, v = ts << 32 | val, w) with
 * partition, ts, val < 2^32, so any 64-bit v is valid and (k, v) order is
 * (partition, ts, val) order; partition >= 2^32 is DBSP_ERR_INVALID with the
 * state unchanged.  range_of as above.
 * A time (partition, ts) is output iff the input integral holds a row at it
 * with w > 0 (the value loop breaks at the first !weight.le0(),
 * rolling_aggregate.rs:572-592: once per time however many values it holds,
 * never for a time of negative rows only).  Its value M is the max (min) of
 * val over the partition's integral rows with time in range_of(ts) and ANY
 * non-zero weight, negative included (Max::aggregate / Min::aggregate return
 * the extreme value "with non-zero weight"; the tree's leaves are that
 * aggregate per time, radix_tree/updater.rs:393).
 * Output deltas are rows (k = partition<<32 | ts, v = M, w = +-1), the tick's
 * change of that relation, consolidated.  Ranges that exclude the row's own
 * time (an Option output) and arbitrary Fold aggregators are out of scope. */
typedef enum { DBSP_ROLL_SUM = 0, DBSP_ROLL_MAX = 1, DBSP_ROLL_MIN = 2 } dbsp_roll_agg;
/* rolling_aggregate.rs:286-359 with the aggregator chosen; fixed for the
 * handle's life.  dbsp_rolling_step, _step_wm (time = v >> 32 for MAX / MIN:
 * late rows, watermark and sweeps as for the sum), _stats, _compact,
 * _wm_stats and _destroy take either kind of handle.  dbsp_rolling_create is
 * this call with DBSP_ROLL_SUM. */
dbsp_status dbsp_rolling_create_agg(dbsp_ctx *ctx, dbsp_roll_agg agg,
                                    uint64_t before, uint64_t after,
                                    dbsp_rolling **out);
/* Radix-tree rolling Max / Min batch primitive (radix_tree/mod.rs:1-75 with
 * Agg::Semigroup = max | min; leaves radix_tree/updater.rs:393): one output
 * row per row (partition, ts << 32 | val, w) of a consolidated batch:
 * (k, v, w = M as i64) with M over the partition's rows with time in
 * [ts - before, ts + after], rows of either sign counting.  MAX or MIN only
 * (DBSP_ERR_INVALID otherwise). */
dbsp_status dbsp_rolling_minmax(dbsp_ctx *ctx, const dbsp_batch *in,
                                dbsp_roll_agg agg, uint64_t before,
                                uint64_t after, dbsp_batch *out);
/* rolling_aggregate.rs:487-604 (eval).  k/v/w: n raw (unsorted,
 * unconsolidated) delta rows in device memory; out: the tick's consolidated
 * output delta (device arrays owned by the caller, null when empty; host
 * visible on return).  DBSP_ERR_INVALID, with the operator's state
 * unchanged, if a partition or ts is >= 2^32 (detected on the device). */
dbsp_status dbsp_rolling_step(dbsp_rolling *r, const uint64_t *k,
                              const uint64_t *v, const int64_t *w, int64_t n,
                              dbsp_batch *out);
/* rows / spine batches of the input and output traces (Spine introspection,
 * trace/spine_fueled.rs:107-119); any out pointer may be null */
dbsp_status dbsp_rolling_stats(dbsp_rolling *r, int64_t *in_rows,
                               int *in_batches, int64_t *out_rows,
                               int *out_batches);
dbsp_status dbsp_rolling_destroy(dbsp_rolling *r);

/* Watermark-bounded state (partitioned_rolling_aggregate_with_watermark,
 * rolling_aggregate.rs:155-220 and :286-321).  The operator keeps a monotone
 * watermark wm (0 at creation) and the bound
 * lb = sat_sub(wm, before + after), 0 if before + after overflows u64.
 * Rows of both traces with time < lb may be deleted: a row at ts >= wm only
 * affects times >= wm - after, whose sums and retractions read nothing
 * below lb, so the per-tick output equals the unbounded operator's as long
 * as every row has ts >= wm.  A step with watermark x:
 *   1. wm' = max(wm, x);
 *   2. rows of the consolidated delta with ts < wm' are dropped whole and
 *      counted (the reference only "does not expect" them,
 *      rolling_aggregate.rs:126-129; dropping is this library's choice);
 *   3. the dbsp_rolling_step tick on the surviving rows; on its
 *      DBSP_ERR_INVALID nothing changes, wm and the counters included;
 *   4. each trace whose rows exceed 2 * (rows after its previous sweep)
 *      + 4096 is swept at lb (the TraceBounds lower bound, operator/
 *      trace.rs:463-607, as an order-preserving device compaction) and its
 *      surviving batches merged into one; no sweep while lb = 0.
 * n == 0 still advances the watermark and may sweep.  dbsp_rolling_step is
 * this call with watermark 0. */
dbsp_status dbsp_rolling_step_wm(dbsp_rolling *r, const uint64_t *k,
                                 const uint64_t *v, const int64_t *w, int64_t n,
                                 uint64_t watermark, dbsp_batch *out);
/* sweep both traces at the current bound now, whatever the policy says
 * (trace.rs:463-607) */
dbsp_status dbsp_rolling_compact(dbsp_rolling *r);
/* watermark.rs:33-75 state and the bound derived from it
 * (rolling_aggregate.rs:199-204), rows dropped as late, traces swept; any
 * pointer may be null */
dbsp_status dbsp_rolling_wm_stats(dbsp_rolling *r, uint64_t *watermark,
                                  uint64_t *lower_bound, int64_t *late_rows,
                                  int64_t *sweeps);

/* TraceBounds val/key lower bound applied to one batch (operator/trace.rs
 * :463-607): out = the rows of `in` whose time is >= bound, in order (so a
 * consolidated batch stays consolidated).  mode 0: time = v (rows
 * (partition, ts, w)); mode 1: time = k & 0xffffffff (rows
 * (partition<<32 | ts, sum, w)); mode 2: time = v >> 32 (rows
 * (partition, ts << 32 | val, w), the low half of v ignored).  Device arrays
 * in and out; out is owned by the caller, null when empty. */
dbsp_status dbsp_truncate_below(dbsp_ctx *ctx, const dbsp_batch *in, int mode,
                                uint64_t bound, dbsp_batch *out);

/* ---- incremental top-K per group ----
 * SQL's ROW_NUMBER() OVER (PARTITION BY g ORDER BY x DESC) <= K, kept up to
 * date.  Replaces the aggregate(Fold) that keeps the last K values of a
 * key's cursor-ordered run in a VecDeque (pop_front at capacity, push_back)
 * and the flat_map behind it (crates/nexmark/src/queries/q19.rs).
 * Rows are (k, v, w).  A row's group is g = k >> group_shift; the low
 * group_shift bits of k, then all of v, order the rows inside a group, so
 * plain (k, v) order is (group, rank) order.  A row is PRESENT iff its total
 * weight in the input integral is non-zero, negative totals included
 * (Fold::aggregate steps on !weight.is_zero(), aggregate/fold.rs:83-92, once
 * per value whatever the weight).  The maintained relation holds, for every
 * group, its last min(K, present rows) present rows in (k, v) order, each
 * with weight +1.  So a weight change that keeps presence (1 -> 2) outputs
 * nothing, a row taken to net 0 vanishes, and a row at net -1 is present.
 * Out of scope: ascending order (q18's fold), a rank-number column,
 * watermark-bounded state, sharded ranks. */

/* The batch primitive (q19.rs's fold + flat_map over one consolidated
 * batch): the last <= K rows of every group of `in`, each with weight +1, in
 * order.  1 <= K <= 65536 and 0 <= group_shift <= 63, else DBSP_ERR_INVALID.
 * out: device arrays owned by the caller, null when empty; host visible on
 * return. */
dbsp_status dbsp_topk(dbsp_ctx *ctx, const dbsp_batch *in, int64_t K,
                      int group_shift, dbsp_batch *out);

/* The stateful operator (the aggregate operator under q19.rs's fold with its
 * input trace and its output trace, operator/aggregate/mod.rs:479-547): the
 * input integral and the integral of its own outputs, both as spines. */
typedef struct dbsp_topk_op dbsp_topk_op;
/* flags: every affected group recomputes its top-K from its whole run of the
 * input integral (the refill path), whether or not the tick could have
 * changed its membership that way.  A diagnostic and a test oracle: outputs
 * are the same either way. */
#define DBSP_TOPK_REFILL_ALL 1u
/* circuit construction of the aggregate (Stream::aggregate,
 * aggregate/mod.rs:204-250).  K and
 * group_shift as for dbsp_topk; an unknown flag bit is DBSP_ERR_INVALID. */
dbsp_status dbsp_topk_create(dbsp_ctx *ctx, int64_t K, int group_shift,
                             uint32_t flags, dbsp_topk_op **out);
/* AggregateIncremental::eval (aggregate/mod.rs:479-547) for this fold.
 * k/v/w: n raw (unsorted, unconsolidated) delta rows in device memory; any
 * (k, v) is valid.  out: the tick's consolidated change of the relation, rows
 * (k, v, +-1) (device arrays owned by the caller, null when empty; host
 * visible on return).  n == 0 and a delta that consolidates to nothing
 * change nothing and return an empty out.  Work per tick follows the delta:
 * only a group whose full top-K loses a member reads its run of the input
 * integral. */
dbsp_status dbsp_topk_step(dbsp_topk_op *op, const uint64_t *k,
                           const uint64_t *v, const int64_t *w, int64_t n,
                           dbsp_batch *out);
/* rows / spine batches of the two traces (Spine introspection,
 * trace/spine_fueled.rs:107-119) and cumulative counters: groups a delta
 * touched, groups sent down the refill path, rows the refill gather copied
 * out of the input trace.  Any out pointer may be null. */
dbsp_status dbsp_topk_stats(dbsp_topk_op *op, int64_t *in_rows,
                            int *in_batches, int64_t *out_rows,
                            int *out_batches, int64_t *groups_seen,
                            int64_t *groups_refilled, int64_t *rows_gathered);
dbsp_status dbsp_topk_destroy(dbsp_topk_op *op);

/* ---- incremental antijoin and semijoin ----
 * SQL's NOT EXISTS / NOT IN (antijoin) and EXISTS / IN (semijoin), kept up
 * to date; with dbsp_join_spine, the parts of LEFT / FULL OUTER JOIN.
 * Replaces Stream::antijoin (crates/dbsp/src/operator/join.rs:294-320), which
 * composes A - A |><| distinct(B) out of a distinct, a two-sided join and a
 * minus; here it is one operator over two traces.
 * Left rows are (k, v, w).  The right side is a KEY SET: keys (k, w), the
 * case I2::Val = ().  A key is PRESENT iff its total weight in the integral
 * of the right side is > 0, the distinct rule (operator/distinct.rs); a key
 * at net -1 is absent.
 *   DBSP_ANTIJOIN  A restricted to the keys absent from B: `antijoin`.
 *   DBSP_SEMIJOIN  A restricted to the keys present in B: A |><| distinct(B),
 *                  the term join.rs:313 subtracts.  It is NOT the reference's
 *                  semijoin_stream (operator/semijoin.rs:38-142), the
 *                  per-batch operator that multiplies a row's weight by its
 *                  key's weight: here a left row keeps its own weight.
 * Multi-valued right sides: the reference applies distinct() to the right
 * side's (key, value) PAIRS before its join, so a key with m distinct present
 * values yields weight w * (1 - m).  That follows from its composition, not
 * from SQL; it is not reproduced.  Callers project the right side to its
 * keys first, the case in which both agree.
 * Out of scope: the outer join itself (DESIGN.md says how it composes),
 * watermark-bounded state, sharded ranks. */
#define DBSP_ANTIJOIN 0
#define DBSP_SEMIJOIN 1

/* The batch primitive (join.rs:298-319 over one batch and one key set): the
 * rows of the consolidated batch `a` whose key is absent from (antijoin) or
 * present in (semijoin) the key set, in order, weights unchanged.  bk/bw: nb
 * sorted distinct keys in device memory with non-zero weights; a key of
 * negative weight is absent.  An unknown mode is DBSP_ERR_INVALID.  out:
 * device arrays owned by the caller, null when empty; host visible on
 * return. */
dbsp_status dbsp_antijoin(dbsp_ctx *ctx, const dbsp_batch *a,
                          const uint64_t *bk, const int64_t *bw, int64_t nb,
                          int mode, dbsp_batch *out);

/* The stateful operator (antijoin's distinct, join and minus with their three
 * traces, join.rs:298-319): the integrals of both sides, as spines. */
typedef struct dbsp_antijoin_op dbsp_antijoin_op;
/* circuit construction (Stream::antijoin, join.rs:294-297); the mode is fixed
 * here, an unknown one is DBSP_ERR_INVALID */
dbsp_status dbsp_antijoin_create(dbsp_ctx *ctx, int mode,
                                 dbsp_antijoin_op **out);
/* One tick of the composed circuit (distinct.rs:273 DistinctIncremental::eval,
 * JoinTrace::eval for both sides, and the minus).  ak/av/aw: na raw
 * (unsorted, unconsolidated) left rows, bk/bw: nb raw right keys, all in
 * device memory; either side may be empty (its pointers then unread); any
 * row and any key is valid.  out: the tick's consolidated change (device
 * arrays owned by the caller, null when empty; host visible on return).  Both
 * sides empty, or consolidating to nothing, change nothing and return an
 * empty out.  Work per tick follows the deltas: the left trace is read only
 * for keys whose presence FLIPS this tick, and a tick that flips no key
 * reads none of it. */
dbsp_status dbsp_antijoin_step(dbsp_antijoin_op *op, const uint64_t *ak,
                               const uint64_t *av, const int64_t *aw,
                               int64_t na, const uint64_t *bk,
                               const int64_t *bw, int64_t nb, dbsp_batch *out);
/* rows / spine batches of the two traces (Spine introspection,
 * trace/spine_fueled.rs:107-119) and cumulative counters: keys whose presence
 * flipped, rows of the left integral (consolidated) re-emitted under a flip,
 * delta rows the filter dropped.  Any out pointer may be null. */
dbsp_status dbsp_antijoin_stats(dbsp_antijoin_op *op, int64_t *a_rows,
                                int *a_batches, int64_t *b_rows,
                                int *b_batches, int64_t *keys_flipped,
                                int64_t *rows_gathered,
                                int64_t *rows_filtered);
dbsp_status dbsp_antijoin_destroy(dbsp_antijoin_op *op);

/* ---- incremental arg-max per group, ties kept ----
 * SQL's RANK() OVER (PARTITION BY g ORDER BY x DESC) = 1, or WHERE x =
 * (SELECT MAX(x) ...) per group, kept up to date.  Replaces the tail of
 * crates/nexmark/src/queries/q7.rs:82-93: aggregate(Min) over the negated
 * price, joined back to the rows on the price.
 * Rows are (k, v, w), with 0 <= rank_shift <= group_shift <= 63.  A row's
 * group is k >> group_shift and its rank k >> rank_shift: the rank includes
 * the group bits, so equal ranks imply one group and plain (k, v) order is
 * (group, rank, tie order) order.  A row is PRESENT iff its total weight in
 * the input integral is non-zero, negative totals included (top-K's rule).
 * The maintained relation holds, for every group that has a present row, all
 * present rows whose rank equals the group's largest present rank, EACH AT
 * ITS OWN INTEGRAL WEIGHT (the reference's join multiplies by the row's
 * weight).  So a tie row going from weight 1 to 2 outputs +1 for that row.
 * One divergence from the reference: Min::aggregate
 * (operator/aggregate/min.rs:38-57) sums the weights of all rows sharing a
 * price and skips a price whose sum is zero; here a rank stays present as
 * long as any single row at it is present.  The two agree on every relation
 * whose weights are positive (every Nexmark stream) and differ only when
 * different rows at one rank carry weights of mixed sign that cancel.
 * Out of scope: a Min direction, sharded ranks, watermark-bounded state. */

/* The batch primitive: the rows of the consolidated batch `in` whose rank is
 * their group's largest, weights unchanged, in order.  Invalid shifts
 * (negative, > 63, rank_shift > group_shift) are DBSP_ERR_INVALID.  out:
 * device arrays owned by the caller, null when empty; host visible on
 * return. */
dbsp_status dbsp_argmax(dbsp_ctx *ctx, const dbsp_batch *in, int group_shift,
                        int rank_shift, dbsp_batch *out);

/* The stateful operator: the input integral and the integral of its own
 * outputs, both as spines (the aggregate's input and output traces,
 * operator/aggregate/mod.rs:479-547). */
typedef struct dbsp_argmax_op dbsp_argmax_op;
/* flags: every affected group recomputes its tie set from its whole run of
 * the input integral (the refill path).  A diagnostic and a test oracle:
 * outputs are the same either way. */
#define DBSP_ARGMAX_REFILL_ALL 1u
/* shifts as for dbsp_argmax; an unknown flag bit is DBSP_ERR_INVALID */
dbsp_status dbsp_argmax_create(dbsp_ctx *ctx, int group_shift, int rank_shift,
                               uint32_t flags, dbsp_argmax_op **out);
/* k/v/w: n raw (unsorted, unconsolidated) delta rows in device memory; any
 * (k, v) is valid.  out: the tick's consolidated change of the relation
 * (device arrays owned by the caller, null when empty; host visible on
 * return).  n == 0 and a delta that consolidates to nothing change nothing
 * and return an empty out.  A group's run of the input integral is read (the
 * refill) iff the group had a present row before the tick and no present row
 * of at least its old largest rank remains after it: its maximum drops, or
 * it empties.  A stream on which no group's maximum ever decreases reads
 * nothing of the input integral. */
dbsp_status dbsp_argmax_step(dbsp_argmax_op *op, const uint64_t *k,
                             const uint64_t *v, const int64_t *w, int64_t n,
                             dbsp_batch *out);
/* as dbsp_topk_stats: rows / spine batches of the two traces and the
 * cumulative groups a delta touched, groups refilled and rows the refill
 * gather copied out of the input trace.  Any out pointer may be null. */
dbsp_status dbsp_argmax_stats(dbsp_argmax_op *op, int64_t *in_rows,
                              int *in_batches, int64_t *out_rows,
                              int *out_batches, int64_t *groups_seen,
                              int64_t *groups_refilled,
                              int64_t *rows_gathered);
dbsp_status dbsp_argmax_destroy(dbsp_argmax_op *op);

dbsp_status dbsp_agg_linear_upsert(dbsp_ctx *ctx,
                                   const uint64_t *delta_keys, int64_t nd,
                                   const dbsp_batch *in_trace,
                                   const dbsp_batch *out_trace,
                                   dbsp_batch *out_raw);

/* Max aggregate + upsert (reference operator/aggregate/max.rs:26-60). Same
 * contract as above but the new per-key value is the largest val whose total
 * weight in in_trace is non-zero (None if no such val). */
dbsp_status dbsp_agg_max_upsert(dbsp_ctx *ctx,
                                const uint64_t *delta_keys, int64_t nd,
                                const dbsp_batch *in_trace,
                                const dbsp_batch *out_trace,
                                dbsp_batch *out_raw);

/* q6's fold + upsert (queries/q6.rs:97-110 over aggregate/fold.rs:76-96).
 * Same contract as above; in_trace rows are (seller, auction<<27 | price).
 * The new per-key value is the floor average of the prices (low 27 bits of
 * the val) of the last <= 10 rows of the key's run; every row of a
 * consolidated trace counts, whatever the sign of its weight. */
dbsp_status dbsp_agg_last10_upsert(dbsp_ctx *ctx,
                                   const uint64_t *delta_keys, int64_t nd,
                                   const dbsp_batch *in_trace,
                                   const dbsp_batch *out_trace,
                                   dbsp_batch *out_raw);

/* The insert half of the linear aggregate over a spine, as the q5 tick runs
 * it: the distinct keys of the consolidated delta, per-key weight sums of
 * in_batches (0..24, sorted by k, passed verbatim) added batch by batch into
 * one zeroed accumulator, then (key, sum, +1) for every non-zero sum.
 * out_keys (device, caller frees; null when the delta is empty) and n_keys
 * receive the distinct keys; out_raw the emitted rows, in the order their
 * tickets were drawn (undefined: compare as a set).  Synchronous. */
dbsp_status dbsp_agg_sum_spine(dbsp_ctx *ctx, const dbsp_batch *delta,
                               const dbsp_batch *in_batches, int n_batches,
                               uint64_t **out_keys, int64_t *n_keys,
                               dbsp_batch *out_raw);

/* Where dbsp_wm_update's kernel takes the tick's max event time from: the
 * last of the first n sorted keys with n passed by value, the same with n
 * read from a device word, or an already reduced maximum (0 = none). */
typedef enum {
    DBSP_WM_HOST_N = 0,
    DBSP_WM_DEV_N  = 1,
    DBSP_WM_GMAX   = 2,
} dbsp_wm_source;

/* One step of the device watermark (queries/q5.rs:85-96, q8.rs:62-71) on
 * scratch device words.  state (host, in/out): {wm, s0, e0, have_prev}.
 * bounds (host, in/out): {s0, e0, s1, e1, have_prev, err}; what the caller
 * puts in is what the kernel finds there.  ak: ak_len sorted device keys; n is
 * the length the kernel sees (n > ak_len is DBSP_ERR_INVALID; a negative n
 * sets err = 1 and leaves every other word as it was).  DBSP_WM_GMAX ignores
 * ak and n and takes gmax.  wm = max(wm, max - lag) when the tick has a
 * maximum (precondition max >= lag), rounded = wm - wm % tumble, the new
 * window [rounded - width saturating at 0, rounded).  Synchronous. */
dbsp_status dbsp_wm_update(dbsp_ctx *ctx, uint64_t *state, uint64_t *bounds,
                           int source, const uint64_t *ak, int64_t ak_len,
                           int64_t n, uint64_t gmax, uint64_t width,
                           uint64_t tumble, uint64_t lag);

/* Route 2 of dbsp_window_spine: the watermark step the window bounds come
 * from.  state is in/out; wm_n is the tick batch's length as the watermark
 * kernel sees it and bn as the ranges kernel sees it, both through device
 * words (either above batch->len is DBSP_ERR_INVALID; negative ones are
 * passed on). */
typedef struct {
    uint64_t state[4];
    int64_t wm_n;
    int64_t bn;
    uint64_t width, tumble, lag;
} dbsp_window_chain;

/* The window stage over a whole spine, by the kernels the q5 / q8 ticks run.
 * trace_batches: n_batches (0..24) batches sorted by k, passed verbatim, an
 * empty batch keeping its three regions; batch: this tick's delta.
 * route 1: k_window_ranges_multi with the host bounds {s0, e0, s1, e1,
 * have_prev, -} (read).  route 2: k_wm_update on chain->state with the tick
 * batch's keys as its source, then the ranges launch reading the bounds and
 * the batch length from the device; bounds (written) receives what the
 * watermark published.  total: the row total, or the -1 verdict of an err
 * watermark or a negative bn (no table, no rows).  table_host receives the
 * (3 * n_batches + 1) * 5 region words [src, lo, len, sign, goff], regions per
 * batch in the order retract [s0, min(s1,e0)), shrink [e1, e0), insert
 * [max(e0,s1), e1), the tick batch's [s1, e1) last.  out_raw: the emitted
 * rows in table order.  A table that points outside its batches is
 * DBSP_ERR_INTERNAL and nothing is emitted.  Synchronous. */
dbsp_status dbsp_window_spine(dbsp_ctx *ctx, const dbsp_batch *trace_batches,
                              int n_batches, const dbsp_batch *batch,
                              int route, uint64_t *bounds,
                              dbsp_window_chain *chain, int64_t *total,
                              int64_t *table_host, dbsp_batch *out_raw);

/* Window operator: 3-region retract/insert range scan over a time-keyed trace.
 * Replaces Window::eval (operator/time_series/window.rs:144-220).
 * trace = integral of the stream up to but NOT including this tick;
 * batch = this tick's delta;  (s0,e0) = previous window (s0=e0=0, have_prev=0 on
 * the first tick);  (s1,e1) = new bounds.  Output raw rows. */
dbsp_status dbsp_window(dbsp_ctx *ctx, const dbsp_batch *trace,
                        const dbsp_batch *batch,
                        int have_prev, uint64_t s0, uint64_t e0,
                        uint64_t s1, uint64_t e1,
                        dbsp_batch *out_raw);

/* Key partitioning for the worker exchange.
 * Replaces shard_batch (operator/communication/shard.rs:165-199) with the hash
 * of hash.rs:9-13 (xxh3_64 with seed 0x7f95_ef85_be33_c337 over the 8 key
 * bytes).  Rows of `in` are stably scattered into nshards contiguous runs of
 * `out` by xxh3(k) % nshards; host-visible shard offsets written to
 * offsets_host[nshards+1] after sync.  The exchange itself (reference
 * exchange.rs:45-251, an N^2 mailbox) is an RCCL grouped send/recv over xGMI —
 * see dbsp_comm_* below. */
dbsp_status dbsp_shard_partition(dbsp_ctx *ctx, const dbsp_batch *in,
                                 int nshards, dbsp_batch *out,
                                 int64_t *offsets_host);

/* ---- f64-weight variants (config C5: the f64 sum aggregate path).
 * Weights travel in the same 8-byte column as f64 bit patterns.  All f64
 * reductions use a position-fixed order (segmented tree / batch order);
 * documented tolerance vs a sequential sum: |err| <= 2 ulp * reduction depth
 * (SURVEY.md §8d).  Zero-weight elimination follows the reference's F64
 * is_zero (== 0.0, so -0.0 is eliminated; algebra/floats.rs:24). */
dbsp_status dbsp_sort_consolidate_f64(dbsp_ctx *ctx, const uint64_t *k_in,
                                      const uint64_t *v_in, const double *w_in,
                                      int64_t n, dbsp_batch *out);
/* dbsp_merge with f64 weights: the same three size bands and kernels as the
 * C5 spine's merges; a poisoned length returns DBSP_ERR_INTERNAL. */
dbsp_status dbsp_merge_f64(dbsp_ctx *ctx, const dbsp_batch *a,
                           const dbsp_batch *b, dbsp_batch *out);
/* weigh (aggregate/mod.rs:297-323) with f(k, v) = f64_from_bits(v):
 * (k, v, w) -> raw rows (k, (), f64(v) * w); caller consolidates. */
dbsp_status dbsp_weigh_f64(dbsp_ctx *ctx, const dbsp_batch *in,
                           dbsp_batch *out_raw);
/* linear aggregate over an f64-weighted input trace + upsert against an
 * i64-weighted output trace whose values are f64 bit patterns. */
dbsp_status dbsp_agg_linear_upsert_f64(dbsp_ctx *ctx,
                                       const uint64_t *delta_keys, int64_t nd,
                                       const dbsp_batch *in_trace,
                                       const dbsp_batch *out_trace,
                                       dbsp_batch *out_raw);

/* Incremental distinct (operator/distinct.rs:273: DistinctIncremental at
 * root scope): for each delta pair, out = [w_before + dw > 0] - [w_before > 0]
 * where w_before is the pair's total weight in the delayed integral (passed
 * as its spine batches: distinct is NOT linear in the trace).  The output is
 * consolidated by construction.  Unlocks Nexmark q4/q6/q9 (SURVEY.md
 * §8f.2); the antijoin has an operator of its own, dbsp_antijoin_step, which
 * applies this rule to a key set. */
dbsp_status dbsp_distinct_inc(dbsp_ctx *ctx, const dbsp_batch *delta,
                              const dbsp_batch *trace_batches, int n_batches,
                              dbsp_batch *out);

/* Distinct keys of a consolidated batch (device out, caller frees). */
dbsp_status dbsp_unique_keys(dbsp_ctx *ctx, const dbsp_batch *in,
                             uint64_t **out_keys, int64_t *n_out);

/* Reference hash (host-callable too, for tests): xxh3_64(le_bytes(key), seed). */
uint64_t dbsp_xxh3_u64(uint64_t key, uint64_t seed);

/* ---- RCCL exchange over xGMI (replaces exchange.rs:45-251) ---- */
/* nccl_id is the 128-byte ncclUniqueId obtained by rank 0 and distributed
 * out-of-band (e.g. torch.distributed broadcast). */
dbsp_status dbsp_comm_init(dbsp_ctx *ctx, int rank, int world,
                           const void *nccl_id /* 128 bytes */);
/* All-to-all-v of row columns: send_counts[world] rows from `send` (contiguous
 * runs in shard order, as produced by dbsp_shard_partition); receives into
 * `recv` (capacity recv_cap rows); recv_counts_host[world] written after sync. */
dbsp_status dbsp_comm_alltoallv(dbsp_ctx *ctx, const dbsp_batch *send,
                                const int64_t *send_counts,
                                dbsp_batch *recv, int64_t recv_cap,
                                int64_t *recv_counts_host);

/* ======================================================================
 * Engine-level entry points (host-side mirror of the Circuit/Stream API;
 * see engine.cpp for the operator-by-operator mapping)
 * ====================================================================== */

typedef struct dbsp_engine dbsp_engine;

/* query: 0, 3, 5, 8 (Nexmark — the same operator DAG as
 * crates/nexmark/src/queries/q{0,3,5,8}.rs over the mirrored API), or 100
 * (config C5: the synthetic 1B-row OrdIndexedZSet x 10M-row delta
 * incremental join + f64 sum aggregate of BASELINE configs[4]), or 101
 * (per-auction rolling bid volume:
 *  bids.map_index(|b| (b.auction, (b.date_time, b.price)))
 *      .partitioned_rolling_aggregate_linear(...),
 *  operator/time_series/rolling_aggregate.rs:367-419 over the Nexmark bid
 *  stream; output rows (auction<<32 | date_time, sum of prices, +-1)), or
 * 102 (per-auction rolling highest bid: the same map_index into
 *      .partitioned_rolling_aggregate(Max, range),
 *  rolling_aggregate.rs:235-321; input rows (auction, date_time<<32 | price,
 *  w), output rows (auction<<32 | date_time, highest price, +-1); a bid
 *  whose date_time or price is >= 2^32 makes the step DBSP_ERR_INVALID with
 *  the state unchanged), or
 * 19 (Nexmark q19, the top K bids of every auction, queries/q19.rs:40-57:
 *      bids.flat_map_index(|b| (b.auction, (b.price, b))) into the top-K
 *  operator above; rows k = auction << 27 | price, v = bidder << 32 |
 *  date_time, group_shift 27, so the group is the auction and the order
 *  inside it (price, bidder, date_time): the reference's (price, Bid) order
 *  restricted to the fields dbsp_event carries (channel, url and extra are
 *  not in the event row).  Output rows are input rows, +-1.  A bid with
 *  auction >= 2^37, price >= 2^27, bidder >= 2^32 or date_time >= 2^32 makes
 *  the step DBSP_ERR_INVALID, detected on the device, with the state
 *  unchanged; the next tick is unaffected.  world > 1 is DBSP_ERR_INVALID at
 *  create: the exchange hashes k, which would split a group across ranks), or
 * 103 (auctions nobody has bid on yet:
 *      auctions.map_index(|a| (a.id, a.seller))
 *          .antijoin(&bids.map_index(|b| (b.auction, ())))
 *  Stream::antijoin, join.rs:294-320, on the antijoin operator above; rows
 *  (auction id, seller, w), output rows are input rows, signed.  world > 1
 *  is DBSP_ERR_INVALID at create: sharding by k would be correct, but no
 *  multi-rank run of it has been made), or
 * 7 (Nexmark q7, the highest bids of the last tumbled window, queries/q7.rs:
 *  45-94: bids by date_time, watermark_monotonic(date_time - 4000) rounded
 *  down to 10000, the window [rounded saturating-minus 10000, rounded), and
 *  the arg-max operator above over rows k = price << 32 | date_time,
 *  v = auction << 32 | bidder with group_shift 59 and rank_shift 32: one
 *  group, ranked by price.  Output rows are those rows at the bids' weights,
 *  signed.  A tick's largest date_time must be >= 4000, as for query 5.  A
 *  bid with date_time >= 2^32, price >= 2^27, auction >= 2^32 or bidder >=
 *  2^32 makes the step DBSP_ERR_INVALID, detected on the device, with the
 *  state unchanged; the next tick is unaffected.  world > 1 is
 *  DBSP_ERR_INVALID at create: one group cannot be split across ranks.  The
 *  bid-by-time trace is not trimmed.  channel, url and extra are not in the
 *  event row). */
dbsp_status dbsp_engine_create(dbsp_engine **out, dbsp_ctx *ctx, int query,
                               int rank, int world);

/* Query 101 / 102 range: [date_time - before_ms, date_time + after_ms]
 * (RelRange, range.rs:93-104).  Defaults 10000 / 0.  DBSP_ERR_INVALID on
 * another query or after the engine's first step. */
dbsp_status dbsp_engine_rolling_init(dbsp_engine *e, uint64_t before_ms,
                                     uint64_t after_ms);
/* watermark_monotonic(|ts| ts.saturating_sub(lateness_ms)) over the bid stream
 * (watermark.rs:33-75) feeding partitioned_rolling_aggregate_with_watermark
 * (rolling_aggregate.rs:155-220): per tick the watermark is the largest bid
 * time seen so far, this tick's rows included, minus lateness_ms, and the
 * step is dbsp_rolling_step_wm (query 102: the bid time is v >> 32).
 * Sharded ranks use their rank-local maximum
 * (no collective).  Off by default; DBSP_ERR_INVALID on another query or
 * after the first step. */
dbsp_status dbsp_engine_rolling_lateness(dbsp_engine *e, uint64_t lateness_ms);
/* Query 102's aggregator (aggregate/max.rs:36-55, min.rs:38-57):
 * DBSP_ROLL_MAX (the default) or DBSP_ROLL_MIN.  DBSP_ERR_INVALID on another
 * query, another aggregator or after the first step. */
dbsp_status dbsp_engine_rolling_agg(dbsp_engine *e, dbsp_roll_agg agg);
/* query 101 / 102 trace rows and watermark counters (Spine introspection,
 * trace/spine_fueled.rs:107-119); any out pointer may be null */
dbsp_status dbsp_engine_rolling_stats(dbsp_engine *e, int64_t *in_rows,
                                      int64_t *out_rows, int64_t *late_rows,
                                      int64_t *sweeps);
/* Query 19's K (q19.rs:38 TOP_BIDS; default 10, 1..65536).
 * DBSP_ERR_INVALID on another query or after the engine's first step. */
dbsp_status dbsp_engine_topk_init(dbsp_engine *e, int64_t K);
/* query 19 trace rows and the operator's cumulative counters (as
 * dbsp_topk_stats); any out pointer may be null */
dbsp_status dbsp_engine_topk_stats(dbsp_engine *e, int64_t *in_rows,
                                   int64_t *out_rows, int64_t *groups_seen,
                                   int64_t *groups_refilled,
                                   int64_t *rows_gathered);
/* query 103 trace rows and the operator's cumulative counters (as
 * dbsp_antijoin_stats); any out pointer may be null */
dbsp_status dbsp_engine_antijoin_stats(dbsp_engine *e, int64_t *a_rows,
                                       int64_t *b_rows, int64_t *keys_flipped,
                                       int64_t *rows_gathered,
                                       int64_t *rows_filtered);
/* query 7 trace rows of the arg-max operator and its cumulative counters
 * (as dbsp_argmax_stats); any out pointer may be null */
dbsp_status dbsp_engine_argmax_stats(dbsp_engine *e, int64_t *in_rows,
                                     int64_t *out_rows, int64_t *groups_seen,
                                     int64_t *groups_refilled,
                                     int64_t *rows_gathered);
dbsp_status dbsp_engine_destroy(dbsp_engine *e);

/* C5 (query 100) setup: device-generates the n_trace-row (k, f64-bits, +1)
 * indexed trace (counter-based splitmix64; sorted-unique by construction)
 * and fixes the per-tick delta size.  After this, step ranges index delta
 * ROWS: dbsp_engine_run_staged(e, 0, steps*n_delta, n_delta) runs `steps`
 * ticks, each one a fresh device-generated n_delta-row delta joined and
 * aggregated incrementally (operator mapping in the engine source). */
dbsp_status dbsp_engine_c5_init(dbsp_engine *e, int64_t n_trace,
                                int64_t n_delta, uint64_t seed);

/* One clock tick: ingest `events` (host array, this tick's input delta) and run
 * every operator once in dependency order — the mirror of DBSPHandle::step
 * (circuit/dbsp_handle.rs:246) + the static scheduler (circuit/schedule/).
 * The tick's output delta is retained on device; fetch with
 * dbsp_engine_output. */
dbsp_status dbsp_engine_step(dbsp_engine *e, const dbsp_event *events, int64_t n);

/* Events may instead be pre-staged to HBM once (bench: inputs resident before
 * the timed region) and stepped by index range. */
dbsp_status dbsp_engine_stage_events(dbsp_engine *e, const dbsp_event *events,
                                     int64_t n);
dbsp_status dbsp_engine_step_staged(dbsp_engine *e, int64_t lo, int64_t hi);
/* Run staged events [lo,hi) in tick-sized steps inside one call (the
 * benchmark loop; per-tick outputs are produced and replaced in turn —
 * read dbsp_engine_output afterwards for the LAST tick only). */
dbsp_status dbsp_engine_run_staged(dbsp_engine *e, int64_t lo, int64_t hi,
                                   int64_t tick);

/* Copy last tick's output delta to host rows; returns count via *n_out
 * (capacity cap rows; DBSP_ERR_OVERFLOW if larger). For q0 the output rows are
 * the consolidated event zset re-packed as (hi,lo,w) row pairs per event
 * (see engine.cpp q0 notes). */
dbsp_status dbsp_engine_output(dbsp_engine *e, dbsp_row *out, int64_t cap,
                               int64_t *n_out);

/* Perf counters for the roofline leg: total device ns and bytes of the
 * dominant kernel class since engine creation (measured with hipEvents on the
 * engine's own stream). kind: 0=merge/consolidate sort passes, 1=merge-path,
 * 2=join, 3=aggregate, 4=window, 5=everything-else. */
dbsp_status dbsp_engine_kernel_stats(dbsp_engine *e, int kind,
                                     double *total_ms, double *algo_bytes,
                                     int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* DBSP_HIP_H */
