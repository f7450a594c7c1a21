// kernels_iface.hpp — internal interface between kernels.hip (device code)
// and engine.cpp (host-side Circuit/Stream mirror).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dbsp_hip.h"

// spine-as-kernel-argument descriptor (multi-batch join/probe kernels)
#define MAX_TRACE_BATCHES 24
struct TraceArgs {
    int nb;
    const uint64_t *k[MAX_TRACE_BATCHES];
    const uint64_t *v[MAX_TRACE_BATCHES];
    const int64_t *w[MAX_TRACE_BATCHES];
    int64_t n[MAX_TRACE_BATCHES];
};

#define SORT_BATCH_MAX 8
struct SortArgs {
    int nb;
    const uint64_t *kin[SORT_BATCH_MAX];
    const uint64_t *vin[SORT_BATCH_MAX];
    const int64_t *win[SORT_BATCH_MAX];
    int64_t n[SORT_BATCH_MAX];
    uint64_t *tk[SORT_BATCH_MAX];
    uint64_t *tv[SORT_BATCH_MAX];
    int64_t *tw[SORT_BATCH_MAX];
    uint64_t *ok[SORT_BATCH_MAX];
    uint64_t *ov[SORT_BATCH_MAX];
    int64_t *ow[SORT_BATCH_MAX];
    int64_t *d_len;  // device array, one length per batch
    // optional per-batch DEVICE length (overrides n[b]): lets the sort launch
    // chain behind the producing kernel without a host sync.  If the device
    // length exceeds the fused capacity the kernel writes out_len = -1 and
    // the host re-sorts through the sized paths after its next sync.
    const int64_t *n_dev[SORT_BATCH_MAX];
    // optional per-batch TAKE (overrides n[b] and n_dev[b]): the length is
    // read from the producer's device counter n_take[b], which the sort block
    // hands back ZEROED for the producer's next run; the length it saw is
    // stored to n_seen[b] (a readback slot).  n_cap[b] is the number of input
    // rows that may be read: a counter above it (or above the fused capacity)
    // writes out_len = -1 and sorts nothing.
    int64_t *n_take[SORT_BATCH_MAX];
    int64_t *n_seen[SORT_BATCH_MAX];
    int64_t n_cap[SORT_BATCH_MAX];
};

// batched single-workgroup merges (one pair per workgroup; each na+nb <= 32768)
#define MERGE_BATCH_MAX 4
struct MergeArgs {
    int np;
    const uint64_t *ak[MERGE_BATCH_MAX];
    const uint64_t *av[MERGE_BATCH_MAX];
    const int64_t *aw[MERGE_BATCH_MAX];
    int64_t na[MERGE_BATCH_MAX];
    const uint64_t *bk[MERGE_BATCH_MAX];
    const uint64_t *bv[MERGE_BATCH_MAX];
    const int64_t *bw[MERGE_BATCH_MAX];
    int64_t nb[MERGE_BATCH_MAX];
    // optional device-side b length (the in-train accumulator merge: b is the
    // tick's delta, whose consolidated length lives in a d_len slot); null =>
    // use nb.  A negative device length (failed speculation) => emit -1.
    const int64_t *dnb[MERGE_BATCH_MAX];
    // acc_fold_batch with dnb only: rows of b that may be read; the output
    // columns hold na + bcap rows.  A device length above it emits -1.
    int64_t bcap[MERGE_BATCH_MAX];
    uint64_t *ok[MERGE_BATCH_MAX];
    uint64_t *ov[MERGE_BATCH_MAX];
    int64_t *ow[MERGE_BATCH_MAX];
    int64_t *d_len;
};

// join-tail descriptor: per-plan scan + capacity check + emit into the
// capacity buffer (e*) + sort/consolidate through the scratch (t*) into the
// output store (o*, >= 8192 rows), all in one single-workgroup launch behind
// a probe that kept the start positions.  See k_join_tail_small.
struct JoinTailArgs {
    int np;
    const uint64_t *dk[3], *dv[3];
    const int64_t *dw[3];
    const int64_t *nd_dev[3];
    TraceArgs t[3];
    const int64_t *tn_dev[3];
    const uint32_t *cnts[3];
    const int64_t *starts[3];
    uint64_t *offsets[3];  // out: per-row exclusive offsets (explicit replay)
    int proj[3];
    int64_t *totals;   // out: per-plan row totals (-1: negative length)
    int64_t cap;       // rows of the capacity buffer
    int64_t *d_total;  // out: combined total (or -1)
    int64_t *d_flag;   // out: nonzero = capacity buffer unusable
    int64_t *d_final;  // out: consolidated length (or -1)
    uint64_t *ek, *ev;
    int64_t *ew;
    uint64_t *tk, *tv;
    int64_t *tw;
    uint64_t *ok, *ov;
    int64_t *ow;
};
struct JoinCountArgs {
    int np;
    const uint64_t *dk[3];
    int64_t nd[3];
    TraceArgs t[3];
    uint32_t *cnts[3];
    uint64_t *offsets[3];
    int64_t *d_total;
    // optional device lengths: nd_dev overrides nd (the delta length), and
    // tn_dev overrides t.n[0] for single-batch traces that are themselves
    // tick-fresh deltas.  Negative device lengths (speculative-sort overflow)
    // make the plan write d_total = -1 for the host to detect at its sync.
    const int64_t *nd_dev[3];
    const int64_t *tn_dev[3];
    // optional: the probe also keeps each (row, batch) run's first position,
    // starts[i*nb+b] next to cnts[i*nb+b] (int64: exact for any batch length)
    int64_t *starts[3];
};

// where the device watermark takes the tick's max event time from
struct WmSource {
    const uint64_t *ak;  // sorted time keys of the tick's delta: the last one
    int64_t n;           // ... of n rows,
    const int64_t *n_dev;  // or of *n_dev if set (negative: bounds err = 1,
                           // state untouched)
    const unsigned long long *gmax_dev;  // if set, overrides all the above: an
                                         // already reduced maximum (0 = none)
};

namespace dbspk {
// big-buffer free-list over hipMallocAsync (see kernels.hip): same signature
// shape as hipMallocAsync/hipFreeAsync so call sites stay HIP_CHECK-able
hipError_t cache_malloc(void **out, size_t bytes, hipStream_t s);
hipError_t cache_free(void *p, hipStream_t s);
void cache_trim(hipStream_t s);
// scope the tick-scale (64 KB..4 MB) free-list band: trace-scale engines
// turn it off at init (see the definition for the measured pool interaction)
void cache_small_set(bool on, hipStream_t s);

// A row batch: three device columns of n rows.  f64 weights travel in w as
// their bit patterns.  The engine's DevBatch is this type.
struct Rows {
    uint64_t *k = nullptr, *v = nullptr;
    int64_t *w = nullptr;
    int64_t n = 0;
};

// Conventions below: `const Rows &` inputs are read (n rows); `Rows *out`
// receives FRESH columns from the big-buffer cache (null when empty) and
// their length; a `const Rows &` destination names caller-provided columns,
// and its comment says whether n is read or ignored.  `bool wf64` selects the
// f64-weight instantiation (config C5: deterministic position-fixed
// reduction order, tolerance 2 ulp * reduction depth), as Spine::wf64 does.

dbsp_status scan_excl(hipStream_t s, const uint64_t *in, uint64_t *out,
                      int64_t n, uint64_t *h_total);
void fill_u64(hipStream_t s, uint64_t *p, uint64_t v, int64_t n);

// sort rows by (k major, v minor), ping-ponging between rows and scratch
// (both written; scratch must hold rows.n rows, its n is ignored)
dbsp_status sort_rows(hipStream_t s, const Rows &rows, const Rows &scratch,
                      bool *result_in_scratch);

// consolidate SORTED rows.  The f64 path reduces in place: it OVERWRITES
// in.w (the const covers the descriptor, not the columns).
dbsp_status consolidate_sorted(hipStream_t s, const Rows &in, bool wf64,
                               Rows *out);

dbsp_status merge_rows(hipStream_t s, const Rows &a, const Rows &b, bool wf64,
                       Rows *out);

// device watermark: advance state = {wm, s0, e0, have_prev} by the tick's max
// event time and publish bounds = {s0, e0, s1, e1, have_prev, err} (no sync)
dbsp_status wm_update(hipStream_t s, const WmSource &src, uint64_t width,
                      uint64_t tumble, uint64_t lag, unsigned long long *state,
                      unsigned long long *bounds);
// ranges launch behind wm_update: the bounds are read from the device, and the
// tick batch's length from *bn_dev when it is given (else bn).  err bounds or
// a negative device length leave *d_total = -1.
dbsp_status window_ranges_chain(hipStream_t s, const TraceArgs &t,
                                const uint64_t *bk, int64_t bn,
                                const int64_t *bn_dev,
                                const unsigned long long *bounds,
                                int64_t *table, int64_t *d_total);
// min/max of k and v with the length read from n_dev (rows.n is the capacity
// that sizes the grid); results left in mm_dev[0..3], no sync
dbsp_status minmax_rows_chain(hipStream_t s, const Rows &rows,
                              const int64_t *n_dev,
                              unsigned long long *mm_dev);
// hash-partition two batches with one readback; out0/out1 hold in0.n/in1.n
// rows (their n is ignored)
dbsp_status shard_rows_pair(hipStream_t s, const Rows &in0, const Rows &in1,
                            int nshards, const Rows &out0, const Rows &out1,
                            int64_t *h_off0, int64_t *h_off1);
// device event columns (the §8f3 columnizer, input.rs:591-721): staged
// events split once into SoA columns so the per-tick flatmaps read
// coalesced 8 B streams instead of 56 B strided AoS structs
struct EventCols {
    const uint64_t *kind, *f0, *f1, *f2, *f3, *f4;
    const int64_t *w;
};
dbsp_status columnize_events(hipStream_t s, const dbsp_event *ev, int64_t n,
                             uint64_t *kind, uint64_t *f0, uint64_t *f1,
                             uint64_t *f2, uint64_t *f3, uint64_t *f4,
                             int64_t *w);
// out0/out1: capacity columns, n = their capacity in rows (a row whose ticket
// is at or past it is counted but not stored); lengths land in ctr[0..1]
// (device).  ctr_zero: the caller knows both counters hold 0 already (a
// taking sort handed them back, see SortArgs::n_take), so no memset is queued.
dbsp_status flatmap_events_chain(hipStream_t s, const dbsp_event *ev,
                                 const EventCols *cols, int64_t n, int query,
                                 const Rows &out0, const Rows &out1,
                                 uint64_t *ctr, bool ctr_zero = false);

// fixed-frame pair exchange (engine exchange fast path): both partitioned
// streams packed into per-peer segments of fixed capacity P0/P1 rows with a
// 2-word count header, so ONE equal-count ncclAllToAll replaces the
// counts-allgather + host sync + grouped send/recv mesh.  Segment layout
// (u64 words): [cnt0, cnt1, k0(P0), v0(P0), w0(P0), k1(P1), v1(P1), w1(P1)].
// A count above its capacity travels in the header as-is; the unpack kernel
// then writes -1 totals (sentinel) and the engine replays the exchange
// through the dynamic alltoallv path on every rank.
struct FramePairArgs {
    const uint64_t *p0k, *p0v;
    const int64_t *p0w;
    const uint64_t *p1k, *p1v;
    const int64_t *p1w;
    int64_t off0[9], off1[9];  // host partition offsets (nshards <= 8)
    int world;
    int64_t P0, P1;
    uint64_t *frame;
};
dbsp_status frames_pack_pair(hipStream_t s, const FramePairArgs &a);
// chained variant: hash-partition both RAW streams straight into the frames
// (lengths read from device counters, in0.n/in1.n ignored; n_cap bounds the
// launch grid)
dbsp_status shard_frames_chain(hipStream_t s, const Rows &in0,
                               const int64_t *n0_dev, const Rows &in1,
                               const int64_t *n1_dev, int world, int64_t P0,
                               int64_t P1, int64_t n_cap, uint64_t *frame);
// r0/r1: capacity columns (n ignored); totals land in d_tot0/d_tot1 (device)
dbsp_status frames_unpack_pair(hipStream_t s, const uint64_t *frame,
                               int world, int64_t P0, int64_t P1,
                               const Rows &r0, const Rows &r1,
                               int64_t *d_tot0, int64_t *d_tot1);
// fused single-workgroup sort+consolidate: up to SORT_BATCH_MAX (8)
// independent small (n <= 8192) raw batches sorted+consolidated concurrently,
// one workgroup each, lengths left in d_len[i] (device)
dbsp_status sort_cons_small_batch(hipStream_t s, const SortArgs &args,
                                  bool wf64);
// min/max of k and v (one sync): mm = {kmin, vmin, kmax, vmax}
dbsp_status minmax_rows(hipStream_t s, const Rows &rows, uint64_t mm[4]);
// dense-range consolidate: weights scattered into a kspan*vspan histogram,
// nonzero cells emitted in index order (sorted); i64 only.  out names
// caller-provided columns of in.n rows; its n is WRITTEN (one sync).
dbsp_status sort_cons_dense(hipStream_t s, const Rows &in, uint64_t kbase,
                            uint64_t vbase, int64_t kspan, int64_t vspan,
                            Rows *out);
// chained dense consolidate: length to *out_n_dev, no sync (out.n ignored)
dbsp_status sort_cons_dense_chain(hipStream_t s, const Rows &in,
                                  uint64_t kbase, uint64_t vbase,
                                  int64_t kspan, int64_t vspan,
                                  const Rows &out, int64_t *out_n_dev);

// single-workgroup merges of up to MERGE_BATCH_MAX pairs of consolidated
// batches (each na+nb <= 32768; the spine merges keep it for pairs <= 4096
// and send larger ones to merge_mid_batch): one launch, no host sync; lengths
// left in d_len[p] (device)
dbsp_status merge_small_batch(hipStream_t s, const MergeArgs &args, bool wf64);
// fixed-grid multi-WG merge with optional device-side b lengths (in-train
// accumulator fold); scratch holds np * (MERGE_MID_SCRATCH) int64 slots
#define MERGE_MID_SCRATCH 33
dbsp_status merge_mid_batch(hipStream_t s, const MergeArgs &args,
                            int64_t *scratch, bool wf64);

// accumulator fold: a (consolidated, na known on the host) plus b (a
// consolidated delta of at most 8192 rows whose length is read from dnb[p],
// or nb[p] when dnb[p] is null) for up to MERGE_BATCH_MAX pairs in one launch.
// Every workgroup classifies all of b against a and emits its own slice of a
// with the b rows that land in it: no count pass, no scratch, nothing passes
// between workgroups.  Lengths are left in d_len[p]; a negative or oversized
// device length gives -1.  Pair p runs on acc_fold_wgs(na[p]) workgroups of
// ceil(na / wgs) consecutive a rows each; b rows past the end of a go to the
// last one.
#define ACC_FOLD_SLICE 1024  // a workgroup's slice is at most this many rows
#define ACC_FOLD_WGS_MAX 64  // ... until na exceeds 64 * 1024
#define ACC_FOLD_NA_MAX ((int64_t)1 << 30)
__host__ __device__ static inline int acc_fold_wgs(int64_t na) {
    const int64_t g = (na + ACC_FOLD_SLICE - 1) / ACC_FOLD_SLICE;
    return (int)(g < 1 ? 1 : g > ACC_FOLD_WGS_MAX ? ACC_FOLD_WGS_MAX : g);
}
dbsp_status acc_fold_batch(hipStream_t s, const MergeArgs &args, bool wf64);

// The small-join scan and the tail sum matches in 32 bits, so a plan set's
// combined matches must stay below 2^32.
// the probe phase of a join over up to 3 plans (nd <= 8192 each): per-plan
// per-row/per-batch cnts and, if asked, start positions; no scan
dbsp_status join_probe_batch(hipStream_t s, const JoinCountArgs &args);
// the probe plus the single-workgroup scan, two launches: exclusive offsets,
// totals to d_total[i] (device)
dbsp_status join_count_scan_batch(hipStream_t s, const JoinCountArgs &args);
// the single-workgroup tail that consumes a probe which kept the starts
dbsp_status join_tail_small(hipStream_t s, const JoinTailArgs &a);
// emit phase over precomputed cnts/offsets into out (n_out rows; out.n
// ignored)
dbsp_status join_emit_prepared(hipStream_t s, const Rows &delta,
                               const TraceArgs &t, const uint32_t *cnts,
                               const uint64_t *offsets, int64_t n_out,
                               int proj, uint64_t param, const Rows &out);

// join delta against a whole spine (TraceArgs) in one count/emit pair
dbsp_status join_spine_rows(hipStream_t s, const Rows &delta,
                            const TraceArgs &t, int proj, uint64_t param,
                            Rows *out);

dbsp_status join_rows(hipStream_t s, const Rows &delta, const Rows &trace,
                      int proj, uint64_t param, Rows *out);

// incremental distinct over a whole spine (non-linear: the per-pair total
// must be summed across batches before the indicator)
dbsp_status distinct_inc_rows(hipStream_t s, const Rows &delta,
                              const TraceArgs &t, Rows *out);

// aggregate + upsert of the delta keys over the input trace `in`, retracting
// against the output trace `out_trace`.  AGG_LAST10 is q6's fold: avg of the
// last <= 10 vals in the key's run (cursor order).
enum AggMode { AGG_LINEAR = 0, AGG_MAX = 1, AGG_LAST10 = 2 };
dbsp_status agg_upsert_rows(hipStream_t s, AggMode mode, const uint64_t *keys,
                            int64_t nd, const Rows &in, const Rows &out_trace,
                            Rows *out);

// multi-batch linear aggregate: accumulate per-delta-key weight sums of one
// trace batch into acc[nd] (aggregation is linear in the trace, so spines are
// summed batch by batch); f64 sums run in batch-position order
dbsp_status agg_sum_batch(hipStream_t s, const uint64_t *keys, int64_t nd,
                          const Rows &in, int64_t *acc, bool wf64);
// emit (key, acc, +1) for acc != 0 into out's caller-provided columns of nd
// rows (ticket append; caller consolidates); out->n is WRITTEN (one sync).
// f64: v holds the sum's bit pattern.
dbsp_status emit_nonzero(hipStream_t s, const uint64_t *keys,
                         const int64_t *acc, int64_t nd, bool wf64, Rows *out);

// multi-batch window: ranges for all spine batches + tick batch in one launch
// (region table rows [src,lo,len,sign,goff]; total left in *d_total), then one
// grid-stride emit into out (total rows; out.n and batch.n ignored)
dbsp_status window_ranges_multi(hipStream_t s, const TraceArgs &t,
                                const uint64_t *bk, int64_t bn, int have_prev,
                                uint64_t s0, uint64_t e0, uint64_t s1,
                                uint64_t e1, int64_t *table, int64_t *d_total);
dbsp_status window_emit_multi(hipStream_t s, const TraceArgs &t,
                              const Rows &batch, const int64_t *table,
                              int nreg, int64_t total, const Rows &out);

// out holds in.n rows (its n is ignored)
dbsp_status shard_rows(hipStream_t s, const Rows &in, int nshards,
                       const Rows &out, int64_t *h_offsets);

// out0/out1 name caller-provided capacity columns; their n is WRITTEN (one
// sync)
dbsp_status flatmap_events(hipStream_t s, const dbsp_event *ev,
                           const EventCols *cols, int64_t n, int query,
                           Rows *out0, Rows *out1);

// out holds in.n rows (its n is ignored)
dbsp_status map_rows(hipStream_t s, const Rows &in, int mode, const Rows &out);

// distinct keys of a consolidated (sorted) batch
dbsp_status unique_keys(hipStream_t s, const uint64_t *kk, int64_t n,
                        uint64_t **okeys, int64_t *out_n);

// C5 synthetic operands: out.n (read) sorted-unique rows by construction
// (k_i = stride*i + h(i)%jitter, jitter < stride; val_mode 0 = uniform f64
// bits, 1 = zero)
dbsp_status c5_gen_rows(hipStream_t s, const Rows &out, uint64_t stride,
                        uint64_t jitter, uint64_t seed, int val_mode);

// radix-tree rolling aggregate (§8f4): per input row (partition, ts, w),
// the weight sum over the partition's rows with time in [ts-width, ts];
// out holds in.n rows (its n is ignored)
dbsp_status rolling_agg_rows(hipStream_t s, const Rows &in, uint64_t width,
                             const Rows &out);

// ---- incremental partitioned rolling aggregate (rolling_aggregate.rs
// :487-604); times and partitions < 2^32, ranges saturate at 0 / 2^32-1 ----
// Merged run lists of a consolidated (p, ts)-sorted delta (weights unread).
// *ranges is one 6*n-word device buffer (caller frees with cache_free)
// holding the columns [gp | glo | ghi | ap | alo | ahi], each n words apart:
// the gather ranges (p, [ts-before-after, ts+before+after]) in the first
// n_gather entries of the g columns, the affected ranges
// (p, [ts-after, ts+before]) in the first n_affected entries of the a
// columns.  *err = 1 (and no ranges) if a partition or time is >= 2^32.
// time_hi: the delta's rows are (p, ts << 32 | val) and the time is v >> 32
// (rows of one (p, ts) have equal ranges and fall into one run); otherwise
// the time is v.  One host sync.
dbsp_status roll_ranges(hipStream_t s, const Rows &delta, bool time_hi,
                        uint64_t before, uint64_t after, uint64_t **ranges,
                        int64_t *n_gather, int64_t *n_affected, int *err);
// copy the rows of every spine batch that fall in a range, weights times
// sign.  mode 0: (k, v) in [(p, lo), (p, hi)]; mode 1: k in
// [p<<32|lo, p<<32|hi]; mode 2: (k, v) in [(p, lo<<32), (p, hi<<32|0xffffffff)]
// (rows whose v packs ts << 32 | val).  Ranges must be disjoint; output is
// RAW (range-major, batch-minor runs).
dbsp_status range_gather(hipStream_t s, const uint64_t *rp,
                         const uint64_t *rlo, const uint64_t *rhi, int64_t nr,
                         const TraceArgs &t, int mode, int64_t sign,
                         Rows *out);
// keep the rows of every spine batch whose time is >= bound, in order
// (trace.rs:463-607 lower bound).  mode 0: time = v (rows (p, ts, w));
// mode 1: time = k & 0xffffffff (rows (p<<32|ts, sum, w)); mode 2: time =
// v >> 32 (rows (p, ts<<32|val, w)).  out is a caller
// array of t.nb entries: batch b's survivors in fresh columns (null when
// none survive).  Stable, so a consolidated batch stays consolidated.  One
// host sync for all lengths.
dbsp_status truncate_spine(hipStream_t s, const TraceArgs &t, int mode,
                           uint64_t bound, Rows *out);
// per row (p, ts, w > 0) of the consolidated slice that the delta affects
// (delta's weights unread): (p<<32|ts, sum of slice weights of p over
// [ts-before, ts+after], +1), in slice order (sorted, distinct keys)
dbsp_status roll_eval_rows(hipStream_t s, const Rows &slice,
                           const Rows &delta, uint64_t before, uint64_t after,
                           Rows *out);


// ---- rolling Max / Min (partitioned_rolling_aggregate with Agg = Max | Min,
// rolling_aggregate.rs:235-321; aggregate/max.rs:36-55, min.rs:38-57) over
// rows (p, ts << 32 | val, w) ----
// batch primitive: per row of the consolidated batch, (k, v, M) with M the
// max (is_min: min) of val over the partition's rows with time in
// [ts - before, ts + after], weights of either sign counting; out holds in.n
// rows (its n is ignored)
dbsp_status rolling_minmax_rows(hipStream_t s, const Rows &in, bool is_min,
                                uint64_t before, uint64_t after,
                                const Rows &out);
// per TIME (p, ts) of the consolidated slice that holds a row of w > 0 and
// that the delta affects (delta's weights unread): (p<<32|ts, M over
// [ts-before, ts+after] of the slice, +1), in slice order (sorted, distinct
// keys)
dbsp_status roll_eval_minmax_rows(hipStream_t s, const Rows &slice,
                                  const Rows &delta, bool is_min,
                                  uint64_t before, uint64_t after, Rows *out);

// ---- incremental top-K per group (the aggregate(Fold) + flat_map of
// queries/q19.rs; presence = non-zero total weight, aggregate/fold.rs:83-92).
// A row's group is k >> shift (0..63); its keys are the inclusive range
// [k & ~mask, k | mask], mask = 2^shift - 1 ----
// Classify the rows of a consolidated delta against the input integral
// BEFORE the tick (t: its spine batches) and list the affected groups.
// *plan is one 4*n-word device buffer (caller frees with cache_free) holding
// the columns [cls | gidx | glo | ghi], each n words apart: cls (int64) +1
// appear / -1 vanish / 0 neither and gidx the group index per delta row;
// glo/ghi the key range of the first n_groups affected groups, in key order.
// One host sync.
dbsp_status topk_classify(hipStream_t s, const Rows &delta, const TraceArgs &t,
                          int shift, uint64_t **plan, int64_t *n_groups);
// copy the rows of every spine batch with k in [klo[r], khi[r]], weights
// times sign; ranges disjoint, output RAW (range-major, batch-minor runs)
dbsp_status keyrange_gather(hipStream_t s, const uint64_t *klo,
                            const uint64_t *khi, int64_t nr,
                            const TraceArgs &t, int64_t sign, Rows *out);
// Per-group refill flag.  cur: the affected groups' current top-K rows,
// consolidated (weights unread).  A group refills iff one of its vanish rows
// r has count(cur_g) == K and r >= first(cur_g); refill_all flags them all.
// *verdict is one 3*ng-word device buffer (caller frees) [refill | rlo | rhi]:
// the flag per group, then the key ranges of the n_refill flagged groups.
// One host sync.
dbsp_status topk_verdict(hipStream_t s, const Rows &delta,
                         const uint64_t *plan, int64_t ng, const Rows &cur,
                         int64_t K, bool refill_all, uint64_t **verdict,
                         int64_t *n_refill);
// raw candidate rows of the groups NOT refilled: cur's rows at +1, appear
// rows at +1, vanish rows that are in cur at -1
dbsp_status topk_candidates(hipStream_t s, const Rows &delta,
                            const uint64_t *plan, int64_t ng,
                            const uint64_t *refill, const Rows &cur,
                            Rows *out);
// the last <= K rows of every group of a consolidated slice, as (k, v, +1),
// in order
dbsp_status topk_select(hipStream_t s, const Rows &slice, int64_t K, int shift,
                        Rows *out);

// ---- incremental antijoin / semijoin (Stream::antijoin, operator/join.rs:
// 294-320).  The right side is a key set held as rows (k, 0, w); a key is
// present iff its total weight over every batch is > 0 (operator/distinct.rs).
// The kernels read k and w of a key-set batch, never v ----
// Per key of the consolidated key delta db (distinct keys, v unread):
// flip = [before + dw > 0] - [before > 0] with before its weight in t BEFORE
// the tick.  *plan is one 2*n_flip-word device buffer (caller frees with
// cache_free; null when nothing flips) [key | mul]: the flipped keys in order
// and mul (int64) = -flip for the antijoin, +flip for the semijoin.  One host
// sync.
dbsp_status anti_flip(hipStream_t s, const Rows &db, const TraceArgs &t,
                      bool anti, uint64_t **plan, int64_t *n_flip);
// copy the rows of every spine batch with k == keys[r], weights times
// mul[r]; keys distinct, output RAW (key-major, batch-minor runs)
dbsp_status keyrange_gather_mul(hipStream_t s, const uint64_t *keys,
                                const int64_t *mul, int64_t nr,
                                const TraceArgs &t, Rows *out);
// the rows of a consolidated batch a whose key is absent from (anti) or
// present in (!anti) the key set t, in order: one search per key head
dbsp_status anti_filter(hipStream_t s, const Rows &a, const TraceArgs &t,
                        bool anti, Rows *out);

// ---- incremental arg-max per group, ties kept (the tail of queries/q7.rs:
// 82-93).  Group k >> group_shift, rank k >> rank_shift, rank_shift <=
// group_shift; presence as for top-K, per row.  The plan is topk_classify's
// and both gathers are keyrange_gather ----
// Per-group refill flag.  cur: the affected groups' current tie sets,
// consolidated, at their real weights.  A group with rows in cur refills iff
// every one of them vanishes in the tick and no delta row of rank >= cur's
// rank is present after it; refill_all flags every affected group.  *verdict
// is one 3*ng-word device buffer (caller frees) [refill | rlo | rhi], as
// topk_verdict's.  One host sync.
dbsp_status argmax_verdict(hipStream_t s, const Rows &delta,
                           const uint64_t *plan, int64_t ng, const Rows &cur,
                           int rank_shift, bool refill_all, uint64_t **verdict,
                           int64_t *n_refill);
// raw candidate rows of the groups NOT refilled: cur's rows at their weights
// and the delta rows of rank >= cur's rank (all of them where the group has
// none in cur) at theirs
dbsp_status argmax_candidates(hipStream_t s, const Rows &delta,
                              const uint64_t *plan, int64_t ng,
                              const uint64_t *refill, const Rows &cur,
                              int rank_shift, Rows *out);
// the rows of a consolidated slice whose rank is their group's largest, at
// their own weights, in order
dbsp_status argmax_select(hipStream_t s, const Rows &slice, int group_shift,
                          int rank_shift, Rows *out);
// w[i] = -w[i] (no sync)
void negate_weights(hipStream_t s, int64_t *w, int64_t n);
// query 7: rows (date_time << 27 | price, v, w) -> (price << 32 | date_time,
// v, w); out holds in.n rows (its n is ignored)
dbsp_status map_price_time(hipStream_t s, const Rows &in, const Rows &out);

uint64_t host_xxh3_u64(uint64_t key, uint64_t seed);

}  // namespace dbspk
