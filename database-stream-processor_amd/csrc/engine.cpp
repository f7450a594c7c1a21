// engine.cpp — host-side mirror of the reference's Circuit/Stream API driving
// the CDNA4 kernels (kernels.hip) over HBM-resident batches.
//
// The reference keeps one OS thread per worker, each evaluating an identical
// operator DAG once per tick under a static scheduler
// (circuit/circuit_builder.rs:1403, circuit/schedule/static_scheduler.rs,
// dbsp_handle.rs:246).  Here: one PROCESS per GPU (rank), one HIP stream per
// rank as the scheduler's execution lane, and the per-query operator DAG is
// evaluated in construction (= topological) order by dbsp_engine_step.
// Cross-worker exchange (operator/communication/exchange.rs:45-251, an N^2
// mailbox) is an RCCL grouped send/recv (all-to-all-v) over xGMI.
//
// Trace state: each Z1Trace/TraceAppend feedback loop (operator/trace.rs:173-460)
// is a Spine — a stack of consolidated batches with geometric sizes
// (spine_fueled.rs:107-119).  Unlike the reference's fueled incremental merging
// (spine_fueled.rs:856: merges amortised across ticks because a CPU merge is
// slow), GPU merges run to completion per launch — the merge-path kernel moves
// GB/ms, so the spine policy only decides WHEN to merge (same power-of-two
// level policy), not how much fuel each tick contributes.
//
// Linear operators (join, window, linear aggregate, upsert retraction) are
// evaluated per spine batch and summed — the reference reads spines through a
// k-way CursorList (trace/cursor/cursor_list.rs); linearity makes per-batch
// evaluation + one consolidate equivalent and keeps every kernel a flat
// sorted-array pass.

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <functional>

#include "../../include/dbsp_hip.h"
#include "kernels_iface.hpp"

#define HIP_CHECK_ST(x)                                                   \
    do {                                                                  \
        hipError_t err_ = (x);                                            \
        if (err_ != hipSuccess) {                                         \
            fprintf(stderr, "HIP error %s at %s:%d\n",                    \
                    hipGetErrorString(err_), __FILE__, __LINE__);         \
            return DBSP_ERR_INTERNAL;                                     \
        }                                                                 \
    } while (0)

#define TRY(x)                                                            \
    do {                                                                  \
        dbsp_status st_ = (x);                                            \
        if (st_ != DBSP_OK) return st_;                                   \
    } while (0)

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------

struct KernelStat {
    double ms = 0;
    double bytes = 0;
    int64_t launches = 0;
};

// Length-slot layout of dbsp_ctx::d_len / h_len (int64 slots; the one
// description of it).  Kernels leave lengths, totals and -1 poison/overflow
// sentinels in the device slots; the host reads them from the pinned mirror
// after a readback (read_len below), normally at the same index.
//
//   [LEN_OP ..)          ops that sync at once (sized sorts and merges, the
//                        aggregate's join count) borrow up to SORT_BATCH_MAX
//                        slots from the start of tick base 0 (they alias
//                        that base's first offsets)
//   [sb, sb + LEN_TICK)  one chained tick, sb = LEN_BASE0 or LEN_BASE1 (q3's
//                        pipelined trains ping-pong; everything else uses
//                        LEN_BASE0).  Offsets inside a base are the L_* below
//   [sb + LEN_TICK, sb + LEN_BASE_N)
//                        HOST only: the landing block of q3's tail readback
//                        (the LH_* offsets below); no kernel writes the
//                        device side of it
//   [LEN_ROUND, +4)      spine-insert merge rounds: their readback can be
//                        consumed after the next train's readbacks have
//                        landed, so it cannot live inside a base
enum : int {
    LEN_SLOTS = 60,
    LEN_OP = 0,
    LEN_TICK = 20,       // kernel-written slots of a tick base
    LEN_BASE_N = 28,     // slots per tick base, host tail block included
    LEN_BASE0 = 0,
    LEN_BASE1 = LEN_BASE_N,
    LEN_ROUND = 2 * LEN_BASE_N,
    LEN_ROUND_N = MERGE_BATCH_MAX,
    // offsets inside a tick base
    L_PLAN = 0,          // 0..2: q3 join-plan count totals (-1: lost spec)
    L_EMIT_TOTAL = 3,    // join tail: combined row total (or -1)
    L_EMIT_FLAG = 4,     // join tail: nonzero = capacity overflow
    L_DENSE = 5,         // q5: chained dense-sort length of the bid delta
    L_FINAL = 6,         // output (final) sort length
    L_WIN = 7,           // single-spine window total (q5, dbsp_window)
    L_RAW = 8,           // 8/9: flatmap raw lengths of streams A/B: the
                         // flatmap's ticket counters.  A taking delta sort
                         // (q3's train) hands them back zeroed and leaves
                         // the lengths at L_RAWN instead
    L_DELTA = 10,        // 10/11: consolidated delta lengths (-1: overflow)
    L_WIN2 = 12,         // 12/13: q8's two window totals (-1: lost spec)
    L_MINMAX = 12,       // 12..15: q5's {kmin, vmin, kmax, vmax} of the bids
    L_XCHG = 16,         // 16/17: framed-exchange receive totals (-1:
                         // frame overflow); q3's unsharded train reuses them
                         // for its two accumulator-merge lengths
    L_RAWN = 18,         // 18/19: raw lengths as a taking delta sort saw
                         // them (what the head readback of a train carries
                         // in place of L_RAW, which then reads 0)
    // A chained q3 tick reads back twice.
    // HEAD: device [L_HEAD, L_HEAD + L_HEAD_N) to the same host offsets.  It
    // carries what is final once the delta sorts and the accumulator merge
    // are: L_RAW (or L_RAWN behind a taking sort), L_DELTA and L_XCHG.  The
    // host wakes on it for the speculation verdict.
    L_HEAD = L_RAW,
    L_HEAD_N = LEN_TICK - L_RAW,
    // TAIL: device [L_PLAN, L_FINAL] — everything the join tail kernel
    // writes — to HOST offsets shifted by LH_TAIL_SHIFT, into the base's
    // host-only block.  That block is clear of the head readback's range
    // and of LEN_OP: ops that sync at once (an overflow replay's sized
    // sorts) may run between a tail readback landing and its consumption.
    LH_TAIL_SHIFT = LEN_TICK,
    LH_TAIL_N = L_FINAL - L_PLAN + 1,
    LH_PLAN = L_PLAN + LH_TAIL_SHIFT,              // 20..22
    LH_EMIT_TOTAL = L_EMIT_TOTAL + LH_TAIL_SHIFT,  // 23
    LH_EMIT_FLAG = L_EMIT_FLAG + LH_TAIL_SHIFT,    // 24
    LH_FINAL = L_FINAL + LH_TAIL_SHIFT,            // 26
};
static_assert(LEN_BASE1 + LEN_BASE_N <= LEN_ROUND &&
                  LEN_ROUND + LEN_ROUND_N <= LEN_SLOTS,
              "both tick bases and the round slots fit the allocation");
static_assert(LEN_BASE0 + LEN_BASE_N <= LEN_BASE1, "tick bases overlap");
static_assert(L_PLAN + 3 <= L_EMIT_TOTAL && L_EMIT_TOTAL < L_EMIT_FLAG &&
                  L_EMIT_FLAG < L_FINAL && L_FINAL < L_HEAD,
              "the tail readback's device range holds the join tail's "
              "outputs and nothing of the head");
static_assert(L_HEAD <= L_RAW && L_HEAD <= L_DELTA &&
                  L_DELTA + 2 <= L_HEAD + L_HEAD_N &&
                  L_XCHG + 2 <= L_HEAD + L_HEAD_N &&
                  L_HEAD <= L_RAWN && L_RAWN + 2 <= L_HEAD + L_HEAD_N &&
                  L_HEAD + L_HEAD_N <= LEN_TICK,
              "the head readback carries raw, delta and merge lengths");
static_assert(L_XCHG + 2 <= L_RAWN && L_RAWN + 2 <= LEN_TICK,
              "the taken raw lengths have slots of their own");
static_assert(LEN_OP + SORT_BATCH_MAX <= L_RAW,
              "no op scratch slot aliases a flatmap counter: only flatmaps "
              "and taking sorts write those (dbsp_ctx::raw_zero)");
static_assert(LH_PLAN >= LEN_TICK && LH_PLAN >= LEN_OP + SORT_BATCH_MAX &&
                  LH_PLAN + LH_TAIL_N <= LEN_BASE_N,
              "tail-readback host range stays inside its base, clear of "
              "the head readback and the op scratch");
static_assert(LEN_OP + SORT_BATCH_MAX <= LEN_TICK, "op scratch inside base 0");

struct dbsp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool profile = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KernelStat stats[6];
    // RCCL
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    bool force_shard = false;  // exercise the full partition+alltoallv path
                               // even at world=1 (self-exchange; test hook)
    // persistent length scratch (device + pinned host)
    int64_t *d_len = nullptr;  // LEN_SLOTS slots, layout above
    int64_t *h_len = nullptr;
    int64_t *d_mid = nullptr;  // merge_mid per-WG count scratch
                               // (MERGE_BATCH_MAX pairs)
    // "raw counters known zero", per tick base (0: LEN_BASE0, 1: LEN_BASE1):
    // the base's L_RAW pair holds 0 once everything enqueued so far has run,
    // because the last thing enqueued that writes it is a taking sort behind
    // the flatmap.  flatmap_chain consumes it (skips its memset and clears
    // it: the flatmap dirties the counters); only sort_pair_chain's taking
    // form sets it.  Nothing else writes those two slots.
    bool raw_zero[2] = {false, false};
    bool q3_fold = true;       // in-train fold by k_acc_fold (DBSP_Q3_FOLD=0:
                               // merge_mid_batch, for comparison)
    bool q3_take = true;       // the train's sorts take the flatmap counters
                               // (DBSP_Q3_TAKE=0: plain sorts, so every
                               // flatmap keeps its counter fill)
    int timer_depth = 0;  // ScopedTimer nesting guard (shared event pair)
    // per-tick transient bump arena (reset at each engine tick; falls back to
    // the stream-ordered pool when exhausted)
    uint8_t *arena = nullptr;
    size_t arena_sz = 0;
    size_t arena_off = 0;
    // ping-pong halves: a pipelined tick launches the NEXT tick's front half
    // while this tick finishes, so two ticks' transients are live at once
    size_t arena_base = 0;
    size_t arena_half = 0;  // half size (arena_sz / 2); 0 = no split
    hipEvent_t ev_sync = nullptr;   // tick-end event (pre-front-launch point)
    hipEvent_t ev_sync2 = nullptr;  // early-wake event (post-count readback)
    hipEvent_t ev_tick[2] = {nullptr, nullptr};  // pipelined-train events
    hipEvent_t ev_tail[2] = {nullptr, nullptr};  // train tail (post 2nd readback)
    // q3 train fork: `stream` is the LOOP stream (flatmap, delta sorts, fold,
    // head readback, ev_tick: what the host waits for each tick); the probe,
    // the join tail and the tail readback run on the BACK stream `side`
    // behind ev_fork (recorded on the loop stream after the delta sorts) and
    // end in ev_tail.  q3_fork is off under DBSP_PROFILE (ScopedTimer's
    // events assume one stream) and with DBSP_Q3_FORK=0.
    hipStream_t side = nullptr;
    hipEvent_t ev_fork[2] = {nullptr, nullptr};
    bool q3_fork = false;
    // index of the last ev_tail recorded on the back stream that the loop
    // stream has not been ordered behind (neither by a stream wait nor by a
    // host sync); -1: no back-stream work can be live.  See q3_join_back.
    int back_live = -1;
    // deferred spine-insert round (train path): the last small-merge round's
    // length readback is resolved at the NEXT insert/step on a near-empty
    // stream instead of blocking behind the next tick's freshly enqueued
    // train (the LEN_ROUND host slots hold its counts until then)
    hipEvent_t ev_insert = nullptr;
    int pend_n = 0;
    void *pend_spine[4] = {};
    uint64_t *pend_k[4] = {}, *pend_v[4] = {};
    int64_t *pend_w[4] = {};
    int pend_slot[4] = {};  // LEN_ROUND + s holds each result length
};

// Length readback: copy `count` device slots from `first` to host slots from
// `host_first`; with sync, wait for them.  Every read of h_len follows one.
// `s`: the stream to copy on (null = the main stream).
static dbsp_status read_len_to(dbsp_ctx *c, int host_first, int first,
                               int count, bool sync,
                               hipStream_t s = nullptr) {
    if (!s) s = c->stream;
    HIP_CHECK_ST(hipMemcpyAsync(c->h_len + host_first, c->d_len + first,
                                count * sizeof(int64_t),
                                hipMemcpyDeviceToHost, s));
    if (sync) HIP_CHECK_ST(hipStreamSynchronize(s));
    return DBSP_OK;
}
static inline dbsp_status read_len(dbsp_ctx *c, int first, int count,
                                   bool sync = true) {
    return read_len_to(c, first, first, count, sync);
}
// a host length slot whose kernel poisons it (-1) on a broken fused barrier
static inline dbsp_status checked_len(dbsp_ctx *c, int slot, int64_t &n) {
    n = c->h_len[slot];
    return n < 0 ? DBSP_ERR_INTERNAL : DBSP_OK;
}

static void *arena_alloc(dbsp_ctx *c, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    size_t limit = c->arena_half ? c->arena_base + c->arena_half : c->arena_sz;
    if (!c->arena || c->arena_base + c->arena_off + bytes > limit)
        return nullptr;
    void *p = c->arena + c->arena_base + c->arena_off;
    c->arena_off += bytes;
    return p;
}

// restart the bump arena in the half that does not start at `base` (two
// ticks' transients are live at once); an unsplit arena just restarts
static inline void arena_other_half(dbsp_ctx *c, size_t base) {
    if (c->arena_half) c->arena_base = base ? 0 : c->arena_half;
    c->arena_off = 0;
}

static inline bool in_arena(dbsp_ctx *c, const void *p) {
    return c->arena && p >= c->arena && p < c->arena + c->arena_sz;
}

// Scratch owned for a scope: a stream-cache block goes back to the cache on
// the ctx stream when the scope ends, whichever return ends it, so TRY is
// safe around it; a block of the tick arena needs no free.
struct ScratchBuf {
    dbsp_ctx *c = nullptr;
    void *p = nullptr;
    bool cached = false;  // p is a cache_malloc block: ours to free
    ScratchBuf() = default;
    // adopt a block some kernel-interface call cache_malloc'd
    ScratchBuf(dbsp_ctx *c_, void *block) : c(c_), p(block), cached(true) {}
    ScratchBuf(const ScratchBuf &) = delete;
    ScratchBuf &operator=(const ScratchBuf &) = delete;
    ~ScratchBuf() { reset(); }
    // arena_first: the tick arena, the stream cache only when that is full
    dbsp_status alloc(dbsp_ctx *c_, size_t bytes, bool arena_first = false) {
        reset();
        c = c_;
        if (arena_first) p = arena_alloc(c, bytes);
        if (!p) {
            HIP_CHECK_ST(dbspk::cache_malloc(&p, bytes, c->stream));
            cached = true;
        }
        return DBSP_OK;
    }
    void reset() {
        if (cached) (void)dbspk::cache_free(p, c->stream);
        release();
    }
    // ownership passes out: the caller frees
    void *release() {
        void *r = p;
        p = nullptr;
        cached = false;
        return r;
    }
    template <class T> T *as() const { return (T *)p; }
};

// Join on demand (q3 trains; the ordering argument above the q3 tick): put
// the loop stream behind everything enqueued on the back stream so far.  The
// back stream runs in order, so its last ev_tail covers all of it.  Called
// before anything on the loop stream frees, recycles or overwrites what a
// probe or join tail in flight may still use; free when nothing is in flight.
static inline void q3_join_back(dbsp_ctx *c) {
    if (c->back_live < 0) return;
    (void)hipStreamWaitEvent(c->stream, c->ev_tail[c->back_live], 0);
    c->back_live = -1;
}
// the same where the host itself must be behind the back stream
static inline void q3_sync_back(dbsp_ctx *c) {
    if (c->back_live < 0) return;
    (void)hipEventSynchronize(c->ev_tail[c->back_live]);
    c->back_live = -1;
}

extern "C" dbsp_status dbsp_ctx_create(dbsp_ctx **out, int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        fprintf(stderr,
                "dbsp: NO GPU AVAILABLE (hipGetDeviceCount: %s). The product "
                "path requires an MI355X; there is no CPU fallback.\n",
                hipGetErrorString(e));
        return DBSP_ERR_NOGPU;
    }
    dbsp_ctx *c = new dbsp_ctx();
    c->device = device;
    // spin-wait syncs: the tick pipeline syncs on data-dependent lengths a few
    // times per tick; yield-based waits cost 10-20 us each
    (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
    HIP_CHECK_ST(hipSetDevice(device));
    // keep freed stream-ordered allocations in the pool (the tick pipeline
    // allocates/frees ~20 buffers per tick; without this the pool trims back
    // to the OS between ticks)
    {
        hipMemPool_t mp;
        if (hipDeviceGetDefaultMemPool(&mp, device) == hipSuccess) {
            uint64_t thresh = UINT64_MAX;
            (void)hipMemPoolSetAttribute(mp, hipMemPoolAttrReleaseThreshold,
                                         &thresh);
        }
    }
    HIP_CHECK_ST(hipStreamCreate(&c->stream));
    HIP_CHECK_ST(hipEventCreate(&c->ev0));
    HIP_CHECK_ST(hipEventCreate(&c->ev1));
    HIP_CHECK_ST(hipEventCreateWithFlags(&c->ev_sync, hipEventDisableTiming));
    HIP_CHECK_ST(hipEventCreateWithFlags(&c->ev_sync2, hipEventDisableTiming));
    HIP_CHECK_ST(hipEventCreateWithFlags(&c->ev_tick[0], hipEventDisableTiming));
    HIP_CHECK_ST(hipEventCreateWithFlags(&c->ev_tick[1], hipEventDisableTiming));
    HIP_CHECK_ST(hipEventCreateWithFlags(&c->ev_insert, hipEventDisableTiming));
    HIP_CHECK_ST(hipEventCreateWithFlags(&c->ev_tail[0], hipEventDisableTiming));
    HIP_CHECK_ST(hipEventCreateWithFlags(&c->ev_tail[1], hipEventDisableTiming));
    HIP_CHECK_ST(hipStreamCreate(&c->side));
    HIP_CHECK_ST(hipEventCreateWithFlags(&c->ev_fork[0], hipEventDisableTiming));
    HIP_CHECK_ST(hipEventCreateWithFlags(&c->ev_fork[1], hipEventDisableTiming));
    const char *p = getenv("DBSP_PROFILE");
    c->profile = p && p[0] == '1';
    const char *fs = getenv("DBSP_FORCE_SHARD");
    c->force_shard = fs && fs[0] == '1';
    const char *fk = getenv("DBSP_Q3_FORK");
    c->q3_fork = !c->profile && !(fk && fk[0] == '0');
    const char *fo = getenv("DBSP_Q3_FOLD");
    c->q3_fold = !(fo && fo[0] == '0');
    const char *tk = getenv("DBSP_Q3_TAKE");
    c->q3_take = !(tk && tk[0] == '0');
    HIP_CHECK_ST(hipMalloc(&c->d_len, LEN_SLOTS * sizeof(int64_t)));
    HIP_CHECK_ST(hipMalloc(&c->d_mid, MERGE_BATCH_MAX * MERGE_MID_SCRATCH *
                                          sizeof(int64_t)));
    // generation tags count up from 1: recycled memory must not look tagged
    HIP_CHECK_ST(hipMemset(c->d_mid, 0, MERGE_BATCH_MAX * MERGE_MID_SCRATCH *
                                            sizeof(int64_t)));
    c->arena_sz = (size_t)512 << 20;
    c->arena_half = c->arena_sz / 2;
    if (hipMalloc(&c->arena, c->arena_sz) != hipSuccess) {
        c->arena = nullptr;
        c->arena_sz = 0;
    }
    HIP_CHECK_ST(hipHostMalloc(&c->h_len, LEN_SLOTS * sizeof(int64_t)));
    *out = c;
    return DBSP_OK;
}

static void drop_pending_insert(dbsp_ctx *c);

extern "C" dbsp_status dbsp_ctx_destroy(dbsp_ctx *c) {
    if (!c) return DBSP_OK;
    q3_sync_back(c);
    drop_pending_insert(c);
    if (c->ev_insert) (void)hipEventDestroy(c->ev_insert);
    if (c->ev_tail[0]) (void)hipEventDestroy(c->ev_tail[0]);
    if (c->ev_tail[1]) (void)hipEventDestroy(c->ev_tail[1]);
    if (c->ev_sync) (void)hipEventDestroy(c->ev_sync);
    if (c->ev_sync2) (void)hipEventDestroy(c->ev_sync2);
    if (c->ev_tick[0]) (void)hipEventDestroy(c->ev_tick[0]);
    if (c->ev_tick[1]) (void)hipEventDestroy(c->ev_tick[1]);
    if (c->comm) ncclCommDestroy(c->comm);
    (void)hipStreamSynchronize(c->stream);
    if (c->side) {
        (void)hipStreamSynchronize(c->side);
        (void)hipStreamDestroy(c->side);
    }
    if (c->ev_fork[0]) (void)hipEventDestroy(c->ev_fork[0]);
    if (c->ev_fork[1]) (void)hipEventDestroy(c->ev_fork[1]);
    if (c->d_len) (void)hipFree(c->d_len);
    if (c->d_mid) (void)hipFree(c->d_mid);
    dbspk::cache_trim(c->stream);
    (void)hipStreamSynchronize(c->stream);
    if (c->arena) (void)hipFree(c->arena);
    if (c->h_len) (void)hipHostFree(c->h_len);
    (void)hipEventDestroy(c->ev0);
    (void)hipEventDestroy(c->ev1);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_ctx_sync(dbsp_ctx *c) {
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    q3_sync_back(c);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_dev_alloc(dbsp_ctx *c, size_t bytes, void **out) {
    HIP_CHECK_ST(hipMallocAsync(out, bytes, c->stream));
    return DBSP_OK;
}
extern "C" dbsp_status dbsp_dev_free(dbsp_ctx *c, void *p) {
    HIP_CHECK_ST(dbspk::cache_free(p, c->stream));
    return DBSP_OK;
}
extern "C" dbsp_status dbsp_h2d(dbsp_ctx *c, void *dst, const void *src,
                                size_t bytes) {
    HIP_CHECK_ST(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return DBSP_OK;
}
extern "C" dbsp_status dbsp_d2h(dbsp_ctx *c, void *dst, const void *src,
                                size_t bytes) {
    HIP_CHECK_ST(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    return DBSP_OK;
}

// profiling helpers: ops sync internally, so record/elapse inline
struct ScopedTimer {
    dbsp_ctx *c;
    int cls;
    double bytes;
    bool active;
    ScopedTimer(dbsp_ctx *c_, int cls_, double bytes_) : c(c_), cls(cls_), bytes(bytes_) {
        // nested ops (e.g. the merge tree inside a medium sort) attribute to
        // the OUTER class — one shared event pair
        active = c->profile && c->timer_depth == 0;
        c->timer_depth++;
        if (active) (void)hipEventRecord(c->ev0, c->stream);
    }
    ~ScopedTimer() {
        c->timer_depth--;
        if (active) {
            (void)hipEventRecord(c->ev1, c->stream);
            (void)hipEventSynchronize(c->ev1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
            c->stats[cls].ms += ms;
            c->stats[cls].bytes += bytes;
            c->stats[cls].launches += 1;
        }
    }
};

// ---------------------------------------------------------------------------
// device batches + spine
// ---------------------------------------------------------------------------

using DevBatch = dbspk::Rows;

static void free_batch(dbsp_ctx *c, DevBatch &b) {
    if (b.k && !in_arena(c, b.k)) (void)dbspk::cache_free(b.k, c->stream);
    if (b.v && !in_arena(c, b.v)) (void)dbspk::cache_free(b.v, c->stream);
    if (b.w && !in_arena(c, b.w)) (void)dbspk::cache_free(b.w, c->stream);
    b = DevBatch{};
}

static dbsp_status alloc_batch(dbsp_ctx *c, int64_t n, DevBatch &b,
                               bool transient = false) {
    b.n = n;
    if (transient) {
        size_t one = (size_t)(n * 8 + 8 + 255) & ~(size_t)255;
        uint8_t *blk = (uint8_t *)arena_alloc(c, 3 * one);
        if (blk) {
            b.k = (uint64_t *)blk;
            b.v = (uint64_t *)(blk + one);
            b.w = (int64_t *)(blk + 2 * one);
            return DBSP_OK;
        }
    }
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&b.k, n * sizeof(uint64_t) + 8, c->stream));
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&b.v, n * sizeof(uint64_t) + 8, c->stream));
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&b.w, n * sizeof(int64_t) + 8, c->stream));
    return DBSP_OK;
}

// device-to-device copy of n rows' three columns to dst rows [off, off + n)
static dbsp_status copy_cols(dbsp_ctx *c, const DevBatch &dst, int64_t off,
                             const uint64_t *k, const uint64_t *v,
                             const void *w, int64_t n) {
    if (n == 0) return DBSP_OK;
    HIP_CHECK_ST(hipMemcpyAsync(dst.k + off, k, n * 8, hipMemcpyDeviceToDevice, c->stream));
    HIP_CHECK_ST(hipMemcpyAsync(dst.v + off, v, n * 8, hipMemcpyDeviceToDevice, c->stream));
    HIP_CHECK_ST(hipMemcpyAsync(dst.w + off, w, n * 8, hipMemcpyDeviceToDevice, c->stream));
    return DBSP_OK;
}

// concat batches into one freshly allocated batch (raw, unsorted use)
static dbsp_status concat_batches(dbsp_ctx *c, const std::vector<DevBatch> &in,
                                  DevBatch &out, bool transient = false) {
    int64_t total = 0;
    for (auto &b : in) total += b.n;
    TRY(alloc_batch(c, total, out, transient));
    int64_t off = 0;
    for (auto &b : in) {
        TRY(copy_cols(c, out, off, b.k, b.v, b.w, b.n));
        off += b.n;
    }
    out.n = total;
    return DBSP_OK;
}

// copy a batch (for inserting a delta into a spine while retaining it)
static dbsp_status copy_batch(dbsp_ctx *c, const DevBatch &in, DevBatch &out) {
    TRY(alloc_batch(c, in.n > 0 ? in.n : 1, out));
    out.n = in.n;
    return copy_cols(c, out, 0, in.k, in.v, in.w, in.n);
}

static inline void put_batch(dbsp_batch *out, const DevBatch &b) {
    out->k = b.k; out->v = b.v; out->w = b.w; out->len = b.n;
}
static inline DevBatch as_batch(const dbsp_batch *b) {
    return DevBatch{b->k, b->v, b->w, b->len};
}

// ---- launch-descriptor fills ----

// slot i of a fused sort: in -> out through scratch.  n_dev (a device length
// slot) overrides the host length, which then stays 0.
static inline void sort_slot(SortArgs &sa, int i, const DevBatch &in,
                             const DevBatch &scratch, const DevBatch &out,
                             const int64_t *n_dev = nullptr) {
    sa.kin[i] = in.k; sa.vin[i] = in.v; sa.win[i] = in.w;
    sa.n[i] = n_dev ? 0 : in.n;
    sa.n_dev[i] = n_dev;
    sa.tk[i] = scratch.k; sa.tv[i] = scratch.v; sa.tw[i] = scratch.w;
    sa.ok[i] = out.k; sa.ov[i] = out.v; sa.ow[i] = out.w;
}

// the taking form: the length comes from the producer's counter `take`,
// which the sort hands back zeroed, leaving what it saw at `seen`; in.n is
// the capacity of the input columns
static inline void sort_slot_take(SortArgs &sa, int i, const DevBatch &in,
                                  const DevBatch &scratch, const DevBatch &out,
                                  int64_t *take, int64_t *seen) {
    sort_slot(sa, i, in, scratch, out, take);
    sa.n_dev[i] = nullptr;
    sa.n_take[i] = take;
    sa.n_seen[i] = seen;
    sa.n_cap[i] = in.n;
}

// pair p of a batched merge: a + b -> out.  dnb (a device length slot)
// overrides b's host length, which then stays 0; bcap bounds it for the
// accumulator fold (out holds a.n + bcap rows).
static inline void merge_pair(MergeArgs &ma, int p, const DevBatch &a,
                              const DevBatch &b, const DevBatch &out,
                              const int64_t *dnb = nullptr, int64_t bcap = 0) {
    ma.ak[p] = a.k; ma.av[p] = a.v; ma.aw[p] = a.w; ma.na[p] = a.n;
    ma.bk[p] = b.k; ma.bv[p] = b.v; ma.bw[p] = b.w;
    ma.nb[p] = dnb ? 0 : b.n;
    ma.dnb[p] = dnb;
    ma.bcap[p] = dnb ? bcap : b.n;
    ma.ok[p] = out.k; ma.ov[p] = out.v; ma.ow[p] = out.w;
}

static inline void trace_push(TraceArgs &t, const DevBatch &b) {
    t.k[t.nb] = b.k; t.v[t.nb] = b.v; t.w[t.nb] = b.w; t.n[t.nb] = b.n;
    t.nb++;
}
static inline TraceArgs trace_args_one(const DevBatch &b) {
    TraceArgs t{};
    trace_push(t, b);
    return t;
}

// wf64: f64 weights, carried as their bit patterns (config C5's weighted
// integral spine; position-fixed reduction orders, algebra/floats.rs:24 zero
// elimination)
static dbsp_status merge_batches(dbsp_ctx *c, const DevBatch &a,
                                 const DevBatch &b, DevBatch &out,
                                 bool wf64 = false);

// medium raw batches (8192 < n <= 64k): chunk into <=8 fused single-WG sorts
// in ONE launch, then a batched single-WG merge tree (3 launches, 1 sync per
// round) — replaces ~25 launches of the global radix pipeline at these sizes
static dbsp_status sort_medium(dbsp_ctx *c, DevBatch raw, DevBatch &out) {
    int nch = (int)((raw.n + 8191) / 8192);
    SortArgs sa{};
    sa.nb = nch;
    std::vector<DevBatch> chunks(nch), scratch(nch);
    for (int i = 0; i < nch; i++) {
        int64_t lo = (int64_t)i * 8192;
        int64_t len = std::min<int64_t>(8192, raw.n - lo);
        TRY(alloc_batch(c, len, scratch[i], true));
        TRY(alloc_batch(c, len, chunks[i], true));
        sort_slot(sa, i, DevBatch{raw.k + lo, raw.v + lo, raw.w + lo, len},
                  scratch[i], chunks[i]);
    }
    sa.d_len = c->d_len + LEN_OP;
    TRY(dbspk::sort_cons_small_batch(c->stream, sa, false));
    TRY(read_len(c, LEN_OP, nch));
    for (int i = 0; i < nch; i++) chunks[i].n = c->h_len[LEN_OP + i];
    free_batch(c, raw);
    for (auto &sc : scratch) free_batch(c, sc);
    // batched pairwise merge rounds
    std::vector<DevBatch> cur(chunks.begin(), chunks.end());
    while (cur.size() > 1) {
        std::vector<DevBatch> next;
        MergeArgs ma{};   // tiny pairs (<= 4096): single-WG
        MergeArgs mm{};   // mid pairs (<= 32768): fixed-grid multi-WG
        std::vector<DevBatch> results;
        std::vector<int> slots;  // h_len slot per result (smalls then mids)
        std::vector<bool> ismid;
        size_t i = 0;
        for (; i + 1 < cur.size() &&
               (int)results.size() < MERGE_BATCH_MAX; i += 2) {
            DevBatch &a = cur[i], &b = cur[i + 1];
            if (a.n + b.n > 32768) break;  // fall through to merge_batches
            DevBatch res;
            bool final_round = (cur.size() == 2);
            TRY(alloc_batch(c, a.n + b.n, res, !final_round));
            MergeArgs &mx = a.n + b.n <= 4096 ? ma : mm;
            merge_pair(mx, mx.np++, a, b, res);
            ismid.push_back(&mx == &mm);
            results.push_back(res);
        }
        if (!results.empty()) {
            {
                int ps = 0, pm = ma.np;
                for (bool m : ismid) slots.push_back(m ? pm++ : ps++);
            }
            ma.d_len = c->d_len + LEN_OP;
            mm.d_len = c->d_len + LEN_OP + ma.np;
            if (ma.np > 0) TRY(dbspk::merge_small_batch(c->stream, ma, false));
            if (mm.np > 0)
                TRY(dbspk::merge_mid_batch(c->stream, mm, c->d_mid, false));
            TRY(read_len(c, LEN_OP, ma.np + mm.np));
            for (size_t p = 0; p < results.size(); p++)
                TRY(checked_len(c, LEN_OP + slots[p], results[p].n));
            for (size_t j = 0; j < 2 * results.size(); j++)
                free_batch(c, cur[j]);
            next.insert(next.end(), results.begin(), results.end());
        }
        // remaining (odd leftover or >32k pairs) via the generic path
        for (; i + 1 < cur.size(); i += 2) {
            DevBatch res;
            TRY(merge_batches(c, cur[i], cur[i + 1], res));
            free_batch(c, cur[i]);
            free_batch(c, cur[i + 1]);
            next.push_back(res);
        }
        if (i < cur.size()) next.push_back(cur[i]);  // odd carry
        cur = std::move(next);
    }
    out = cur.empty() ? DevBatch{} : cur[0];
    return DBSP_OK;
}

// sort + consolidate a RAW batch (consumes `raw`)
static dbsp_status sort_consolidate_batch(dbsp_ctx *c, DevBatch raw, DevBatch &out) {
    if (raw.n == 0) {
        free_batch(c, raw);
        out = DevBatch{};
        return DBSP_OK;
    }
    ScopedTimer t(c, 0, (double)raw.n * 48.0);
    if (raw.n > 8192) {
        // dense-range probe: a tick's delta usually covers a tiny key box
        // (q5 bids: ~4-8 ms timestamps x the ~100-auction in-flight window),
        // where a weight histogram over (krange+1)*(vrange+1) cells replaces
        // the whole sort.  Worth one extra sync only above the fused size.
        uint64_t mm[4];
        TRY(dbspk::minmax_rows(c->stream, raw, mm));
        const uint64_t kr = mm[2] - mm[0], vr = mm[3] - mm[1];
        const int64_t dense_cap =
            std::min<int64_t>((int64_t)1 << 22, 8 * raw.n);
        if (kr < (uint64_t)dense_cap && vr < (uint64_t)dense_cap &&
            (int64_t)((kr + 1) * (vr + 1)) <= dense_cap) {
            DevBatch res;
            TRY(alloc_batch(c, raw.n, res));
            TRY(dbspk::sort_cons_dense(c->stream, raw, mm[0], mm[1],
                                       (int64_t)(kr + 1), (int64_t)(vr + 1),
                                       &res));
            free_batch(c, raw);
            out = res;
            return DBSP_OK;
        }
    }
    if (raw.n > 8192 && raw.n <= 65536) return sort_medium(c, raw, out);
    DevBatch scratch;
    TRY(alloc_batch(c, raw.n, scratch, true));
    if (raw.n <= 8192) {
        // fused single-workgroup path: one launch + one length readback
        DevBatch res;
        TRY(alloc_batch(c, raw.n, res));
        SortArgs sa{};
        sa.nb = 1;
        sort_slot(sa, 0, raw, scratch, res);
        sa.d_len = c->d_len + LEN_OP;
        TRY(dbspk::sort_cons_small_batch(c->stream, sa, false));
        TRY(read_len(c, LEN_OP, 1));
        res.n = c->h_len[LEN_OP];
        free_batch(c, raw);
        free_batch(c, scratch);
        out = res;
        return DBSP_OK;
    }
    bool in_scratch = false;
    TRY(dbspk::sort_rows(c->stream, raw, scratch, &in_scratch));
    TRY(dbspk::consolidate_sorted(c->stream, in_scratch ? scratch : raw, false,
                                  &out));
    free_batch(c, raw);
    free_batch(c, scratch);
    return DBSP_OK;
}

static dbsp_status merge_batches(dbsp_ctx *c, const DevBatch &a,
                                 const DevBatch &b, DevBatch &out, bool wf64) {
    ScopedTimer t(c, 1, (double)(a.n + b.n) * 48.0);
    // three bands: tiny pairs (<= 4k) in one single-WG launch; mid pairs
    // (<= 32k) in the fixed-grid multi-WG merge (a 16k single-WG merge
    // serializes ~126 us — q4's bid spine — where merge_mid takes ~12);
    // larger through the multi-block two-pass
    if (a.n + b.n <= 32768) {
        DevBatch res;
        TRY(alloc_batch(c, a.n + b.n, res));
        MergeArgs ma{};
        ma.np = 1;
        merge_pair(ma, 0, a, b, res);
        ma.d_len = c->d_len + LEN_OP;
        if (a.n + b.n <= 4096)
            TRY(dbspk::merge_small_batch(c->stream, ma, wf64));
        else
            TRY(dbspk::merge_mid_batch(c->stream, ma, c->d_mid, wf64));
        TRY(read_len(c, LEN_OP, 1));
        TRY(checked_len(c, LEN_OP, res.n));  // fused-barrier poison
        out = res;
        return DBSP_OK;
    }
    return dbspk::merge_rows(c->stream, a, b, wf64, &out);
}

// Spine: stack of consolidated batches; invariant size[i] >= 2*size[i+1]
// (power-of-two leveling, spine_fueled.rs:107-119; merges run to completion)
struct Spine {
    std::vector<DevBatch> batches;  // largest first
    bool wf64 = false;  // f64-weighted batches (C5's weighted integral)

    int64_t total() const {
        int64_t t = 0;
        for (auto &b : batches) t += b.n;
        return t;
    }

    dbsp_status merge2(dbsp_ctx *c, const DevBatch &a, const DevBatch &b,
                       DevBatch &out) const {
        return merge_batches(c, a, b, out, wf64);
    }

    // more batches than a TraceArgs holds: merge down to one
    dbsp_status cap_batches(dbsp_ctx *c) {
        if ((int)batches.size() > MAX_TRACE_BATCHES) return consolidate_all(c);
        return DBSP_OK;
    }

    dbsp_status insert(dbsp_ctx *c, DevBatch b) {
        if (b.n == 0) {
            free_batch(c, b);
            return DBSP_OK;
        }
        batches.push_back(b);
        while (batches.size() >= 2) {
            DevBatch &top = batches[batches.size() - 1];
            DevBatch &below = batches[batches.size() - 2];
            if (top.n * 2 < below.n) break;  // geometric invariant holds
            DevBatch merged;
            TRY(merge2(c, below, top, merged));
            replace_top2(c, merged);
        }
        return DBSP_OK;
    }

    // insert a copy: the caller retains b
    dbsp_status insert_copy(dbsp_ctx *c, const DevBatch &b) {
        DevBatch cpy;
        TRY(copy_batch(c, b, cpy));
        return insert(c, cpy);
    }

    // exhaustive merge to a single batch (consolidate.rs:33-47 semantics)
    dbsp_status consolidate_all(dbsp_ctx *c) {
        while (batches.size() >= 2) {
            DevBatch merged;
            TRY(merge2(c, batches[batches.size() - 2], batches.back(), merged));
            replace_top2(c, merged);
        }
        return DBSP_OK;
    }

    // the two topmost batches give way to their merge (dropped when empty).
    // A q3 probe in flight on the back stream may still read them: whatever
    // recycles their blocks runs behind the join (free when none is).
    void replace_top2(dbsp_ctx *c, DevBatch merged) {
        q3_join_back(c);
        free_batch(c, batches.back());
        batches.pop_back();
        free_batch(c, batches.back());
        batches.pop_back();
        if (merged.n > 0)
            batches.push_back(merged);
        else
            free_batch(c, merged);
    }

    void clear(dbsp_ctx *c) {
        for (auto &b : batches) free_batch(c, b);
        batches.clear();
    }
};

// a spine's non-empty batches as a kernel argument
static TraceArgs trace_args_of(const Spine &sp) {
    TraceArgs t{};
    for (auto &b : sp.batches)
        if (b.n != 0) trace_push(t, b);
    return t;
}

// Incremental partitioned rolling aggregate with the linear weight-sum
// aggregator (PartitionedRollingAggregate::eval, operator/time_series/
// rolling_aggregate.rs:487-604; range_of(ts) = [ts - before, ts + after],
// RelRange::new(Before(before), After(after)), range.rs:93-104).
// in_sp is the input integral INCLUDING the current tick, out_sp the integral
// of this operator's own outputs EXCLUDING it.  step() is defined below the
// spine helpers it uses.
//
// agg (fixed at creation) selects the aggregator.  DBSP_ROLL_SUM: rows
// (partition, ts, w), the value weighed into w.  DBSP_ROLL_MAX / _MIN
// (partitioned_rolling_aggregate<TS, V, Agg>, rolling_aggregate.rs:235-321;
// aggregate/max.rs:36-55, min.rs:38-57): rows (partition, ts << 32 | val, w),
// one output per time holding a row of w > 0, its value the extreme val of
// ANY non-zero weight over range_of(ts).  The output rows have the sum's
// form, so out_sp, its retraction gather and its sweep are shared.
struct RollingOp {
    uint64_t before = 10000, after = 0;
    dbsp_roll_agg agg = DBSP_ROLL_SUM;
    Spine in_sp, out_sp;

    bool time_hi() const { return agg != DBSP_ROLL_SUM; }  // time = v >> 32
    // in_sp's range-gather and truncation mode (out_sp's is always 1)
    int in_mode() const { return time_hi() ? 2 : 0; }

    // delta: consolidated rows (partition, ts, w), retained by the caller;
    // out: the tick's consolidated output delta (p<<32|ts, sum, +-1).
    // DBSP_ERR_INVALID (state unchanged) if a partition or time is >= 2^32.
    dbsp_status step(dbsp_ctx *c, const DevBatch &delta, DevBatch &out);

    // Watermark-bounded state (partitioned_rolling_aggregate_with_watermark,
    // rolling_aggregate.rs:155-220 and :286-321).  wm only grows; both
    // spines may drop their rows below lower_bound() = wm - (before + after):
    // a row at ts >= wm affects times >= wm - after, whose sums and
    // retractions read nothing below the bound.
    // A sweep is a few launches plus a length sync, not worth it for fewer
    // dead rows than this; the break-even has not been measured.
    static constexpr int64_t SWEEP_FLOOR = 4096;
    uint64_t wm = 0;
    int64_t late_rows = 0, sweeps = 0;
    int64_t in_live = 0, out_live = 0;  // rows after each spine's last sweep

    static uint64_t bound_of(uint64_t wm_, uint64_t before_, uint64_t after_) {
        const uint64_t both = before_ + after_;
        if (both < before_ || both > wm_) return 0;
        return wm_ - both;
    }
    uint64_t lower_bound() const { return bound_of(wm, before, after); }

    // step() with the watermark raised to max(wm, x) first.  Delta rows
    // below the new watermark are dropped whole and counted in late_rows
    // (the reference only "does not expect" them, rolling_aggregate.rs
    // :126-129; dropping is this operator's choice).  On DBSP_ERR_INVALID
    // nothing changes, the watermark and the counters included.
    dbsp_status step_wm(dbsp_ctx *c, const DevBatch &delta, uint64_t x,
                        DevBatch &out);
    // sweep one spine at lower_bound(): mode 0 = in_sp, 1 = out_sp
    dbsp_status sweep(dbsp_ctx *c, int mode);
    // sweep the spines that outgrew 2 * live + SWEEP_FLOOR
    dbsp_status sweep_policy(dbsp_ctx *c);

    void clear(dbsp_ctx *c) {
        in_sp.clear(c);
        out_sp.clear(c);
    }
};

// Incremental top-K per group: the last min(K, present rows) present rows of
// every group in (k, v) order, each at weight +1, kept up to date (the
// aggregate(Fold) + flat_map of crates/nexmark/src/queries/q19.rs; SQL's
// ROW_NUMBER() OVER (PARTITION BY g ORDER BY x DESC) <= K).  A row's group is
// k >> group_shift; a row is present iff its total weight in the input
// integral is non-zero, negative totals included (aggregate/fold.rs:83-92).
// in_sp is the input integral, out_sp the integral of this operator's own
// outputs EXCLUDING the current tick; step() is defined below the spine
// helpers it uses.
struct TopKOp {
    int64_t K = 10;
    int group_shift = 0;
    bool refill_all = false;  // DBSP_TOPK_REFILL_ALL
    Spine in_sp, out_sp;
    // cumulative: affected groups, groups sent down the refill path, rows the
    // refill gather copied out of in_sp
    int64_t groups_seen = 0, groups_refilled = 0, rows_gathered = 0;

    // delta: consolidated rows, retained by the caller; out: the tick's
    // consolidated output delta (k, v, +-1).  Any (k, v) is valid.
    dbsp_status step(dbsp_ctx *c, const DevBatch &delta, DevBatch &out);

    void clear(dbsp_ctx *c) {
        in_sp.clear(c);
        out_sp.clear(c);
    }
};

// Incremental antijoin / semijoin: A restricted to the keys absent from
// (DBSP_ANTIJOIN) or present in (DBSP_SEMIJOIN) a key set B, kept up to date
// (Stream::antijoin, operator/join.rs:294-320, which composes it as
// A - A |><| distinct(B); the semijoin is the subtracted term, join.rs:313).
// A key is present iff its total weight in the integral of B is > 0
// (operator/distinct.rs).  a_sp is the integral of A, b_sp the integral of
// B's keys as rows (k, 0, w), both EXCLUDING the current tick on entry;
// step() is defined below the spine helpers it uses.
struct AntiJoinOp {
    bool anti = true;  // DBSP_ANTIJOIN
    Spine a_sp, b_sp;
    // cumulative: keys whose presence flipped, rows of the A integral
    // (consolidated) that a flip re-emitted, delta rows the filter dropped
    int64_t keys_flipped = 0, rows_gathered = 0, rows_filtered = 0;

    // da: consolidated rows, db: consolidated key rows (k, 0, w); both
    // retained by the caller, either may be empty.  out: the tick's
    // consolidated output delta.  Any row and any key is valid.
    dbsp_status step(dbsp_ctx *c, const DevBatch &da, const DevBatch &db,
                     DevBatch &out);

    void clear(dbsp_ctx *c) {
        a_sp.clear(c);
        b_sp.clear(c);
    }
};

// Incremental arg-max per group, ties kept: for every group with a present
// row, all present rows whose rank is the group's largest present rank, each
// at its own integral weight, kept up to date (the tail of
// crates/nexmark/src/queries/q7.rs:82-93, aggregate(Min) over the negated
// price joined back on the price; SQL's RANK() OVER (PARTITION BY g ORDER BY
// x DESC) = 1).  A row's group is k >> group_shift, its rank k >> rank_shift
// (rank_shift <= group_shift); presence is top-K's rule, per row.  One
// divergence: Min::aggregate (operator/aggregate/min.rs:38-57) sums the
// weights of all rows sharing a price and skips a price whose sum is zero,
// while here a rank is present as long as one row at it is; the two differ
// only when different rows at one rank carry weights of mixed sign that
// cancel, never on positive weights.  in_sp is the input integral, out_sp
// the integral of this operator's own outputs EXCLUDING the current tick;
// step() is defined at the end of this file.
struct ArgMaxOp {
    int group_shift = 0, rank_shift = 0;
    bool refill_all = false;  // DBSP_ARGMAX_REFILL_ALL
    Spine in_sp, out_sp;
    // cumulative: affected groups, groups sent down the refill path, rows the
    // refill gather copied out of in_sp
    int64_t groups_seen = 0, groups_refilled = 0, rows_gathered = 0;

    // delta: consolidated rows, retained by the caller; out: the tick's
    // consolidated output delta.  Any (k, v) is valid.
    dbsp_status step(dbsp_ctx *c, const DevBatch &delta, DevBatch &out);

    void clear(dbsp_ctx *c) {
        in_sp.clear(c);
        out_sp.clear(c);
    }
};

// ---- pieces of the keyed-aggregate stage, shared with their test probes ----

// The small join route (delta.n <= 8192): probe and single-workgroup scan,
// the match total read back, then the emit over the prepared counts.  out
// stays empty when nothing matches.
static dbsp_status join_small(dbsp_ctx *c, const DevBatch &delta,
                              const TraceArgs &t, int proj, uint64_t param,
                              bool transient, DevBatch &out) {
    ScratchBuf cnts, offsets;
    TRY(cnts.alloc(c, (size_t)delta.n * t.nb * 4 + 8, transient));
    TRY(offsets.alloc(c, (size_t)(delta.n + 1) * 8, transient));
    JoinCountArgs jca{};
    jca.np = 1;
    jca.dk[0] = delta.k;
    jca.nd[0] = delta.n;
    jca.t[0] = t;
    jca.cnts[0] = cnts.as<uint32_t>();
    jca.offsets[0] = offsets.as<uint64_t>();
    jca.d_total = c->d_len + LEN_OP;
    TRY(dbspk::join_count_scan_batch(c->stream, jca));
    TRY(read_len(c, LEN_OP, 1));
    int64_t total = 0;
    TRY(checked_len(c, LEN_OP, total));  // fused-barrier poison
    if (total == 0) return DBSP_OK;
    TRY(alloc_batch(c, total, out, transient));
    dbsp_status st = dbspk::join_emit_prepared(
        c->stream, delta, t, cnts.as<uint32_t>(), offsets.as<uint64_t>(),
        total, proj, param, out);
    if (st != DBSP_OK) free_batch(c, out);
    return st;
}

// Per-key weight sums of keys[nk] across the nb batches, one accumulator
// summed batch by batch (an empty batch keeps its turn), then the
// ticket-ordered emit of (key, sum, +1) for the non-zero sums into ins.
// wf64: f64 weights, the sums travel as bit patterns.
static dbsp_status agg_sum_emit(dbsp_ctx *c, const uint64_t *keys, int64_t nk,
                                const DevBatch *batches, int nb, bool wf64,
                                bool transient, DevBatch &ins) {
    ScratchBuf acc;
    TRY(acc.alloc(c, nk * 8 + 8));
    HIP_CHECK_ST(hipMemsetAsync(acc.p, 0, nk * 8, c->stream));
    for (int b = 0; b < nb; b++)
        TRY(dbspk::agg_sum_batch(c->stream, keys, nk, batches[b],
                                 acc.as<int64_t>(), wf64));
    TRY(alloc_batch(c, nk, ins, transient));
    dbsp_status st = dbspk::emit_nonzero(c->stream, keys, acc.as<int64_t>(),
                                         nk, wf64, &ins);
    if (st != DBSP_OK) free_batch(c, ins);
    return st;
}

// ---------------------------------------------------------------------------
// kernel-level C ABI (device-pointer primitives; used by GPU parity tests)
// ---------------------------------------------------------------------------

extern "C" dbsp_status dbsp_sort_consolidate(dbsp_ctx *c, const uint64_t *k_in,
                                             const uint64_t *v_in,
                                             const int64_t *w_in, int64_t n,
                                             dbsp_batch *out) {
    DevBatch raw;
    TRY(alloc_batch(c, n, raw));
    TRY(copy_cols(c, raw, 0, k_in, v_in, w_in, n));
    DevBatch res;
    TRY(sort_consolidate_batch(c, raw, res));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_merge(dbsp_ctx *c, const dbsp_batch *a,
                                  const dbsp_batch *b, dbsp_batch *out) {
    DevBatch res;
    TRY(merge_batches(c, as_batch(a), as_batch(b), res));
    TRY(dbsp_ctx_sync(c));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_acc_fold(dbsp_ctx *c, const dbsp_batch *acc,
                                     const dbsp_batch *delta, dbsp_batch *out) {
    const DevBatch a = as_batch(acc), b = as_batch(delta);
    if (a.n < 0 || b.n > 8192) return DBSP_ERR_INVALID;
    // the delta length travels through a device slot, verbatim, as the
    // train's does (a negative one is the poison the fold must pass on)
    const int64_t bcap = b.n > 0 ? b.n : 0;
    DevBatch res;
    TRY(alloc_batch(c, a.n + bcap, res));
    c->h_len[LEN_OP] = b.n;
    HIP_CHECK_ST(hipMemcpyAsync(c->d_len + LEN_OP, c->h_len + LEN_OP,
                                sizeof(int64_t), hipMemcpyHostToDevice,
                                c->stream));
    MergeArgs ma{};
    ma.np = 1;
    merge_pair(ma, 0, a, b, res, c->d_len + LEN_OP, bcap);
    ma.d_len = c->d_len + LEN_OP + 1;
    dbsp_status st;
    {
        ScopedTimer t(c, 1, (double)(a.n + bcap) * 48.0);
        st = dbspk::acc_fold_batch(c->stream, ma, false);
    }
    if (st == DBSP_OK) st = read_len(c, LEN_OP + 1, 1);
    if (st == DBSP_OK) st = checked_len(c, LEN_OP + 1, res.n);
    if (st != DBSP_OK) {
        free_batch(c, res);
        return st;
    }
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_join(dbsp_ctx *c, const dbsp_batch *delta,
                                 const dbsp_batch *trace, dbsp_proj proj,
                                 uint64_t param, dbsp_batch *out) {
    DevBatch res;
    {
        ScopedTimer t(c, 2, (double)delta->len * 24.0);
        TRY(dbspk::join_rows(c->stream, as_batch(delta), as_batch(trace), proj,
                             param, &res));
    }
    put_batch(out, res);
    return DBSP_OK;
}

// the spine of a test-facing join: every batch keeps its slot, empty or not
static dbsp_status trace_verbatim(const dbsp_batch *batches, int n,
                                  TraceArgs &t) {
    if (n < 0 || n > MAX_TRACE_BATCHES || (n > 0 && !batches))
        return DBSP_ERR_INVALID;
    t = TraceArgs{};
    for (int i = 0; i < n; i++) {
        if (batches[i].len < 0) return DBSP_ERR_INVALID;
        trace_push(t, as_batch(&batches[i]));
    }
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_join_spine(dbsp_ctx *c, const dbsp_batch *delta,
                                       const dbsp_batch *trace_batches,
                                       int n_batches, dbsp_proj proj,
                                       uint64_t param, int path,
                                       dbsp_batch *out) {
    const DevBatch d = as_batch(delta);
    TraceArgs t;
    TRY(trace_verbatim(trace_batches, n_batches, t));
    if (d.n < 0 || (path != 1 && path != 2)) return DBSP_ERR_INVALID;
    if (path == 2 && d.n > 8192) return DBSP_ERR_INVALID;
    DevBatch res;
    if (path == 1 || t.nb == 0)
        TRY(dbspk::join_spine_rows(c->stream, d, t, proj, param, &res));
    else
        TRY(join_small(c, d, t, proj, param, /*transient=*/false, res));
    TRY(dbsp_ctx_sync(c));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_join_tail(dbsp_ctx *c, const dbsp_join_plan *plans,
                                      int np, int64_t cap, int64_t *verdict,
                                      uint64_t *const *offsets_host,
                                      dbsp_batch *out) {
    if (np < 1 || np > 3 || cap < 8192 || !plans || !verdict || !offsets_host)
        return DBSP_ERR_INVALID;
    // device length slots: [0..2] nd, [3..5] tn, [6..8] totals, [9] d_total,
    // [10] d_flag, [11] d_final
    enum { S_ND = 0, S_TN = 3, S_TOT = 6, S_TOTAL = 9, S_FLAG = 10,
           S_FINAL = 11, S_N = 12 };
    int64_t h[S_N] = {};
    JoinCountArgs jca{};
    JoinTailArgs ta{};
    jca.np = ta.np = np;
    for (int p = 0; p < np; p++) {
        const dbsp_join_plan &pl = plans[p];
        if (pl.delta.len < 0 || pl.n_batches < 1) return DBSP_ERR_INVALID;
        TRY(trace_verbatim(pl.trace_batches, pl.n_batches, jca.t[p]));
        // a length the kernels accept must lie inside the columns
        if (pl.nd >= 0 && pl.nd <= 8192 && pl.nd > pl.delta.len)
            return DBSP_ERR_INVALID;
        if (pl.fresh) {
            if (pl.n_batches != 1 || pl.tn > pl.trace_batches[0].len)
                return DBSP_ERR_INVALID;
            jca.t[p].n[0] = 0;  // read from the device, as a chained tick's
        }
        h[S_ND + p] = pl.nd;
        h[S_TN + p] = pl.fresh ? pl.tn : 0;
    }
    int64_t *slots = nullptr;
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&slots, S_N * 8, c->stream));
    HIP_CHECK_ST(hipMemcpyAsync(slots, h, S_N * 8, hipMemcpyHostToDevice,
                                c->stream));
    std::vector<void *> bufs{slots};
    auto release = [&]() {
        for (void *b : bufs) (void)dbspk::cache_free(b, c->stream);
    };
    dbsp_status st = DBSP_OK;
    for (int p = 0; p < np && st == DBSP_OK; p++) {
        const dbsp_join_plan &pl = plans[p];
        const size_t n_cap = (size_t)pl.delta.len, nb = (size_t)pl.n_batches;
        void *cn = nullptr, *of = nullptr, *sp = nullptr;
        if (dbspk::cache_malloc(&cn, n_cap * nb * 4 + 8, c->stream) !=
                hipSuccess ||
            dbspk::cache_malloc(&of, (n_cap + 1) * 8, c->stream) !=
                hipSuccess ||
            dbspk::cache_malloc(&sp, n_cap * nb * 8 + 8, c->stream) !=
                hipSuccess)
            st = DBSP_ERR_OOM;
        for (void *b : {cn, of, sp})
            if (b) bufs.push_back(b);
        jca.dk[p] = ta.dk[p] = pl.delta.k;
        ta.dv[p] = pl.delta.v;
        ta.dw[p] = pl.delta.w;
        jca.nd[p] = 0;
        jca.nd_dev[p] = ta.nd_dev[p] = slots + S_ND + p;
        jca.tn_dev[p] = ta.tn_dev[p] = pl.fresh ? slots + S_TN + p : nullptr;
        ta.t[p] = jca.t[p];
        jca.cnts[p] = (uint32_t *)cn;
        ta.cnts[p] = (const uint32_t *)cn;
        jca.starts[p] = (int64_t *)sp;
        ta.starts[p] = (const int64_t *)sp;
        jca.offsets[p] = ta.offsets[p] = (uint64_t *)of;
        ta.proj[p] = pl.proj;
    }
    DevBatch comb, scr, store;
    if (st == DBSP_OK) st = alloc_batch(c, cap, comb);
    if (st == DBSP_OK) st = alloc_batch(c, 8192, scr);
    if (st == DBSP_OK) st = alloc_batch(c, 8192, store);
    jca.d_total = slots + S_TOT;
    ta.totals = slots + S_TOT;
    ta.cap = cap;
    ta.d_total = slots + S_TOTAL;
    ta.d_flag = slots + S_FLAG;
    ta.d_final = slots + S_FINAL;
    ta.ek = comb.k; ta.ev = comb.v; ta.ew = comb.w;
    ta.tk = scr.k; ta.tv = scr.v; ta.tw = scr.w;
    ta.ok = store.k; ta.ov = store.v; ta.ow = store.w;
    if (st == DBSP_OK) st = dbspk::join_probe_batch(c->stream, jca);
    if (st == DBSP_OK) st = dbspk::join_tail_small(c->stream, ta);
    if (st == DBSP_OK &&
        hipMemcpyAsync(h, slots, S_N * 8, hipMemcpyDeviceToHost, c->stream) !=
            hipSuccess)
        st = DBSP_ERR_INTERNAL;
    if (st == DBSP_OK) st = dbsp_ctx_sync(c);
    for (int p = 0; p < np && st == DBSP_OK; p++) {
        if (h[S_TOT + p] < 0 || plans[p].nd <= 0) continue;
        if (!offsets_host[p]) {
            st = DBSP_ERR_INVALID;
        } else if (hipMemcpyAsync(offsets_host[p], ta.offsets[p],
                                  (size_t)plans[p].nd * 8,
                                  hipMemcpyDeviceToHost,
                                  c->stream) != hipSuccess) {
            st = DBSP_ERR_INTERNAL;
        }
    }
    if (st == DBSP_OK) st = dbsp_ctx_sync(c);
    free_batch(c, scr);
    release();
    DevBatch res;
    if (st == DBSP_OK) {
        for (int i = 0; i < 3; i++) verdict[i] = i < np ? h[S_TOT + i] : 0;
        verdict[3] = h[S_TOTAL];
        verdict[4] = h[S_FLAG];
        verdict[5] = h[S_FINAL];
        if (h[S_FINAL] >= 0 && h[S_FINAL] <= 8192) {
            std::swap(res, store);
            res.n = h[S_FINAL];
        } else if (h[S_FINAL] < 0 && h[S_FLAG] == 0 && h[S_TOTAL] >= 0 &&
                   h[S_TOTAL] <= cap) {
            std::swap(res, comb);
            res.n = h[S_TOTAL];
        }
    }
    free_batch(c, comb);
    free_batch(c, store);
    if (st != DBSP_OK) return st;
    put_batch(out, res);
    return DBSP_OK;
}

// Radix-tree rolling aggregate primitive (operator/time_series/radix_tree/
// + rolling_aggregate.rs:235-280): per input row
// (partition, ts, w) of a consolidated (partition, time)-sorted batch, the
// weight sum over that partition's rows with time in [ts - width, ts]
// (RelRange(Before(width), Before(0)).range_of, range.rs:93-110).  Built on
// a flat radix-16 prefix-aggregate tree over the row array — the GPU-native
// form of the reference's per-prefix aggregate nodes.
extern "C" dbsp_status dbsp_rolling_agg(dbsp_ctx *c, const dbsp_batch *in,
                                        uint64_t width, dbsp_batch *out) {
    DevBatch res;
    TRY(alloc_batch(c, in->len > 0 ? in->len : 1, res));
    {
        ScopedTimer t(c, 3, 0.0);
        TRY(dbspk::rolling_agg_rows(c->stream, as_batch(in), width, res));
    }
    res.n = in->len;
    put_batch(out, res);
    return DBSP_OK;
}

static dbsp_status agg_upsert(dbsp_ctx *c, dbspk::AggMode mode,
                              const uint64_t *delta_keys, int64_t nd,
                              const dbsp_batch *in_trace,
                              const dbsp_batch *out_trace, dbsp_batch *out) {
    DevBatch res;
    TRY(dbspk::agg_upsert_rows(c->stream, mode, delta_keys, nd,
                               as_batch(in_trace), as_batch(out_trace), &res));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_agg_linear_upsert(dbsp_ctx *c,
                                              const uint64_t *delta_keys,
                                              int64_t nd,
                                              const dbsp_batch *in_trace,
                                              const dbsp_batch *out_trace,
                                              dbsp_batch *out) {
    return agg_upsert(c, dbspk::AGG_LINEAR, delta_keys, nd, in_trace,
                      out_trace, out);
}

extern "C" dbsp_status dbsp_agg_max_upsert(dbsp_ctx *c,
                                           const uint64_t *delta_keys,
                                           int64_t nd,
                                           const dbsp_batch *in_trace,
                                           const dbsp_batch *out_trace,
                                           dbsp_batch *out) {
    return agg_upsert(c, dbspk::AGG_MAX, delta_keys, nd, in_trace, out_trace,
                      out);
}

extern "C" dbsp_status dbsp_agg_last10_upsert(dbsp_ctx *c,
                                              const uint64_t *delta_keys,
                                              int64_t nd,
                                              const dbsp_batch *in_trace,
                                              const dbsp_batch *out_trace,
                                              dbsp_batch *out) {
    return agg_upsert(c, dbspk::AGG_LAST10, delta_keys, nd, in_trace,
                      out_trace, out);
}

// the insert half of agg_linear_spine on its own; the unique keys go to the
// caller, who frees them
extern "C" dbsp_status dbsp_agg_sum_spine(dbsp_ctx *c, const dbsp_batch *delta,
                                          const dbsp_batch *in_batches,
                                          int n_batches, uint64_t **out_keys,
                                          int64_t *n_keys, dbsp_batch *out) {
    TraceArgs t;
    TRY(trace_verbatim(in_batches, n_batches, t));
    if (delta->len < 0 || !out_keys || !n_keys) return DBSP_ERR_INVALID;
    *out_keys = nullptr;
    *n_keys = 0;
    uint64_t *k = nullptr;
    int64_t nk = 0;
    TRY(dbspk::unique_keys(c->stream, delta->k, delta->len, &k, &nk));
    ScratchBuf keys(c, k);
    DevBatch ins;
    if (nk > 0) {
        std::vector<DevBatch> batches;
        for (int b = 0; b < n_batches; b++)
            batches.push_back(as_batch(&in_batches[b]));
        TRY(agg_sum_emit(c, k, nk, batches.data(), n_batches, false,
                         /*transient=*/false, ins));
    }
    TRY(dbsp_ctx_sync(c));
    *out_keys = (uint64_t *)keys.release();
    *n_keys = nk;
    put_batch(out, ins);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_shard_partition(dbsp_ctx *c, const dbsp_batch *in,
                                            int nshards, dbsp_batch *out,
                                            int64_t *offsets_host) {
    DevBatch res;
    TRY(alloc_batch(c, in->len, res));
    TRY(dbspk::shard_rows(c->stream, as_batch(in), nshards, res, offsets_host));
    put_batch(out, res);
    return DBSP_OK;
}

// ---- f64-weight C ABI (config C5) ----

extern "C" dbsp_status dbsp_sort_consolidate_f64(dbsp_ctx *c,
                                                 const uint64_t *k_in,
                                                 const uint64_t *v_in,
                                                 const double *w_in, int64_t n,
                                                 dbsp_batch *out) {
    DevBatch raw;
    TRY(alloc_batch(c, n > 0 ? n : 1, raw, true));
    TRY(copy_cols(c, raw, 0, k_in, v_in, w_in, n));
    raw.n = n;
    if (n == 0) {
        put_batch(out, DevBatch{});
        return DBSP_OK;
    }
    if (n <= 8192) {
        DevBatch scratch, res;
        TRY(alloc_batch(c, n, scratch, true));
        TRY(alloc_batch(c, n, res));
        SortArgs sa{};
        sa.nb = 1;
        sort_slot(sa, 0, raw, scratch, res);
        sa.d_len = c->d_len + LEN_OP;
        TRY(dbspk::sort_cons_small_batch(c->stream, sa, true));
        TRY(read_len(c, LEN_OP, 1));
        res.n = c->h_len[LEN_OP];
        put_batch(out, res);
        return DBSP_OK;
    }
    // big path: the radix sort moves the weight column bitwise; the
    // consolidate uses the deterministic segmented tree
    DevBatch scratch;
    TRY(alloc_batch(c, n, scratch, true));
    bool in_scratch = false;
    TRY(dbspk::sort_rows(c->stream, raw, scratch, &in_scratch));
    DevBatch res;
    TRY(dbspk::consolidate_sorted(c->stream, in_scratch ? scratch : raw, true,
                                  &res));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_merge_f64(dbsp_ctx *c, const dbsp_batch *a,
                                      const dbsp_batch *b, dbsp_batch *out) {
    // the same three-band dispatch the C5 weighted-integral spine takes
    DevBatch res;
    TRY(merge_batches(c, as_batch(a), as_batch(b), res, /*wf64=*/true));
    TRY(dbsp_ctx_sync(c));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_weigh_f64(dbsp_ctx *c, const dbsp_batch *in,
                                      dbsp_batch *out) {
    DevBatch res;
    TRY(alloc_batch(c, in->len > 0 ? in->len : 1, res));
    TRY(dbspk::map_rows(c->stream, as_batch(in), 4, res));
    res.n = in->len;
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_agg_linear_upsert_f64(dbsp_ctx *c,
                                                  const uint64_t *delta_keys,
                                                  int64_t nd,
                                                  const dbsp_batch *in_trace,
                                                  const dbsp_batch *out_trace,
                                                  dbsp_batch *out) {
    if (nd == 0) {
        put_batch(out, DevBatch{});
        return DBSP_OK;
    }
    const DevBatch in = as_batch(in_trace);
    DevBatch ins;
    TRY(agg_sum_emit(c, delta_keys, nd, &in, 1, /*wf64=*/true,
                     /*transient=*/true, ins));
    // retractions against the (i64-weighted) output trace
    DevBatch retr;
    TRY(dbspk::agg_upsert_rows(c->stream, dbspk::AGG_LINEAR, delta_keys, nd,
                               DevBatch{}, as_batch(out_trace), &retr));
    DevBatch res;
    TRY(alloc_batch(c, ins.n + retr.n, res));
    TRY(copy_cols(c, res, 0, ins.k, ins.v, ins.w, ins.n));
    TRY(copy_cols(c, res, ins.n, retr.k, retr.v, retr.w, retr.n));
    free_batch(c, ins);
    free_batch(c, retr);
    TRY(dbsp_ctx_sync(c));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_distinct_inc(dbsp_ctx *c, const dbsp_batch *delta,
                                         const dbsp_batch *trace_batches,
                                         int n_batches, dbsp_batch *out) {
    if (n_batches > MAX_TRACE_BATCHES) return DBSP_ERR_INVALID;
    TraceArgs t{};
    for (int i = 0; i < n_batches; i++)
        if (trace_batches[i].len != 0) trace_push(t, as_batch(&trace_batches[i]));
    DevBatch res;
    TRY(dbspk::distinct_inc_rows(c->stream, as_batch(delta), t, &res));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_unique_keys(dbsp_ctx *c, const dbsp_batch *in,
                                        uint64_t **out_keys, int64_t *n_out) {
    TRY(dbspk::unique_keys(c->stream, in->k, in->len, out_keys, n_out));
    TRY(dbsp_ctx_sync(c));
    return DBSP_OK;
}

extern "C" uint64_t dbsp_xxh3_u64(uint64_t key, uint64_t seed) {
    return dbspk::host_xxh3_u64(key, seed);
}

// ---------------------------------------------------------------------------
// RCCL exchange (replaces exchange.rs:45-251 over xGMI)
// ---------------------------------------------------------------------------

extern "C" dbsp_status dbsp_comm_unique_id(void *out128) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return DBSP_ERR_INTERNAL;
    memcpy(out128, &id, sizeof(id));
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_comm_init(dbsp_ctx *c, int rank, int world,
                                      const void *nccl_id) {
    // host-side count/offset arrays are sized for one node's worth of ranks
    if (world < 1 || world > 64 || rank < 0 || rank >= world)
        return DBSP_ERR_INVALID;
    ncclUniqueId id;
    memcpy(&id, nccl_id, sizeof(id));
    if (ncclCommInitRank(&c->comm, world, id, rank) != ncclSuccess)
        return DBSP_ERR_INTERNAL;
    c->rank = rank;
    c->world = world;
    return DBSP_OK;
}

// all-to-all-v of the three row columns; counts exchanged first
static dbsp_status alltoallv_cols(dbsp_ctx *c, const DevBatch &send,
                                  const int64_t *send_counts, DevBatch &recv,
                                  int64_t *recv_counts) {
    int world = c->world;
    // exchange counts (device staging for RCCL)
    // ONE allgather of every rank's send-count vector beats a grouped
    // world^2 send/recv mesh on setup latency; rank p's row holds what p
    // sends to each peer, so what WE receive from p is row[p][rank]
    int64_t *d_send_cnt, *d_all_cnt;
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&d_send_cnt, world * 8, c->stream));
    HIP_CHECK_ST(
        dbspk::cache_malloc((void **)&d_all_cnt, (size_t)world * world * 8,
                            c->stream));
    HIP_CHECK_ST(hipMemcpyAsync(d_send_cnt, send_counts, world * 8,
                                hipMemcpyHostToDevice, c->stream));
    if (ncclAllGather(d_send_cnt, d_all_cnt, world, ncclInt64, c->comm,
                      c->stream) != ncclSuccess)
        return DBSP_ERR_INTERNAL;
    int64_t h_all[64 * 64];
    HIP_CHECK_ST(hipMemcpyAsync(h_all, d_all_cnt, (size_t)world * world * 8,
                                hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    int64_t recv_total = 0;
    for (int r = 0; r < world; r++) {
        recv_counts[r] = h_all[(size_t)r * world + c->rank];
        recv_total += recv_counts[r];
    }
    TRY(alloc_batch(c, recv_total, recv));
    // data columns
    int64_t soff = 0, roff = 0;
    ncclGroupStart();
    soff = 0; roff = 0;
    for (int r = 0; r < world; r++) {
        if (send_counts[r] > 0) {
            ncclSend(send.k + soff, send_counts[r], ncclUint64, r, c->comm, c->stream);
            ncclSend(send.v + soff, send_counts[r], ncclUint64, r, c->comm, c->stream);
            ncclSend(send.w + soff, send_counts[r], ncclInt64, r, c->comm, c->stream);
        }
        if (recv_counts[r] > 0) {
            ncclRecv(recv.k + roff, recv_counts[r], ncclUint64, r, c->comm, c->stream);
            ncclRecv(recv.v + roff, recv_counts[r], ncclUint64, r, c->comm, c->stream);
            ncclRecv(recv.w + roff, recv_counts[r], ncclInt64, r, c->comm, c->stream);
        }
        soff += send_counts[r];
        roff += recv_counts[r];
    }
    ncclGroupEnd();
    HIP_CHECK_ST(dbspk::cache_free(d_send_cnt, c->stream));
    HIP_CHECK_ST(dbspk::cache_free(d_all_cnt, c->stream));
    recv.n = recv_total;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_comm_alltoallv(dbsp_ctx *c, const dbsp_batch *send,
                                           const int64_t *send_counts,
                                           dbsp_batch *recv, int64_t recv_cap,
                                           int64_t *recv_counts_host) {
    (void)recv_cap;
    DevBatch s{send->k, send->v, send->w, send->len};
    DevBatch r;
    TRY(alltoallv_cols(c, s, send_counts, r, recv_counts_host));
    recv->k = r.k; recv->v = r.v; recv->w = r.w; recv->len = r.n;
    return DBSP_OK;
}

static inline bool sharding_on(dbsp_ctx *c) {
    return c->world > 1 || (c->force_shard && c->comm);
}

// shard + exchange + rebuild: the full shard() operator
// (shard.rs:88-199: hash-split, exchange, re-consolidate).  hint > 0
// enables the fixed-frame fast path (see shard_exchange_pair below).
static dbsp_status shard_exchange(dbsp_ctx *c, DevBatch local, DevBatch &out,
                                  int64_t hint = 0) {
    if (!sharding_on(c)) {
        out = local;
        return DBSP_OK;
    }
    DevBatch parts;
    TRY(alloc_batch(c, local.n, parts));
    int64_t offsets[65];
    TRY(dbspk::shard_rows(c->stream, local, c->world, parts, offsets));
    free_batch(c, local);
    if (hint > 0 && c->world <= 8 && c->comm) {
        const int64_t P = 2 * hint / c->world + 512;
        const int64_t S = 2 + 3 * P + 3;  // degenerate pair: stream1 cap 1
        uint64_t *fsend, *frecv;
        HIP_CHECK_ST(dbspk::cache_malloc((void **)&fsend,
                                         (size_t)c->world * S * 8, c->stream));
        HIP_CHECK_ST(dbspk::cache_malloc((void **)&frecv,
                                         (size_t)c->world * S * 8, c->stream));
        dbspk::FramePairArgs fa{};
        fa.p0k = parts.k; fa.p0v = parts.v; fa.p0w = parts.w;
        fa.p1k = parts.k; fa.p1v = parts.v; fa.p1w = parts.w;
        for (int r = 0; r <= c->world; r++) {
            fa.off0[r] = offsets[r];
            fa.off1[r] = 0;  // empty stream1
        }
        fa.world = c->world;
        fa.P0 = P;
        fa.P1 = 1;
        fa.frame = fsend;
        TRY(dbspk::frames_pack_pair(c->stream, fa));
        if (ncclAllToAll(fsend, frecv, (size_t)S, ncclUint64, c->comm,
                         c->stream) != ncclSuccess)
            return DBSP_ERR_INTERNAL;
        DevBatch r0, r1;
        TRY(alloc_batch(c, c->world * P, r0, true));
        TRY(alloc_batch(c, c->world, r1, true));
        TRY(dbspk::frames_unpack_pair(c->stream, frecv, c->world, P, 1, r0, r1,
                                      c->d_len + L_XCHG,
                                      c->d_len + L_XCHG + 1));
        TRY(read_len(c, L_XCHG, 2));
        HIP_CHECK_ST(dbspk::cache_free(fsend, c->stream));
        HIP_CHECK_ST(dbspk::cache_free(frecv, c->stream));
        if (c->h_len[L_XCHG] >= 0) {
            r0.n = c->h_len[L_XCHG];
            free_batch(c, parts);
            TRY(sort_consolidate_batch(c, r0, out));
            return DBSP_OK;
        }
        // overflow sentinel: dynamic replay below (all ranks together)
    }
    int64_t send_counts[64];
    for (int r = 0; r < c->world; r++) send_counts[r] = offsets[r + 1] - offsets[r];
    DevBatch recv;
    int64_t recv_counts[64];
    TRY(alltoallv_cols(c, parts, send_counts, recv, recv_counts));
    free_batch(c, parts);
    TRY(sort_consolidate_batch(c, recv, out));
    return DBSP_OK;
}

// ---------------------------------------------------------------------------
// engine: per-query operator DAGs (mirrors nexmark/src/queries/q{0,3,5,8}.rs)
// ---------------------------------------------------------------------------

struct Q3Plan {
    int which;  // 0 = delta A (auctions), 1 = delta P (persons)
    TraceArgs t;
    int proj;
    uint32_t *cnts;
    int64_t *starts;  // chained ticks only: the probe's run start positions
    uint64_t *offsets;
    bool small;
    bool dd;  // delta-vs-delta plan (trace length is tick-fresh)
    int slot;
};

struct Q3Train {
    bool pending = false;
    const dbsp_event *ev = nullptr;
    int64_t n = -1;
    int sb = LEN_BASE0, evi = 0;  // length-slot base and event index in use
    int next_sb = LEN_BASE1, next_evi = 0;
    DevBatch rawA, rawP, oA, oP, comb_chain;
    // in-train accumulator merge results (acc side + this tick's delta side);
    // lengths land in the base's L_XCHG pair with the train's readback
    DevBatch res[2];
    Q3Plan plans[3];
    int np = 0;
    size_t arena_base = 0, arena_off = 0;
};
// release the batches a train owns (its deltas and accumulator merges)
static void q3_train_drop(dbsp_ctx *c, Q3Train &T) {
    free_batch(c, T.oA);
    free_batch(c, T.oP);
    free_batch(c, T.res[0]);
    free_batch(c, T.res[1]);
}

// the winning-bid front q4 and q6 share: auctions ⋈ bids, Max per auction
struct WinningBids {
    Spine a_int, b_int;  // auction / bid traces (keyed by auction)
    Spine maxin_sp;      // max input integral (affected-key gather)
    DevBatch maxout;     // consolidated max output integral
};

struct dbsp_engine {
    dbsp_ctx *ctx = nullptr;
    int query = 0;
    int rank = 0, world = 1;

    // staged input events (resident in HBM before the timed region) and
    // their device column split (§8f3 columnizer, input.rs:591-721): the
    // per-tick flatmaps read the SoA columns; the AoS copy is kept for the
    // unstaged dbsp_engine_step path and q0
    dbsp_event *d_events = nullptr;
    int64_t n_events = 0;
    int64_t n_staged = 0;
    uint64_t *ev_cols[7] = {};  // kind,f0..f4,w
    std::vector<dbsp_event> h_events;  // host copy for the q0 CPU path

    // q3 state
    Spine a_int, p_int;
    // train-path accumulator (memtable): mirrors the TOP batch of a_int /
    // p_int when that batch was produced by the in-train (acc ⋈ delta)
    // merge; n==0 means the top is not accumulator-owned (classic inserts,
    // spills, fresh engine) and the next train merges from empty
    DevBatch q3_acc[2];
    // q8 state
    Spine pt_int, at_int, wp_int, wa_int;
    // q5 state
    Spine bt_int, wb_int, counts_int, bc_int;
    DevBatch maxin_int, maxout_int, maxz_int;
    // q4 and q6 state: the winning bids (an engine runs one query), then
    // q4's per-category Average (queries/q4.rs) ...
    WinningBids win;
    Spine q4_avg_int, q4_avgout;   // packed (sum<<20|count) integral + output
    // ... and q6's per-seller last-10 average fold (queries/q6.rs)
    Spine q6_fold_sp;
    DevBatch q6_foldout;
    // C5 state (query 100; BASELINE configs[4]: 1B-row indexed trace x
    // 10M-row delta incremental join + f64 sum aggregate)
    Spine c5_trace;   // (k, f64-bits val, +1 i64) join-side trace
    Spine c5_wint;    // f64-WEIGHTED integral of the weighed join stream
    Spine c5_out;     // aggregate output trace (k -> f64 sum bits, i64 w)
    // query 101 / 102 state: per-auction rolling bid volume / highest bid
    RollingOp roll;
    bool roll_stepped = false;  // rolling_init is rejected after a step
    bool roll_lateness_on = false;  // watermark-bounded state (off by default)
    uint64_t roll_lateness = 0;
    int64_t c5_n_delta = 0;
    uint64_t c5_seed = 0;
    uint64_t c5_delta_stride = 0;

    // chained-tick device watermark state: {wm, s0, e0, have_prev} and the
    // published bounds {s0,e0,s1,e1,have_prev,err} (q5/q8 single-rank path)
    unsigned long long *d_wm = nullptr;     // 4 slots
    unsigned long long *d_bounds = nullptr; // 6 slots
    // host mirror read back at each tick sync (only err is load-bearing on
    // the fast path; the rest feeds the explicit fallback)
    unsigned long long h_bounds[6] = {0, 0, 0, 0, 0, 0};

    // last tick's output; out_store is a reused capacity buffer so the hot
    // path allocates nothing for it (output_is_store marks when output
    // aliases it and must not be freed)
    DevBatch output;
    // pipelined front half of the NEXT tick (q5/q8: launched during this
    // tick's tail via the spines_insert_pair hook, consumed by the next
    // step; the (ev, n) pair is verified at consumption so an out-of-band
    // step never uses a stale front)
    struct {
        bool pending = false;
        const dbsp_event *ev = nullptr;
        int64_t n = -1;
        DevBatch rawA, rawB, oA, oB;
        size_t arena_base = 0, arena_off = 0;
    } front;
    // q3's pipelined full TRAIN (see the q3 tick comment): the whole next
    // tick's launch train enqueued at the end of the current step
    Q3Train train;
    const dbsp_event *next_ev = nullptr;  // set by dbsp_engine_run_staged
    int64_t next_n = -1;

    // chained-tick speculation control: big ticks whose deltas always
    // overflow the fused sort should not pay the speculative launch + redo
    // every tick — three consecutive losses switch the engine to the
    // explicit path until a chained tick wins again
    int spec_fail = 0;
    DevBatch out_store;
    int64_t out_cap = 0;
    bool output_is_store = false;
    std::vector<dbsp_event> q0_output;  // q0 CPU path
    // query 19 state: the top K bids of every auction
    TopKOp topk;
    bool topk_stepped = false;  // topk_init is rejected after a step
    // query 103 state: auctions antijoined with the bids' auction keys
    AntiJoinOp anti;
    // query 7 state: the bids by time, the host watermark {wm, s0, e0,
    // have_prev} in ms (the words k_wm_update keeps on the device for q5 and
    // q8), and the highest bids of the window
    Spine q7_bt;
    uint64_t q7_wm[4] = {0, 0, 0, 0};
    ArgMaxOp argmax;
};

extern "C" dbsp_status dbsp_engine_create(dbsp_engine **out, dbsp_ctx *ctx,
                                          int query, int rank, int world) {
    if (query != 0 && query != 3 && query != 4 && query != 5 &&
        query != 6 && query != 7 && query != 8 && query != 19 &&
        query != 100 &&
        query != 101 && query != 102 && query != 103)
        return DBSP_ERR_INVALID;
    // query 103 would shard correctly by k, but no multi-rank run of it has
    // been made
    if (query == 103 && world > 1) return DBSP_ERR_INVALID;
    // the exchange hashes k, which for query 19 packs the price under the
    // auction: it would split a group across ranks
    if (query == 19 && world > 1) return DBSP_ERR_INVALID;
    // query 7 has one group, the window: it cannot be split across ranks
    if (query == 7 && world > 1) return DBSP_ERR_INVALID;

    dbsp_engine *e = new dbsp_engine();
    e->ctx = ctx;
    e->query = query;
    if (query == 102) e->roll.agg = DBSP_ROLL_MAX;
    if (query == 19) e->topk.group_shift = 27;
    if (query == 7) {
        e->argmax.group_shift = 59;
        e->argmax.rank_shift = 32;
    }
    e->rank = rank;
    e->world = world;
    if (ctx) {
        if (hipMalloc(&e->d_wm, 11 * sizeof(uint64_t)) != hipSuccess) {
            delete e;
            return DBSP_ERR_OOM;
        }
        e->d_bounds = e->d_wm + 4;
        (void)hipMemset(e->d_wm, 0, 11 * sizeof(uint64_t));
    }
    *out = e;
    return DBSP_OK;
}

static void engine_free_output(dbsp_engine *e);

extern "C" dbsp_status dbsp_engine_destroy(dbsp_engine *e) {
    if (e && e->d_wm) (void)hipFree(e->d_wm);
    if (!e) return DBSP_OK;
    dbsp_ctx *c = e->ctx;
    // a pending q3 train's probe and join tail read the spines, the deltas
    // and out_store on the back stream: nothing is freed under them
    if (c) q3_sync_back(c);
    // discard any deferred insert round before the spines it references go
    // away (the merged pair is still in its spine's list, so dropping the
    // result is safe for ANY engine's pending round — at worst re-merged)
    drop_pending_insert(c);
    for (Spine *s : {&e->a_int, &e->p_int, &e->pt_int, &e->at_int, &e->wp_int,
                     &e->wa_int, &e->bt_int, &e->wb_int, &e->counts_int,
                     &e->bc_int, &e->c5_trace, &e->c5_wint, &e->c5_out,
                     &e->win.a_int, &e->win.b_int, &e->win.maxin_sp,
                     &e->q4_avg_int, &e->q4_avgout, &e->q6_fold_sp})
        s->clear(c);
    e->roll.clear(c);
    e->topk.clear(c);
    e->anti.clear(c);
    e->q7_bt.clear(c);
    e->argmax.clear(c);
    free_batch(c, e->win.maxout);
    free_batch(c, e->q6_foldout);
    free_batch(c, e->maxin_int);
    free_batch(c, e->maxout_int);
    free_batch(c, e->maxz_int);
    engine_free_output(e);
    if (e->front.pending) {
        free_batch(c, e->front.oA);
        free_batch(c, e->front.oB);
    }
    if (e->train.pending) {
        (void)hipStreamSynchronize(c->stream);  // back stream: synced above
        q3_train_drop(c, e->train);
    }
    if (e->out_store.k) free_batch(c, e->out_store);
    if (e->d_events) (void)dbspk::cache_free(e->d_events, c->stream);
    for (int i = 0; i < 7; i++)
        if (e->ev_cols[i]) (void)dbspk::cache_free(e->ev_cols[i], c->stream);
    (void)hipStreamSynchronize(c->stream);
    delete e;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_engine_stage_events(dbsp_engine *e,
                                                const dbsp_event *events,
                                                int64_t n) {
    dbsp_ctx *c = e->ctx;
    if (e->d_events) {
        HIP_CHECK_ST(dbspk::cache_free(e->d_events, c->stream));
        e->d_events = nullptr;
    }
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&e->d_events, n * sizeof(dbsp_event) + 64, c->stream));
    HIP_CHECK_ST(hipMemcpyAsync(e->d_events, events, n * sizeof(dbsp_event),
                                hipMemcpyHostToDevice, c->stream));
    // device column split (§8f3): one pass at stage time, outside the timed
    // region; per-tick flatmaps then read coalesced SoA streams
    for (int i = 0; i < 7; i++) {
        if (e->ev_cols[i]) {
            HIP_CHECK_ST(dbspk::cache_free(e->ev_cols[i], c->stream));
            e->ev_cols[i] = nullptr;
        }
        HIP_CHECK_ST(dbspk::cache_malloc((void **)&e->ev_cols[i],
                                         n * 8 + 64, c->stream));
    }
    TRY(dbspk::columnize_events(c->stream, e->d_events, n, e->ev_cols[0],
                                e->ev_cols[1], e->ev_cols[2], e->ev_cols[3],
                                e->ev_cols[4], e->ev_cols[5],
                                (int64_t *)e->ev_cols[6]));
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    e->n_events = n;
    e->n_staged = n;
    if (e->query == 0)
        e->h_events.assign(events, events + n);
    return DBSP_OK;
}

// ---- query 0: CPU-path plumbing config (BASELINE configs[0]) ----
// The reference's q0 is the identity circuit (queries/q0.rs:6-8); the measured
// work is the input path's OrdZSet::from_tuples consolidation
// (input.rs:664, trace/mod.rs:259-263), which this host path mirrors.
static void q0_step_host(dbsp_engine *e, const dbsp_event *ev, int64_t n) {
    std::vector<dbsp_event> v(ev, ev + n);
    std::sort(v.begin(), v.end(), [](const dbsp_event &a, const dbsp_event &b) {
        if (a.kind != b.kind) return a.kind < b.kind;
        if (a.f0 != b.f0) return a.f0 < b.f0;
        if (a.f1 != b.f1) return a.f1 < b.f1;
        if (a.f2 != b.f2) return a.f2 < b.f2;
        if (a.f3 != b.f3) return a.f3 < b.f3;
        return a.f4 < b.f4;
    });
    size_t off = 0;
    auto eq = [](const dbsp_event &a, const dbsp_event &b) {
        return a.kind == b.kind && a.f0 == b.f0 && a.f1 == b.f1 &&
               a.f2 == b.f2 && a.f3 == b.f3 && a.f4 == b.f4;
    };
    if (!v.empty()) {
        for (size_t i = 1; i < v.size(); i++) {
            if (eq(v[off], v[i])) v[off].w += v[i].w;
            else {
                if (v[off].w != 0) off++;
                v[off] = v[i];
            }
        }
        if (v[off].w != 0) off++;
        v.resize(off);
    }
    e->q0_output = std::move(v);
}

// ---- shared helpers ----

// sort+consolidate two independent small raw batches in ONE launch
// (consumes both raws)
static dbsp_status sort_two_small(dbsp_ctx *c, DevBatch rawA, DevBatch rawB,
                                  DevBatch &dA, DevBatch &dB) {
    ScopedTimer t(c, 0, (double)(rawA.n + rawB.n) * 48.0);
    DevBatch sA, sB, oA, oB;
    TRY(alloc_batch(c, rawA.n > 0 ? rawA.n : 1, sA, true));
    TRY(alloc_batch(c, rawB.n > 0 ? rawB.n : 1, sB, true));
    TRY(alloc_batch(c, rawA.n > 0 ? rawA.n : 1, oA));
    TRY(alloc_batch(c, rawB.n > 0 ? rawB.n : 1, oB));
    SortArgs sa{};
    sa.nb = 2;
    sort_slot(sa, 0, rawA, sA, oA);
    sort_slot(sa, 1, rawB, sB, oB);
    sa.d_len = c->d_len + LEN_OP;
    TRY(dbspk::sort_cons_small_batch(c->stream, sa, false));
    TRY(read_len(c, LEN_OP, 2));
    oA.n = c->h_len[LEN_OP];
    oB.n = c->h_len[LEN_OP + 1];
    free_batch(c, rawA);
    free_batch(c, rawB);
    free_batch(c, sA);
    free_batch(c, sB);
    dA = oA;
    dB = oB;
    return DBSP_OK;
}

// sort+consolidate two raw batches: fused when both fit one workgroup
static dbsp_status sort_pair(dbsp_ctx *c, DevBatch r0, DevBatch r1,
                             DevBatch &o0, DevBatch &o1) {
    if (r0.n <= 8192 && r1.n <= 8192) return sort_two_small(c, r0, r1, o0, o1);
    TRY(sort_consolidate_batch(c, r0, o0));
    return sort_consolidate_batch(c, r1, o1);
}

// shard+exchange BOTH streams with one grouped counts phase and one grouped
// data phase (the per-tick collective latency is the scaling cost at 40k-event
// ticks; fusing the two sides halves it)
static dbsp_status shard_exchange_pair(dbsp_ctx *c, DevBatch l0, DevBatch l1,
                                       DevBatch &o0, DevBatch &o1,
                                       int64_t hint0 = 0, int64_t hint1 = 0) {
    if (!sharding_on(c)) {
        o0 = l0;
        o1 = l1;
        return DBSP_OK;
    }
    const int world = c->world;
    DevBatch p0, p1;
    TRY(alloc_batch(c, l0.n > 0 ? l0.n : 1, p0, true));
    TRY(alloc_batch(c, l1.n > 0 ? l1.n : 1, p1, true));
    int64_t off0[65], off1[65];
    TRY(dbspk::shard_rows_pair(c->stream, l0, l1, world, p0, p1, off0, off1));
    p0.n = l0.n;
    p1.n = l1.n;
    free_batch(c, l0);
    free_batch(c, l1);
    // FAST PATH: fixed-frame exchange.  hint0/hint1 = the caller's
    // rank-uniform expectation of each stream's GLOBAL rows this tick (from
    // the tick's event count and the query's mix), so every rank derives
    // the SAME per-peer capacity and the equal-count ncclAllToAll is a
    // legal collective.  Overflow (per-peer count above capacity, e.g.
    // hot-key skew) travels in the frame header; every rank sees -1 totals
    // at its sync below and replays through the dynamic path — identical
    // collective sequence on all ranks, so no deadlock.
    if (hint0 > 0 && hint1 > 0 && world <= 8 && c->comm) {
        const int64_t P0 = 2 * hint0 / world + 512;
        const int64_t P1 = 2 * hint1 / world + 512;
        const int64_t S = 2 + 3 * P0 + 3 * P1;
        uint64_t *fsend, *frecv;
        HIP_CHECK_ST(dbspk::cache_malloc((void **)&fsend,
                                         (size_t)world * S * 8, c->stream));
        HIP_CHECK_ST(dbspk::cache_malloc((void **)&frecv,
                                         (size_t)world * S * 8, c->stream));
        dbspk::FramePairArgs fa{};
        fa.p0k = p0.k; fa.p0v = p0.v; fa.p0w = p0.w;
        fa.p1k = p1.k; fa.p1v = p1.v; fa.p1w = p1.w;
        for (int r = 0; r <= world; r++) {
            fa.off0[r] = off0[r];
            fa.off1[r] = off1[r];
        }
        fa.world = world;
        fa.P0 = P0;
        fa.P1 = P1;
        fa.frame = fsend;
        TRY(dbspk::frames_pack_pair(c->stream, fa));
        if (ncclAllToAll(fsend, frecv, (size_t)S, ncclUint64, c->comm,
                         c->stream) != ncclSuccess)
            return DBSP_ERR_INTERNAL;
        DevBatch r0, r1;
        TRY(alloc_batch(c, world * P0, r0, true));
        TRY(alloc_batch(c, world * P1, r1, true));
        TRY(dbspk::frames_unpack_pair(c->stream, frecv, world, P0, P1, r0, r1,
                                      c->d_len + L_XCHG,
                                      c->d_len + L_XCHG + 1));
        TRY(read_len(c, L_XCHG, 2));
        HIP_CHECK_ST(dbspk::cache_free(fsend, c->stream));
        HIP_CHECK_ST(dbspk::cache_free(frecv, c->stream));
        const int64_t tot0 = c->h_len[L_XCHG], tot1 = c->h_len[L_XCHG + 1];
        if (tot0 >= 0 && tot1 >= 0) {
            r0.n = tot0;
            r1.n = tot1;
            return sort_pair(c, r0, r1, o0, o1);
        }
        // overflow sentinel: fall through to the dynamic exchange on the
        // retained partitioned buffers (all ranks take this same branch)
    }
    // counts: 2 int64 per pair, one grouped phase
    int64_t send_cnt[128], recv_cnt[128];
    for (int r = 0; r < world; r++) {
        send_cnt[2 * r] = off0[r + 1] - off0[r];
        send_cnt[2 * r + 1] = off1[r + 1] - off1[r];
    }
    // one allgather of the 2-per-peer count vectors (see alltoallv_cols)
    int64_t *d_snd, *d_all;
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&d_snd, 2 * world * 8, c->stream));
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&d_all,
                                     (size_t)world * 2 * world * 8, c->stream));
    HIP_CHECK_ST(hipMemcpyAsync(d_snd, send_cnt, 2 * world * 8,
                                hipMemcpyHostToDevice, c->stream));
    if (ncclAllGather(d_snd, d_all, 2 * world, ncclInt64, c->comm,
                      c->stream) != ncclSuccess)
        return DBSP_ERR_INTERNAL;
    int64_t h_all[2 * 64 * 64];
    HIP_CHECK_ST(hipMemcpyAsync(h_all, d_all, (size_t)world * 2 * world * 8,
                                hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    for (int r = 0; r < world; r++) {
        recv_cnt[2 * r] = h_all[(size_t)r * 2 * world + 2 * c->rank];
        recv_cnt[2 * r + 1] = h_all[(size_t)r * 2 * world + 2 * c->rank + 1];
    }
    int64_t tot0 = 0, tot1 = 0;
    for (int r = 0; r < world; r++) {
        tot0 += recv_cnt[2 * r];
        tot1 += recv_cnt[2 * r + 1];
    }
    DevBatch r0, r1;
    TRY(alloc_batch(c, tot0 > 0 ? tot0 : 1, r0, true));
    TRY(alloc_batch(c, tot1 > 0 ? tot1 : 1, r1, true));
    // data: both sides' three columns in one grouped phase
    ncclGroupStart();
    int64_t ro0 = 0, ro1 = 0;
    for (int r = 0; r < world; r++) {
        int64_t s0 = off0[r], n0 = off0[r + 1] - off0[r];
        int64_t s1 = off1[r], n1 = off1[r + 1] - off1[r];
        if (n0 > 0) {
            ncclSend(p0.k + s0, n0, ncclUint64, r, c->comm, c->stream);
            ncclSend(p0.v + s0, n0, ncclUint64, r, c->comm, c->stream);
            ncclSend(p0.w + s0, n0, ncclInt64, r, c->comm, c->stream);
        }
        if (n1 > 0) {
            ncclSend(p1.k + s1, n1, ncclUint64, r, c->comm, c->stream);
            ncclSend(p1.v + s1, n1, ncclUint64, r, c->comm, c->stream);
            ncclSend(p1.w + s1, n1, ncclInt64, r, c->comm, c->stream);
        }
        if (recv_cnt[2 * r] > 0) {
            ncclRecv(r0.k + ro0, recv_cnt[2 * r], ncclUint64, r, c->comm, c->stream);
            ncclRecv(r0.v + ro0, recv_cnt[2 * r], ncclUint64, r, c->comm, c->stream);
            ncclRecv(r0.w + ro0, recv_cnt[2 * r], ncclInt64, r, c->comm, c->stream);
        }
        if (recv_cnt[2 * r + 1] > 0) {
            ncclRecv(r1.k + ro1, recv_cnt[2 * r + 1], ncclUint64, r, c->comm, c->stream);
            ncclRecv(r1.v + ro1, recv_cnt[2 * r + 1], ncclUint64, r, c->comm, c->stream);
            ncclRecv(r1.w + ro1, recv_cnt[2 * r + 1], ncclInt64, r, c->comm, c->stream);
        }
        ro0 += recv_cnt[2 * r];
        ro1 += recv_cnt[2 * r + 1];
    }
    ncclGroupEnd();
    HIP_CHECK_ST(dbspk::cache_free(d_snd, c->stream));
    HIP_CHECK_ST(dbspk::cache_free(d_all, c->stream));
    r0.n = tot0;
    r1.n = tot1;
    return sort_pair(c, r0, r1, o0, o1);
}

static inline double host_us() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

// DBSP_COMMIT_PROF=1: host time of q3_enqueue_train split by group of
// runtime calls (printed with the commit's line).  hook_mark(i) charges the
// time since the previous mark to group i.
enum : int {
    HK_FLATMAP,  // raw-stream arena bumps, counter fill (if any), flatmap
    HK_SORT,     // sort scratch + delta allocations, delta sorts
    HK_ALLOC,    // accumulator-result allocations
    HK_FORK,     // fork event record
    HK_MERGE,    // accumulator fold / merge launch
    HK_HEAD,     // head copy + ev_tick record
    HK_PROBE,    // back-stream wait on the fork event, plan build, probe
    HK_TAIL,     // join tail buffers + launch
    HK_JOIN,     // tail copy + ev_tail record
    HK_N
};
static const bool g_hook_prof = []() {
    const char *v = getenv("DBSP_COMMIT_PROF");
    return v && v[0] == '1';
}();
static double g_hook_t = 0, g_hook_us[HK_N];
static inline void hook_mark(int i) {
    if (!g_hook_prof) return;
    const double t = host_us();
    g_hook_us[i] += t - g_hook_t;
    g_hook_t = t;
}

// flatmap events slice into up to two raw streams, then sort+consolidate
static dbsp_status build_deltas_chain(dbsp_engine *e, const dbsp_event *d_ev,
                                      int64_t n, DevBatch &rawA, DevBatch &rawB,
                                      DevBatch &oA, DevBatch &oB, int sb = 0,
                                      bool take = false);

// If d_ev points into the staged event array, return its column-split view
// (shifted to the same offset) so the flatmap reads coalesced SoA streams.
static bool staged_cols(dbsp_engine *e, const dbsp_event *d_ev,
                        dbspk::EventCols &out) {
    if (!e->ev_cols[0] || !e->d_events || d_ev < e->d_events) return false;
    const int64_t off = d_ev - e->d_events;
    if (off < 0 || off >= e->n_staged) return false;
    out = {e->ev_cols[0] + off, e->ev_cols[1] + off, e->ev_cols[2] + off,
           e->ev_cols[3] + off, e->ev_cols[4] + off, e->ev_cols[5] + off,
           (const int64_t *)(e->ev_cols[6] + off)};
    return true;
}

// chained flatmap: allocate both raw streams (transient) and launch the
// flatmap with its two row counters left on device at d_len[sb + L_RAW..].
// The counters are zeroed by a memset in front of the flatmap unless the
// base's raw_zero flag says a taking sort already did it; either way the
// flag is cleared, because the flatmap leaves them non-zero.
static dbsp_status flatmap_chain(dbsp_engine *e, const dbsp_event *d_ev,
                                 int64_t n, DevBatch &rawA, DevBatch &rawB,
                                 int sb = LEN_BASE0) {
    dbsp_ctx *c = e->ctx;
    const int64_t cap = n > 0 ? n : 1;
    TRY(alloc_batch(c, cap, rawA, true));
    TRY(alloc_batch(c, cap, rawB, true));
    dbspk::EventCols cols{};
    const bool hc = staged_cols(e, d_ev, cols);
    bool &known_zero = c->raw_zero[sb == LEN_BASE1];
    const bool ctr_zero = known_zero;
    known_zero = false;
    return dbspk::flatmap_events_chain(c->stream, d_ev, hc ? &cols : nullptr,
                                       n, e->query, rawA, rawB,
                                       (uint64_t *)(c->d_len + sb + L_RAW),
                                       ctr_zero);
}

// speculative fused sort of two chained streams: input lengths read from the
// device slots nA/nB, output lengths (or -1) left at d_len[sb + L_DELTA..];
// oA/oB stay pending (n = -1) until the caller's readback.  take: nA/nB are
// the base's flatmap counters (L_RAW); the sort hands them back zeroed,
// leaves the lengths at L_RAWN and so re-establishes raw_zero for the base.
static dbsp_status sort_pair_chain(dbsp_ctx *c, const DevBatch &inA,
                                   const DevBatch &inB, int64_t capA,
                                   int64_t capB, int64_t *nA, int64_t *nB,
                                   int sb, int64_t n_events, DevBatch &oA,
                                   DevBatch &oB, bool take = false) {
    DevBatch sA, sB;
    TRY(alloc_batch(c, capA, sA, true));
    TRY(alloc_batch(c, capB, sB, true));
    TRY(alloc_batch(c, capA, oA));
    TRY(alloc_batch(c, capB, oB));
    SortArgs sa{};
    sa.nb = 2;
    if (take) {
        sort_slot_take(sa, 0, inA, sA, oA, nA, c->d_len + sb + L_RAWN);
        sort_slot_take(sa, 1, inB, sB, oB, nB, c->d_len + sb + L_RAWN + 1);
    } else {
        sort_slot(sa, 0, inA, sA, oA, nA);
        sort_slot(sa, 1, inB, sB, oB, nB);
    }
    sa.d_len = c->d_len + sb + L_DELTA;
    {
        ScopedTimer t(c, 0, (double)n_events * 48.0);
        TRY(dbspk::sort_cons_small_batch(c->stream, sa, false));
    }
    if (take) c->raw_zero[sb == LEN_BASE1] = true;
    oA.n = -1;
    oB.n = -1;
    return DBSP_OK;
}

// n1_raw (optional): receives the second raw stream's row count, which the
// front reads back either way (query 19's error word)
static dbsp_status build_deltas(dbsp_engine *e, const dbsp_event *d_ev,
                                int64_t n, DevBatch &d0, DevBatch &d1,
                                bool want_two, int64_t *n1_raw = nullptr) {
    // Explicit-path deltas (sharded ranks, oversized ticks): the front still
    // CHAINS — flatmap and the speculative fused sorts launch back-to-back
    // and one sync reads counts + lengths; deltas over the fused capacity
    // re-sort through the sized paths.  Only then does the key exchange run
    // (it needs host lengths).
    dbsp_ctx *c = e->ctx;
    if (n > 16384) {
        // big ticks: per-stream deltas would lose the sort speculation every
        // time, so run the explicit front (host counts, sized sorts)

        DevBatch raw0, raw1;
        TRY(alloc_batch(c, n > 0 ? n : 1, raw0, true));
        TRY(alloc_batch(c, n > 0 ? n : 1, raw1, true));
        dbspk::EventCols cols{};
        const bool hc = staged_cols(e, d_ev, cols);
        TRY(dbspk::flatmap_events(c->stream, d_ev, hc ? &cols : nullptr, n,
                                  e->query, &raw0, &raw1));
        if (n1_raw) *n1_raw = raw1.n;
        if (want_two && raw0.n <= 8192 && raw1.n <= 8192) {
            TRY(sort_two_small(c, raw0, raw1, d0, d1));
        } else {
            TRY(sort_consolidate_batch(c, raw0, d0));
            if (want_two)
                TRY(sort_consolidate_batch(c, raw1, d1));
            else
                free_batch(c, raw1);
        }
    } else {
        DevBatch rawA, rawB, oA, oB;
        TRY(build_deltas_chain(e, d_ev, n, rawA, rawB, oA, oB));
        TRY(read_len(c, LEN_BASE0, LEN_TICK));
        if (n1_raw) *n1_raw = c->h_len[L_RAW + 1];
        if (c->h_len[L_DELTA] < 0 || c->h_len[L_DELTA + 1] < 0) {
            rawA.n = c->h_len[L_RAW];
            rawB.n = c->h_len[L_RAW + 1];
            free_batch(c, oA);
            free_batch(c, oB);
            TRY(sort_consolidate_batch(c, rawA, d0));
            if (want_two) {
                TRY(sort_consolidate_batch(c, rawB, d1));
            } else {
                free_batch(c, rawB);
            }
        } else {
            oA.n = c->h_len[L_DELTA];
            oB.n = c->h_len[L_DELTA + 1];
            d0 = oA;
            if (want_two) d1 = oB;
            else free_batch(c, oB);
        }
    }
    // worker sharding: co-locate keys across ranks (shard.rs:88)
    if (sharding_on(c)) {
        // frame hints: the generator's event-kind schedule is deterministic
        // (person:auction:bid = 1:3:46, config.rs:128-143), so per-stream
        // global row counts are known from the tick's event count alone
        if (want_two) {
            DevBatch s0, s1;
            const bool ab = e->query == 4 || e->query == 6;
            const int64_t h0 = ab ? 3 * n / 50 + 64 : n / 50 + 64;
            const int64_t h1 = ab ? 46 * n / 50 + 64 : 3 * n / 50 + 64;
            TRY(shard_exchange_pair(c, d0, d1, s0, s1, h0, h1));
            d0 = s0;
            d1 = s1;
        } else {
            DevBatch s0;
            TRY(shard_exchange(c, d0, s0, n));
            d0 = s0;
        }
    }
    return DBSP_OK;
}

// Chained variant (single-rank): flatmap counters stay on device (L_RAW),
// the fused sort launches behind them reading its lengths from the device
// (outputs at L_DELTA, -1 on overflow), and no sync happens here — the
// caller reads everything at its one tick sync and re-sorts through the
// sized paths if the speculation lost.
static dbsp_status build_deltas_chain(dbsp_engine *e, const dbsp_event *d_ev,
                                      int64_t n, DevBatch &rawA, DevBatch &rawB,
                                      DevBatch &oA, DevBatch &oB, int sb,
                                      bool take) {
    dbsp_ctx *c = e->ctx;
    const int64_t cap = n > 0 ? n : 1;
    TRY(flatmap_chain(e, d_ev, n, rawA, rawB, sb));
    hook_mark(HK_FLATMAP);
    TRY(sort_pair_chain(c, rawA, rawB, cap, cap, c->d_len + sb + L_RAW,
                        c->d_len + sb + L_RAW + 1, sb, n, oA, oB, take));
    hook_mark(HK_SORT);
    return DBSP_OK;
}

// Sharded chained front (q3-class pair streams): flatmap -> hash-scatter
// straight into fixed frames (device counters, no pre-sort — shard.rs
// consolidates POST-exchange) -> one equal-count ncclAllToAll -> unpack
// (receive totals at the L_XCHG pair) -> speculative fused sorts reading those
// totals.  The round-1 sharded tick ran the explicit path with ~7 host
// syncs (partition offsets, counts allgather, totals, sorts...); this one
// syncs ONCE at the caller like the unsharded chain.  Overflow anywhere
// (frame capacity, fused-sort capacity) surfaces as -1 lengths and the
// caller replays dynamically — every rank sees the same sentinel at the
// same sync, so the collective sequence stays rank-uniform.
static dbsp_status build_deltas_chain_sharded(
    dbsp_engine *e, const dbsp_event *d_ev, int64_t n, DevBatch &rawA,
    DevBatch &rawB, DevBatch &recvA, DevBatch &recvB, DevBatch &oA,
    DevBatch &oB) {
    dbsp_ctx *c = e->ctx;
    const int world = c->world;
    const int64_t cap = n > 0 ? n : 1;
    int64_t *const raw_len = c->d_len + L_RAW, *const tot = c->d_len + L_XCHG;
    TRY(flatmap_chain(e, d_ev, n, rawA, rawB));
    // frame capacities from the deterministic event mix (config.rs:128-143)
    const int64_t P0 = 2 * (n / 50 + 64) / world + 512;
    const int64_t P1 = 2 * (3 * n / 50 + 64) / world + 512;
    const int64_t S = 2 + 3 * P0 + 3 * P1;
    uint64_t *fsend, *frecv;
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&fsend, (size_t)world * S * 8,
                                     c->stream));
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&frecv, (size_t)world * S * 8,
                                     c->stream));
    TRY(dbspk::shard_frames_chain(c->stream, rawA, raw_len, rawB, raw_len + 1,
                                  world, P0, P1, cap, fsend));
    if (ncclAllToAll(fsend, frecv, (size_t)S, ncclUint64, c->comm,
                     c->stream) != ncclSuccess)
        return DBSP_ERR_INTERNAL;
    const int64_t capA = world * P0, capB = world * P1;
    TRY(alloc_batch(c, capA, recvA, true));
    TRY(alloc_batch(c, capB, recvB, true));
    TRY(dbspk::frames_unpack_pair(c->stream, frecv, world, P0, P1, recvA,
                                  recvB, tot, tot + 1));
    HIP_CHECK_ST(dbspk::cache_free(fsend, c->stream));
    HIP_CHECK_ST(dbspk::cache_free(frecv, c->stream));
    return sort_pair_chain(c, recvA, recvB, capA, capB, tot, tot + 1,
                           LEN_BASE0, n, oA, oB);
}

// join delta against a whole spine in one count/emit pair (join is linear in
// the trace; spine read path = the reference's CursorList)
static dbsp_status join_vs_trace(dbsp_ctx *c, const DevBatch &delta,
                                 const TraceArgs &t, int proj, uint64_t param,
                                 std::vector<DevBatch> &outs) {
    DevBatch o;
    ScopedTimer timer(c, 2, (double)delta.n * 24.0);
    TRY(dbspk::join_spine_rows(c->stream, delta, t, proj, param, &o));
    if (o.n > 0) outs.push_back(o);
    else free_batch(c, o);
    return DBSP_OK;
}
static dbsp_status join_vs_spine(dbsp_ctx *c, const DevBatch &delta,
                                 Spine &spine, int proj, uint64_t param,
                                 std::vector<DevBatch> &outs) {
    if (delta.n == 0 || spine.batches.empty()) return DBSP_OK;
    TRY(spine.cap_batches(c));
    const TraceArgs t = trace_args_of(spine);
    if (t.nb == 0) return DBSP_OK;
    return join_vs_trace(c, delta, t, proj, param, outs);
}
// delta ⋈ delta: the other side's tick batch stands in as a one-batch trace
static dbsp_status join_vs_batch(dbsp_ctx *c, const DevBatch &delta,
                                 const DevBatch &other, int proj,
                                 uint64_t param, std::vector<DevBatch> &outs) {
    if (delta.n <= 0 || other.n <= 0) return DBSP_OK;
    return join_vs_trace(c, delta, trace_args_one(other), proj, param, outs);
}

// gather raw result batches (consumed) into one raw transient batch; a single
// batch is handed through as it is
static dbsp_status gather_raw(dbsp_ctx *c, std::vector<DevBatch> &outs,
                              DevBatch &cat) {
    if (outs.size() == 1) {
        cat = outs[0];
    } else {
        TRY(concat_batches(c, outs, cat, true));
        for (auto &b : outs) free_batch(c, b);
    }
    outs.clear();
    return DBSP_OK;
}

// consolidate a list of raw result batches into one batch
static dbsp_status finalize_raw(dbsp_ctx *c, std::vector<DevBatch> &outs,
                                DevBatch &out) {
    DevBatch cat;
    TRY(gather_raw(c, outs, cat));
    return sort_consolidate_batch(c, cat, out);
}

// ---- window stage (window.rs:144-220) ----
// One leg: a spine windowed against the tick's consolidated delta.  The
// ranges launch reads the bounds the device watermark published and fills
// the region table — three regions per spine batch plus the tick batch, 5
// int64 each — leaving the row total in a d_len slot; the emit copies the
// rows once the caller's sync has brought that total to the host.
struct WindowLeg {
    Spine *trace;           // excludes this tick
    const DevBatch *delta;  // sorted; its n is read only when n_dev is null
    const int64_t *n_dev;   // the delta's device length, or null
    int slot;               // d_len slot of tick base 0 that gets the total
    // filled by window_launch
    TraceArgs ta{};
    int nreg = 0;
    ScratchBuf table;  // let go after the emit
};

// plan each leg (once: a second launch, after a re-sort, reuses the spine
// arguments and the table) and launch its ranges behind the published bounds
static dbsp_status window_launch(dbsp_engine *e, WindowLeg *legs, int n) {
    dbsp_ctx *c = e->ctx;
    for (WindowLeg *w = legs; w < legs + n; w++) {
        if (w->table.p) continue;
        TRY(w->trace->cap_batches(c));
        w->ta = trace_args_of(*w->trace);
        w->nreg = 3 * w->ta.nb + 1;
        TRY(w->table.alloc(c, (size_t)w->nreg * 5 * 8 + 8,
                           /*arena_first=*/true));
    }
    ScopedTimer t(c, 4, 0.0);
    for (WindowLeg *w = legs; w < legs + n; w++)
        TRY(dbspk::window_ranges_chain(c->stream, w->ta, w->delta->k,
                                       w->delta->n, w->n_dev, e->d_bounds,
                                       w->table.as<int64_t>(),
                                       c->d_len + w->slot));
    return DBSP_OK;
}

// emit a launched leg's rows (none for a total of 0 or the -1 of a lost
// speculation) into a batch appended to raw
static dbsp_status window_emit(dbsp_ctx *c, WindowLeg &w,
                               std::vector<DevBatch> &raw,
                               bool transient = true) {
    const int64_t total = c->h_len[w.slot];
    if (total > 0) {
        DevBatch o;
        TRY(alloc_batch(c, total, o, transient));
        TRY(dbspk::window_emit_multi(c->stream, w.ta, *w.delta,
                                     w.table.as<int64_t>(), w.nreg, total, o));
        raw.push_back(o);
    }
    w.table.reset();
    return DBSP_OK;
}

// the operator on its own: the trace is one batch and the bounds come from
// the caller, so the regions come out in the order retract, shrink, insert,
// tick batch
extern "C" dbsp_status dbsp_window(dbsp_ctx *c, const dbsp_batch *trace,
                                   const dbsp_batch *batch, int have_prev,
                                   uint64_t s0, uint64_t e0, uint64_t s1,
                                   uint64_t e1, dbsp_batch *out) {
    const DevBatch b = as_batch(batch);
    WindowLeg w{nullptr, &b, nullptr, L_WIN};
    w.ta = trace_args_one(as_batch(trace));
    w.nreg = 3 * w.ta.nb + 1;
    TRY(w.table.alloc(c, (size_t)w.nreg * 5 * 8 + 8));
    std::vector<DevBatch> res;
    {
        ScopedTimer t(c, 4, 0.0);
        TRY(dbspk::window_ranges_multi(c->stream, w.ta, b.k, b.n, have_prev,
                                       s0, e0, s1, e1, w.table.as<int64_t>(),
                                       c->d_len + w.slot));
        TRY(read_len(c, w.slot, 1));
        TRY(window_emit(c, w, res, /*transient=*/false));
    }
    put_batch(out, res.empty() ? DevBatch{} : res[0]);
    return DBSP_OK;
}

// ---- test-facing: the watermark kernel and the window pair over a spine ----

// scratch device words of one watermark update: the state, the bounds, the
// device length and the reduced maximum
enum { WM_STATE = 0, WM_BOUNDS = 4, WM_N = 10, WM_GMAX = 11, WM_WORDS = 12 };

// upload state / bounds / length / maximum, run k_wm_update from `source`,
// leave everything in dev (no sync, nothing read back)
static dbsp_status wm_update_scratch(dbsp_ctx *c, unsigned long long *dev,
                                     uint64_t *h, const uint64_t state[4],
                                     const uint64_t bounds[6], int source,
                                     const uint64_t *ak, int64_t n,
                                     uint64_t gmax, uint64_t width,
                                     uint64_t tumble, uint64_t lag) {
    for (int i = 0; i < 4; i++) h[WM_STATE + i] = state[i];
    for (int i = 0; i < 6; i++) h[WM_BOUNDS + i] = bounds[i];
    h[WM_N] = (uint64_t)n;
    h[WM_GMAX] = gmax;
    HIP_CHECK_ST(hipMemcpyAsync(dev, h, WM_WORDS * 8, hipMemcpyHostToDevice,
                                c->stream));
    WmSource src{ak, 0, nullptr, nullptr};
    if (source == DBSP_WM_HOST_N) src.n = n;
    else src.n_dev = (const int64_t *)(dev + WM_N);
    if (source == DBSP_WM_GMAX) src.gmax_dev = dev + WM_GMAX;
    return dbspk::wm_update(c->stream, src, width, tumble, lag,
                            dev + WM_STATE, dev + WM_BOUNDS);
}

extern "C" dbsp_status dbsp_wm_update(dbsp_ctx *c, uint64_t *state,
                                      uint64_t *bounds, int source,
                                      const uint64_t *ak, int64_t ak_len,
                                      int64_t n, uint64_t gmax, uint64_t width,
                                      uint64_t tumble, uint64_t lag) {
    if (!state || !bounds || tumble == 0 || ak_len < 0 || n > ak_len ||
        (ak_len > 0 && !ak) || source < DBSP_WM_HOST_N ||
        source > DBSP_WM_GMAX)
        return DBSP_ERR_INVALID;
    unsigned long long *dev = nullptr;
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&dev, WM_WORDS * 8, c->stream));
    uint64_t h[WM_WORDS];
    dbsp_status st = wm_update_scratch(c, dev, h, state, bounds, source, ak, n,
                                       gmax, width, tumble, lag);
    if (st == DBSP_OK &&
        hipMemcpyAsync(h, dev, WM_WORDS * 8, hipMemcpyDeviceToHost,
                       c->stream) != hipSuccess)
        st = DBSP_ERR_INTERNAL;
    if (st == DBSP_OK) st = dbsp_ctx_sync(c);
    (void)dbspk::cache_free(dev, c->stream);
    if (st != DBSP_OK) return st;
    for (int i = 0; i < 4; i++) state[i] = h[WM_STATE + i];
    for (int i = 0; i < 6; i++) bounds[i] = h[WM_BOUNDS + i];
    return DBSP_OK;
}

// a region table the emit may follow: every region inside its source, the
// offsets the running sum of the lengths, the total their sum
static bool window_table_ok(const int64_t *tb, int nreg, const TraceArgs &t,
                            int64_t bcap, int64_t total) {
    int64_t acc = 0;
    for (int r = 0; r < nreg; r++) {
        const int64_t src = tb[r * 5], lo = tb[r * 5 + 1], len = tb[r * 5 + 2];
        if (src != (r < 3 * t.nb ? r / 3 : -1)) return false;
        const int64_t n = src < 0 ? bcap : t.n[src];
        if (lo < 0 || len < 0 || lo > n || len > n - lo) return false;
        if (tb[r * 5 + 3] != 1 && tb[r * 5 + 3] != -1) return false;
        if (tb[r * 5 + 4] != acc) return false;
        acc += len;
    }
    return acc == total;
}

extern "C" dbsp_status dbsp_window_spine(dbsp_ctx *c,
                                         const dbsp_batch *trace_batches,
                                         int n_batches, const dbsp_batch *batch,
                                         int route, uint64_t *bounds,
                                         dbsp_window_chain *chain,
                                         int64_t *total, int64_t *table_host,
                                         dbsp_batch *out) {
    TraceArgs t;
    TRY(trace_verbatim(trace_batches, n_batches, t));
    const DevBatch b = as_batch(batch);
    if (b.n < 0 || !bounds || !total || !table_host ||
        (route != 1 && route != 2))
        return DBSP_ERR_INVALID;
    if (route == 2 &&
        (!chain || chain->tumble == 0 || chain->wm_n > b.n || chain->bn > b.n))
        return DBSP_ERR_INVALID;
    const int nreg = 3 * t.nb + 1;
    int64_t *table = nullptr;
    unsigned long long *dev = nullptr;
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&table,
                                     (size_t)nreg * 5 * 8 + 8, c->stream));
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&dev, (WM_WORDS + 1) * 8,
                                     c->stream));
    int64_t *d_bn = (int64_t *)(dev + WM_WORDS);
    uint64_t h[WM_WORDS];
    dbsp_status st = DBSP_OK;
    if (route == 1) {
        st = dbspk::window_ranges_multi(c->stream, t, b.k, b.n,
                                        bounds[4] != 0, bounds[0], bounds[1],
                                        bounds[2], bounds[3], table,
                                        c->d_len + L_WIN);
    } else {
        const uint64_t none[6] = {};
        if (hipMemcpyAsync(d_bn, &chain->bn, 8, hipMemcpyHostToDevice,
                           c->stream) != hipSuccess)
            st = DBSP_ERR_INTERNAL;
        if (st == DBSP_OK)
            st = wm_update_scratch(c, dev, h, chain->state, none,
                                   DBSP_WM_DEV_N, b.k, chain->wm_n, 0,
                                   chain->width, chain->tumble, chain->lag);
        // the host length stays 0, as in a chained tick
        if (st == DBSP_OK)
            st = dbspk::window_ranges_chain(c->stream, t, b.k, 0, d_bn,
                                            dev + WM_BOUNDS, table,
                                            c->d_len + L_WIN);
        if (st == DBSP_OK &&
            hipMemcpyAsync(h, dev, WM_WORDS * 8, hipMemcpyDeviceToHost,
                           c->stream) != hipSuccess)
            st = DBSP_ERR_INTERNAL;
    }
    if (st == DBSP_OK) st = read_len(c, L_WIN, 1);
    DevBatch res;
    if (st == DBSP_OK) {
        *total = c->h_len[L_WIN];
        if (route == 2) {
            for (int i = 0; i < 4; i++) chain->state[i] = h[WM_STATE + i];
            for (int i = 0; i < 6; i++) bounds[i] = h[WM_BOUNDS + i];
        }
    }
    if (st == DBSP_OK && *total >= 0) {
        if (hipMemcpyAsync(table_host, table, (size_t)nreg * 5 * 8,
                           hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            st = DBSP_ERR_INTERNAL;
        if (st == DBSP_OK) st = dbsp_ctx_sync(c);
        // the emit reads where the table points: follow it only when it
        // stays inside the batches
        if (st == DBSP_OK && !window_table_ok(table_host, nreg, t, b.n, *total))
            st = DBSP_ERR_INTERNAL;
        if (st == DBSP_OK && *total > 0) {
            st = alloc_batch(c, *total, res);
            if (st == DBSP_OK)
                st = dbspk::window_emit_multi(c->stream, t, b, table, nreg,
                                              *total, res);
        }
    }
    if (st == DBSP_OK) st = dbsp_ctx_sync(c);
    (void)dbspk::cache_free(table, c->stream);
    (void)dbspk::cache_free(dev, c->stream);
    if (st != DBSP_OK) {
        free_batch(c, res);
        return st;
    }
    put_batch(out, res);
    return DBSP_OK;
}

// map + sort/consolidate (copies; input retained)
static dbsp_status map_sorted(dbsp_ctx *c, const DevBatch &in, int mode,
                              DevBatch &out) {
    if (in.n == 0) {
        out = DevBatch{};
        return DBSP_OK;
    }
    DevBatch raw;
    TRY(alloc_batch(c, in.n, raw));
    TRY(dbspk::map_rows(c->stream, in, mode, raw));
    TRY(sort_consolidate_batch(c, raw, out));
    return DBSP_OK;
}

// linear aggregate + upsert over spines (aggregate/mod.rs:479-547 +
// upsert.rs:161-208; linear in both traces, so evaluated per spine batch).
// in_trace's weight type is the sums': f64 sums (aggregate_linear's sum over
// C5's weighted integral, aggregate/mod.rs:297-323) accumulate in batch
// order, tolerance 2 ulp * depth.  The output trace is i64-weighted either
// way.
static dbsp_status agg_linear_spine(dbsp_ctx *c, const DevBatch &delta,
                                    const Spine &in_trace, Spine &out_trace,
                                    DevBatch &out) {
    if (delta.n == 0) {
        out = DevBatch{};
        return DBSP_OK;
    }
    ScopedTimer timer(c, 3, 0.0);
    std::vector<DevBatch> outs;
    {
        uint64_t *k = nullptr;
        int64_t nk = 0;
        TRY(dbspk::unique_keys(c->stream, delta.k, delta.n, &k, &nk));
        ScratchBuf keys(c, k);
        // inserts
        DevBatch ins;
        TRY(agg_sum_emit(c, k, nk, in_trace.batches.data(),
                         (int)in_trace.batches.size(), in_trace.wf64,
                         /*transient=*/true, ins));
        if (ins.n > 0) outs.push_back(ins);
        else free_batch(c, ins);
        // retractions ARE a join: probing the output trace with (key, _, -1)
        // rows under proj (k, v2) emits exactly (key, old_val, -old_w) — the
        // upsert contract (upsert.rs:180-195) — in one count/emit pair over
        // the whole spine instead of a scan pipeline per batch.
        TRY(out_trace.cap_batches(c));
        const TraceArgs t = trace_args_of(out_trace);
        if (t.nb > 0) {
            // synthetic delta columns: v = 0, w = -1
            ScratchBuf dv, dw;
            TRY(dv.alloc(c, (size_t)nk * 8 + 8, /*arena_first=*/true));
            TRY(dw.alloc(c, (size_t)nk * 8 + 8, /*arena_first=*/true));
            HIP_CHECK_ST(hipMemsetAsync(dv.p, 0, nk * 8, c->stream));
            HIP_CHECK_ST(hipMemsetAsync(dw.p, 0xFF, nk * 8, c->stream));  // -1
            const DevBatch probe{k, dv.as<uint64_t>(), dw.as<int64_t>(), nk};
            // by size: q4's handful of categories against C5's millions of keys
            DevBatch o;
            if (nk <= 8192)
                TRY(join_small(c, probe, t, DBSP_PROJ_HI_K_LO_V2, 0,
                               /*transient=*/true, o));
            else
                TRY(dbspk::join_spine_rows(c->stream, probe, t,
                                           DBSP_PROJ_HI_K_LO_V2, 0, &o));
            if (o.n > 0) outs.push_back(o);
            else free_batch(c, o);
        }
    }
    return finalize_raw(c, outs, out);
}

static bool spine_needs_merge(Spine &s) {
    size_t m = s.batches.size();
    return m >= 2 && s.batches[m - 1].n * 2 >= s.batches[m - 2].n;
}

// insert one delta into each of two spines, batching the two sides' pending
// merges into single launches with one shared length sync per round
// `hook` (optional) is the tick-pipelining point: it is invoked exactly once,
// after this tick's remaining work and length copies are queued and an event
// recorded, and the first wait is hipEventSynchronize on that event — so
// whatever the hook launches (the NEXT tick's front half) overlaps the
// host-side tail of this tick instead of extending its sync.
// run top-two merge rounds over the given spines until quiescent.  With
// `defer` set (train path), the FIRST batched small-merge round is enqueued,
// the hook fired behind it, and the length readback STASHED in the ctx
// instead of waited for: resolve_pending_insert() consumes it at the next
// insert/step on a near-empty stream.  Without it, a round that runs after
// the hook has enqueued the next tick's train would hipStreamSynchronize
// behind that entire train (~150 us) — the dominant host stall of the
// 40k-tick loop.
static dbsp_status spine_rounds(dbsp_ctx *c, Spine *const *sps, int ns,
                                const std::function<dbsp_status()> *hook,
                                bool *hook_fired, bool defer) {
    while (true) {
        Spine *pending[4];
        int nps = 0;
        for (int i = 0; i < ns && nps < 4; i++) {
            bool dup = false;
            for (int j = 0; j < nps; j++) dup |= pending[j] == sps[i];
            if (!dup && spine_needs_merge(*sps[i])) pending[nps++] = sps[i];
        }
        if (nps == 0) break;
        // two batched launch classes by pair size: tiny pairs (<= 4096
        // rows) go to the single-WG k_merge_small; mid pairs (<= 32768) to
        // the fixed-grid multi-WG merge_mid — a 32k single-WG merge costs
        // ~126 us where merge_mid does it in ~12 (q4's bid spine pushes
        // ~37k rows/tick, so these dominate its tick)
        MergeArgs ma{};   // small
        MergeArgs mm{};   // mid
        DevBatch results[4];
        Spine *owners[4];
        int slotofj[4];
        bool midofj[4];
        int nbatched = 0;
        for (int i = 0; i < nps; i++) {
            Spine &sp = *pending[i];
            DevBatch &top = sp.batches.back();
            DevBatch &below = sp.batches[sp.batches.size() - 2];
            const int64_t tot = top.n + below.n;
            if (tot <= 32768 && nbatched < MERGE_BATCH_MAX) {
                DevBatch res;
                TRY(alloc_batch(c, tot, res));
                MergeArgs &mx = tot <= 4096 ? ma : mm;
                merge_pair(mx, mx.np++, below, top, res);
                midofj[nbatched] = tot > 4096;
                results[nbatched] = res;
                owners[nbatched] = &sp;
                nbatched++;
            } else {
                DevBatch res;
                TRY(merge_batches(c, below, top, res));
                sp.replace_top2(c, res);
            }
        }
        if (nbatched > 0) {
            // dedicated insert slots (LEN_ROUND): the hook below may enqueue
            // the next tick's full train, whose LEN_TICK-slot readback would
            // otherwise overwrite the op slots before this round's merge
            // lengths are consumed after the event wait.  Slots: small pairs
            // first, then mid pairs.
            {
                int ps = 0, pm = ma.np;
                for (int j = 0; j < nbatched; j++)
                    slotofj[j] = midofj[j] ? pm++ : ps++;
            }
            ma.d_len = c->d_len + LEN_ROUND;
            mm.d_len = c->d_len + LEN_ROUND + ma.np;
            if (ma.np > 0) TRY(dbspk::merge_small_batch(c->stream, ma, false));
            if (mm.np > 0)
                TRY(dbspk::merge_mid_batch(c->stream, mm, c->d_mid, false));
            TRY(read_len(c, LEN_ROUND, ma.np + mm.np, /*sync=*/false));
            if (defer && hook && !*hook_fired) {
                (void)hipEventRecord(c->ev_insert, c->stream);
                TRY((*hook)());
                *hook_fired = true;
                c->pend_n = nbatched;
                for (int j = 0; j < nbatched; j++) {
                    c->pend_spine[j] = owners[j];
                    c->pend_k[j] = results[j].k;
                    c->pend_v[j] = results[j].v;
                    c->pend_w[j] = results[j].w;
                    c->pend_slot[j] = slotofj[j];
                }
                return DBSP_OK;  // pops + cascades resolved next tick
            }
            if (hook && !*hook_fired) {
                (void)hipEventRecord(c->ev_sync, c->stream);
                TRY((*hook)());
                *hook_fired = true;
                (void)hipEventSynchronize(c->ev_sync);
            } else {
                HIP_CHECK_ST(hipStreamSynchronize(c->stream));
            }
            for (int j = 0; j < nbatched; j++) {
                TRY(checked_len(c, LEN_ROUND + slotofj[j], results[j].n));
                owners[j]->replace_top2(c, results[j]);
            }
        }
    }
    return DBSP_OK;
}

// consume a deferred insert round: pop the merged pair, publish the result
// (length from the LEN_ROUND host slots, valid once ev_insert has fired), then run any
// cascade rounds synchronously — the stream is near-empty at every call
// site, so these cost only the merge kernels themselves
static dbsp_status resolve_pending_insert(dbsp_ctx *c) {
    if (!c->pend_n) return DBSP_OK;
    (void)hipEventSynchronize(c->ev_insert);
    Spine *owners[4];
    int no = 0;
    const int np = c->pend_n;
    c->pend_n = 0;
    for (int j = 0; j < np; j++) {
        Spine &sp = *(Spine *)c->pend_spine[j];
        DevBatch res{c->pend_k[j], c->pend_v[j], c->pend_w[j], 0};
        TRY(checked_len(c, LEN_ROUND + c->pend_slot[j], res.n));
        sp.replace_top2(c, res);
        bool dup = false;
        for (int i = 0; i < no; i++) dup |= owners[i] == &sp;
        if (!dup) owners[no++] = &sp;
    }
    return spine_rounds(c, owners, no, nullptr, nullptr, false);
}

// teardown guard: free a deferred round's result buffers without touching
// the spines (their batch lists are freed by their own teardown)
static void drop_pending_insert(dbsp_ctx *c) {
    if (!c->pend_n) return;
    (void)hipEventSynchronize(c->ev_insert);
    for (int j = 0; j < c->pend_n; j++) {
        DevBatch res{c->pend_k[j], c->pend_v[j], c->pend_w[j], 0};
        free_batch(c, res);
    }
    c->pend_n = 0;
}

static dbsp_status spines_insert_multi(dbsp_ctx *c, Spine *const *sps,
                                       DevBatch *bs, int ns,
                                       const std::function<dbsp_status()> *hook
                                       = nullptr, bool defer = false) {
    double bytes = 0;
    for (int i = 0; i < ns; i++) bytes += (double)bs[i].n * 48.0;
    ScopedTimer t(c, 1, bytes);
    TRY(resolve_pending_insert(c));
    bool hook_fired = false;
    for (int i = 0; i < ns; i++) {
        if (bs[i].n > 0) sps[i]->batches.push_back(bs[i]);
        else free_batch(c, bs[i]);
    }
    TRY(spine_rounds(c, sps, ns, hook, &hook_fired, defer));
    if (hook && !hook_fired) {
        (void)hipEventRecord(c->ev_sync, c->stream);
        TRY((*hook)());
        (void)hipEventSynchronize(c->ev_sync);
    }
    return DBSP_OK;
}

static dbsp_status spines_insert_pair(dbsp_ctx *c, Spine &s1, DevBatch b1,
                                      Spine &s2, DevBatch b2,
                                      const std::function<dbsp_status()> *hook
                                      = nullptr, bool defer = false) {
    Spine *sps[2] = {&s1, &s2};
    DevBatch bs[2] = {b1, b2};
    return spines_insert_multi(c, sps, bs, 2, hook, defer);
}

static void engine_free_output(dbsp_engine *e) {
    if (!e->output_is_store) free_batch(e->ctx, e->output);
    e->output = DevBatch{};
    e->output_is_store = false;
}

// ---- incremental partitioned rolling aggregate (rolling_aggregate.rs
// :487-604) ----
// Per tick, over a consolidated delta D of nd rows:
//   ranges   D -> merged gather ranges (p, [ts-before-after, ts+before+after])
//            and merged affected ranges (p, [ts-after, ts+before]); a time is
//            affected iff D has a row of its partition inside range_of(time),
//            which is the reference's affected_range_of merged with D's own
//            times (affected_ranges, rolling_aggregate.rs:436-456)
//   gather   in_sp rows inside the gather ranges (they cover the sum range
//            of every affected time), consolidated into one slice
//   eval     radix-16 tree over the slice; every affected slice row of
//            positive weight emits (p<<32|ts, sum over range_of(ts), +1)
//   retract  out_sp rows inside the affected ranges, weights negated
//   output   consolidate(retractions + insertions), appended to out_sp
// Cost follows the rows gathered, not the trace: O(nd log) searches per
// spine batch plus sort/tree/eval over the slice.  The explicit per-op path
// (host length syncs between phases, as q4/q6); no chaining.
dbsp_status RollingOp::step(dbsp_ctx *c, const DevBatch &delta, DevBatch &out) {
    out = DevBatch{};
    if (delta.n == 0) return DBSP_OK;
    ScopedTimer timer(c, 3, 0.0);
    const int64_t n = delta.n;
    // the range lists depend on the delta alone and their kernel raises the
    // precondition word, so they run before any state changes
    uint64_t *rb = nullptr;
    int64_t n_gather = 0, n_affected = 0;
    int err = 0;
    TRY(dbspk::roll_ranges(c->stream, delta, time_hi(), before, after, &rb,
                           &n_gather, &n_affected, &err));
    if (err) return DBSP_ERR_INVALID;
    TRY(in_sp.insert_copy(c, delta));
    TRY(in_sp.cap_batches(c));
    TRY(out_sp.cap_batches(c));
    // gather + consolidate the slice of the input integral
    DevBatch raw, slice;
    TRY(dbspk::range_gather(c->stream, rb, rb + n, rb + 2 * n, n_gather,
                            trace_args_of(in_sp), in_mode(), 1, &raw));
    int64_t moved = raw.n;
    TRY(sort_consolidate_batch(c, raw, slice));
    // insertions
    std::vector<DevBatch> parts;
    if (slice.n > 0) {
        DevBatch ins;
        if (time_hi())
            TRY(dbspk::roll_eval_minmax_rows(c->stream, slice, delta,
                                             agg == DBSP_ROLL_MIN, before,
                                             after, &ins));
        else
            TRY(dbspk::roll_eval_rows(c->stream, slice, delta, before, after,
                                      &ins));
        moved += ins.n;
        if (ins.n > 0) parts.push_back(ins);
    }
    free_batch(c, slice);
    // retractions
    {
        DevBatch ret;
        TRY(dbspk::range_gather(c->stream, rb + 3 * n, rb + 4 * n, rb + 5 * n,
                                n_affected, trace_args_of(out_sp), 1, -1, &ret));
        moved += 2 * ret.n;
        if (ret.n > 0) parts.push_back(ret);
    }
    HIP_CHECK_ST(dbspk::cache_free(rb, c->stream));
    if (!parts.empty()) TRY(finalize_raw(c, parts, out));
    if (out.n > 0) TRY(out_sp.insert_copy(c, out));
    timer.bytes = 24.0 * (double)moved;  // rows gathered + rows emitted
    return DBSP_OK;
}

// rows of one batch with time >= bound, in order (modes as truncate_spine)
static dbsp_status truncate_batch(dbsp_ctx *c, const DevBatch &in, int mode,
                                  uint64_t bound, DevBatch &out) {
    out = DevBatch{};
    if (in.n == 0) return DBSP_OK;
    return dbspk::truncate_spine(c->stream, trace_args_one(in), mode, bound,
                                 &out);
}

dbsp_status RollingOp::step_wm(dbsp_ctx *c, const DevBatch &delta, uint64_t x,
                               DevBatch &out) {
    out = DevBatch{};
    const uint64_t nwm = std::max(wm, x);
    int64_t dropped = 0;
    if (nwm > 0 && delta.n > 0) {
        // stable, so the survivors are still a consolidated delta
        DevBatch surv;
        TRY(truncate_batch(c, delta, in_mode(), nwm, surv));
        dropped = delta.n - surv.n;
        const dbsp_status st = step(c, surv, out);
        free_batch(c, surv);
        if (st != DBSP_OK) return st;
    } else {
        TRY(step(c, delta, out));
    }
    wm = nwm;
    late_rows += dropped;
    return sweep_policy(c);
}

dbsp_status RollingOp::sweep(dbsp_ctx *c, int mode) {
    Spine &sp = mode == 0 ? in_sp : out_sp;
    TRY(sp.cap_batches(c));
    const int nb = (int)sp.batches.size();
    if (nb > 0) {
        TraceArgs t{};  // every batch, empty ones too: outputs are per batch
        for (auto &b : sp.batches) trace_push(t, b);
        DevBatch kept[MAX_TRACE_BATCHES];
        TRY(dbspk::truncate_spine(c->stream, t, mode == 0 ? in_mode() : 1,
                                  lower_bound(), kept));
        std::vector<DevBatch> old;
        old.swap(sp.batches);
        for (auto &b : old) free_batch(c, b);
        // empty batches are dropped and the survivors (at most half of what
        // a policy sweep read) merged into one batch: rows are counted per
        // batch, so only a consolidated spine has live = rows, without
        // retraction/insertion pairs still waiting for a merge.  One batch
        // satisfies size[i] >= 2 * size[i+1] trivially.
        for (int b = 0; b < nb; b++)
            if (kept[b].n > 0) sp.batches.push_back(kept[b]);
        TRY(sp.consolidate_all(c));
    }
    (mode == 0 ? in_live : out_live) = sp.total();
    sweeps++;
    return DBSP_OK;
}

// Doubling rule: amortised O(1) per inserted row, and a spine never holds
// more than 2 * live + SWEEP_FLOOR plus the rows added since its last sweep.
dbsp_status RollingOp::sweep_policy(dbsp_ctx *c) {
    if (lower_bound() == 0) return DBSP_OK;  // no row can be below it
    if (in_sp.total() > 2 * in_live + SWEEP_FLOOR) TRY(sweep(c, 0));
    if (out_sp.total() > 2 * out_live + SWEEP_FLOOR) TRY(sweep(c, 1));
    return DBSP_OK;
}

struct dbsp_rolling {
    dbsp_ctx *ctx = nullptr;
    RollingOp op;
};

extern "C" dbsp_status dbsp_truncate_below(dbsp_ctx *c, const dbsp_batch *in,
                                           int mode, uint64_t bound,
                                           dbsp_batch *out) {
    if (!c || !in || !out || in->len < 0 || mode < 0 || mode > 2)
        return DBSP_ERR_INVALID;
    DevBatch ib{in->k, in->v, in->w, in->len}, res;
    TRY(truncate_batch(c, ib, mode, bound, res));
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    put_batch(out, res);
    return DBSP_OK;
}

static bool roll_agg_valid(dbsp_roll_agg agg) {
    return agg == DBSP_ROLL_SUM || agg == DBSP_ROLL_MAX ||
           agg == DBSP_ROLL_MIN;
}

extern "C" dbsp_status dbsp_rolling_create_agg(dbsp_ctx *c, dbsp_roll_agg agg,
                                               uint64_t before, uint64_t after,
                                               dbsp_rolling **out) {
    if (!c || !out || !roll_agg_valid(agg)) return DBSP_ERR_INVALID;
    dbsp_rolling *r = new dbsp_rolling();
    r->ctx = c;
    r->op.agg = agg;
    r->op.before = before;
    r->op.after = after;
    *out = r;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_rolling_create(dbsp_ctx *c, uint64_t before,
                                           uint64_t after, dbsp_rolling **out) {
    return dbsp_rolling_create_agg(c, DBSP_ROLL_SUM, before, after, out);
}

// Rolling Max / Min batch primitive (the radix tree with Agg::Semigroup =
// max | min, radix_tree/updater.rs:393 leaves, rolling_aggregate.rs:487-604
// queries): per row (partition, ts << 32 | val, w) of a consolidated batch,
// the extreme val over that partition's rows with time in
// [ts - before, ts + after], whatever their weight's sign.
extern "C" dbsp_status dbsp_rolling_minmax(dbsp_ctx *c, const dbsp_batch *in,
                                           dbsp_roll_agg agg, uint64_t before,
                                           uint64_t after, dbsp_batch *out) {
    if (!c || !in || !out || in->len < 0 ||
        (agg != DBSP_ROLL_MAX && agg != DBSP_ROLL_MIN))
        return DBSP_ERR_INVALID;
    DevBatch res;
    TRY(alloc_batch(c, in->len > 0 ? in->len : 1, res));
    {
        ScopedTimer t(c, 3, 0.0);
        TRY(dbspk::rolling_minmax_rows(c->stream, as_batch(in),
                                       agg == DBSP_ROLL_MIN, before, after,
                                       res));
    }
    res.n = in->len;
    put_batch(out, res);
    return DBSP_OK;
}

// a step that does not advance the watermark: step_wm with watermark 0
extern "C" dbsp_status dbsp_rolling_step(dbsp_rolling *r, const uint64_t *k,
                                         const uint64_t *v, const int64_t *w,
                                         int64_t n, dbsp_batch *out) {
    if (!r || !out || n < 0) return DBSP_ERR_INVALID;
    *out = dbsp_batch{nullptr, nullptr, nullptr, 0};
    if (n == 0) return DBSP_OK;
    return dbsp_rolling_step_wm(r, k, v, w, n, 0, out);
}

extern "C" dbsp_status dbsp_rolling_step_wm(dbsp_rolling *r, const uint64_t *k,
                                            const uint64_t *v,
                                            const int64_t *w, int64_t n,
                                            uint64_t watermark,
                                            dbsp_batch *out) {
    if (!r || !out || n < 0) return DBSP_ERR_INVALID;
    dbsp_ctx *c = r->ctx;
    *out = dbsp_batch{nullptr, nullptr, nullptr, 0};
    DevBatch raw, delta, res;
    if (n > 0) {
        TRY(alloc_batch(c, n, raw));
        TRY(copy_cols(c, raw, 0, k, v, w, n));
        TRY(sort_consolidate_batch(c, raw, delta));
    }
    const dbsp_status st = r->op.step_wm(c, delta, watermark, res);
    free_batch(c, delta);
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    if (st != DBSP_OK) return st;
    if (res.n == 0) free_batch(c, res);
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_rolling_stats(dbsp_rolling *r, int64_t *in_rows,
                                          int *in_batches, int64_t *out_rows,
                                          int *out_batches) {
    if (!r) return DBSP_ERR_INVALID;
    if (in_rows) *in_rows = r->op.in_sp.total();
    if (in_batches) *in_batches = (int)r->op.in_sp.batches.size();
    if (out_rows) *out_rows = r->op.out_sp.total();
    if (out_batches) *out_batches = (int)r->op.out_sp.batches.size();
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_rolling_compact(dbsp_rolling *r) {
    if (!r) return DBSP_ERR_INVALID;
    TRY(r->op.sweep(r->ctx, 0));
    TRY(r->op.sweep(r->ctx, 1));
    HIP_CHECK_ST(hipStreamSynchronize(r->ctx->stream));
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_rolling_wm_stats(dbsp_rolling *r,
                                             uint64_t *watermark,
                                             uint64_t *lower_bound,
                                             int64_t *late_rows,
                                             int64_t *sweeps) {
    if (!r) return DBSP_ERR_INVALID;
    if (watermark) *watermark = r->op.wm;
    if (lower_bound) *lower_bound = r->op.lower_bound();
    if (late_rows) *late_rows = r->op.late_rows;
    if (sweeps) *sweeps = r->op.sweeps;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_rolling_destroy(dbsp_rolling *r) {
    if (!r) return DBSP_OK;
    r->op.clear(r->ctx);
    (void)hipStreamSynchronize(r->ctx->stream);
    delete r;
    return DBSP_OK;
}

// ---- query 101: per-auction rolling bid volume ----
// bids.map_index(|b| (b.auction, (b.date_time, b.price)))
//     .partitioned_rolling_aggregate_linear(...)   (the q17-class shape):
// the flatmap weighs the price into the weight, one stream through
// build_deltas (which also exchanges by auction on sharded ranks:
// partitions are independent), then the operator.
// ---- query 102: per-auction rolling highest (or lowest) bid ----
// the same map_index into .partitioned_rolling_aggregate(Max | Min, range):
// the flatmap keeps the price as the value, v = date_time << 32 | price, and
// everything else is query 101's step with the operator's other aggregator.
static bool is_rolling_query(int query) { return query == 101 || query == 102; }

static dbsp_status q101_step(dbsp_engine *e, const dbsp_event *d_ev,
                             int64_t n) {
    dbsp_ctx *c = e->ctx;
    engine_free_output(e);
    e->roll_stepped = true;
    DevBatch d, dummy;
    TRY(build_deltas(e, d_ev, n, d, dummy, false));
    dbsp_status st;
    if (e->roll_lateness_on) {
        // watermark_monotonic(|ts| ts.saturating_sub(lateness)) (watermark.rs
        // :33-75): the maximum includes this tick's own rows; step_wm keeps
        // it monotone.  Sharded ranks see their own bids only, so each rank
        // runs on its rank-local watermark: no collective.
        uint64_t x = 0;
        if (d.n > 0) {
            uint64_t mm[4];
            TRY(dbspk::minmax_rows(c->stream, d, mm));
            // the largest time seen: v itself, or its upper half
            const uint64_t tmax = e->roll.time_hi() ? mm[3] >> 32 : mm[3];
            x = tmax > e->roll_lateness ? tmax - e->roll_lateness : 0;
        }
        st = e->roll.step_wm(c, d, x, e->output);
    } else {
        st = e->roll.step(c, d, e->output);
    }
    free_batch(c, d);
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    return st;
}

extern "C" dbsp_status dbsp_engine_rolling_lateness(dbsp_engine *e,
                                                    uint64_t lateness_ms) {
    if (!e || !is_rolling_query(e->query) || e->roll_stepped)
        return DBSP_ERR_INVALID;
    e->roll_lateness = lateness_ms;
    e->roll_lateness_on = true;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_engine_rolling_stats(dbsp_engine *e,
                                                 int64_t *in_rows,
                                                 int64_t *out_rows,
                                                 int64_t *late_rows,
                                                 int64_t *sweeps) {
    if (!e || !is_rolling_query(e->query)) return DBSP_ERR_INVALID;
    if (in_rows) *in_rows = e->roll.in_sp.total();
    if (out_rows) *out_rows = e->roll.out_sp.total();
    if (late_rows) *late_rows = e->roll.late_rows;
    if (sweeps) *sweeps = e->roll.sweeps;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_engine_rolling_init(dbsp_engine *e,
                                                uint64_t before_ms,
                                                uint64_t after_ms) {
    if (!e || !is_rolling_query(e->query) || e->roll_stepped)
        return DBSP_ERR_INVALID;
    e->roll.before = before_ms;
    e->roll.after = after_ms;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_engine_rolling_agg(dbsp_engine *e,
                                               dbsp_roll_agg agg) {
    if (!e || e->query != 102 || e->roll_stepped ||
        (agg != DBSP_ROLL_MAX && agg != DBSP_ROLL_MIN))
        return DBSP_ERR_INVALID;
    e->roll.agg = agg;
    return DBSP_OK;
}

// ---- q3 tick (queries/q3.rs:35-63) ----
//
// Single-rank ticks run almost entirely as ONE chained launch train with
// device-side lengths:
//   flatmap -> fused delta sorts (speculative, -1 sentinel over 8192 rows)
//   -> 3-plan join probe (counts and run start positions per delta row and
//   spine batch) -> join tail, one single-workgroup kernel: scan of the
//   counts, capacity check, emit into a capacity buffer, output consolidate
//   into the reused store.
// A chained tick reads lengths back twice.  The HEAD readback (raw and delta
// lengths, and on trains the accumulator-merge lengths) is final once the
// delta sorts are; the host wakes at an EVENT recorded right after it —
// while the GPU still runs the probe and the tail — checks the speculation
// from the delta lengths, and immediately queues the spine inserts (whose
// first wait doubles as the pipelining point launching the NEXT tick's
// front).  The TAIL readback (plan totals, emit total / overflow flag,
// output length) is consumed after the inserts.  Emit overflow (combined
// output beyond the capacity buffer) and output overflow (beyond the fused
// sort) are detected there and replayed explicitly from the tail kernel's
// offsets and totals; a plan total that is negative although the delta
// lengths passed is re-counted by that replay.  A lost sort speculation
// re-sorts through the sized paths.  Sharded ranks keep the explicit path
// (the exchange needs host lengths).
//
// Pipelined TRAINS: for run_staged loops the ENTIRE next tick's launch train
// is enqueued at the END of the current step, right after the spine inserts
// commit — at that point the post-insert spine state the next tick's probes
// must read is final, so the train's TraceArgs are correct by construction.
// The next step then only WAITS on the train's events and runs verdicts +
// the accumulator swap, so the per-tick host enqueue work overlaps the
// previous train's GPU execution.  Trains ping-pong the length-slot bases
// (LEN_BASE0 / LEN_BASE1), the events and the arena halves; the
// spine-insert rounds use the LEN_ROUND slots.
//
// The train forks.  The host's loop is: wake on ev_tick(t), verdict + swap,
// enqueue train t+1, whose ev_tick it wakes on next.  What that loop waits
// for — flatmap, delta sorts, the accumulator fold, the head readback — is
// one stream with nothing else in it; what nobody waits for until the
// commit's end — probe, join tail, tail readback — runs beside it:
//   loop (c->stream): flatmap (no fill) -> delta sorts (take) -> record
//                     ev_fork -> fold -> head readback -> record ev_tick
//   back (c->side):   wait ev_fork -> probe -> join tail -> tail readback
//                     -> record ev_tail
// The hook enqueues all loop-stream work first, through ev_tick, then the
// back-stream work.  Nothing flatmap(t+1) or sort(t+1) touches is produced
// by probe(t) or tail(t), so on the common path the loop stream never waits
// for the back stream.
// Ordering argument (what buffer recycling and slot reuse rest on).  The
// free list hands a freed block to the next allocation at once, so reuse is
// safe only where stream order, or a completion the host has observed,
// separates the users.
//  1. Back-stream work of train t+1 waits ev_fork(t+1).  So it follows
//     everything enqueued on the loop stream before it: fold(t), every
//     kernel of commit t (spill rounds, replays of an earlier tick), and
//     flatmap and sorts of t+1.  The back stream runs in order, so it also
//     follows all of back(t).
//  2. The loop stream follows back-stream work only through a JOIN ON DEMAND
//     (q3_join_back: the loop stream waits the last ev_tail recorded, which
//     covers the whole back stream; q3_sync_back where the host must be
//     behind it) or through the commit's own hipEventSynchronize(ev_tail(t)).
//     What back(t) uses: reads the deltas oA/oP(t), every spine batch listed
//     at the enqueue of train t, and d_len[sb + L_DELTA]; reads and writes
//     its arena buffers (cnts, starts, offsets, comb_chain, scr); writes
//     out_store and d_len[sb + L_PLAN .. L_FINAL] — at base 0 those are the
//     LEN_OP slots every sized op borrows — and h_len[sb + LH_*].  Every
//     loop-stream path that frees, recycles or overwrites one of these while
//     a train may be in flight joins first:
//       - Spine::replace_top2, the one place spine batches are freed: the
//         deferred round's resolve at the top of the commit (with its
//         cascade rounds), the immediate merges of a spill round, the
//         consolidate_all calls of the enqueue and of the unpipelined body,
//         the rounds an unpipelined insert runs after its hook.  The first
//         three also join explicitly, ahead of their sized merges' LEN_OP
//         use;
//       - the lost-speculation branch of the commit, before it drops the
//         deltas and replays (sized sorts, possibly a new out_store);
//       - both overflow replays of q3_publish_chained: tail(t) is complete
//         there, but train t+1 is enqueued and its tail writes base 0's
//         first slots when t+1 runs at base 0;
//       - a train that bails after forking (records ev_tail, joins);
//       - a stale train, and engine and context teardown (host syncs).
//     Safe without a join: the frees after q3_publish_chained (the host has
//     synced ev_tail(t); train t+1 reads none of them), free_batch of an
//     empty fold result (loop-stream order), the batched merges of a spill
//     round (they read what the back stream reads, write fresh blocks and
//     use the LEN_ROUND slots and d_mid, which the back stream never
//     touches), and engine_free_output (a replay's output, loop-stream work).
//  3. Length slots: train t+2 reuses the base and the events of train t, and
//     is enqueued by commit t+1, after commit t synced ev_tail(t).
//  4. ARENA RULE: consecutive trains bump from offset 0 of opposite halves,
//     and commit t continues behind train t's transients in t's half.  So a
//     loop-stream write of train t+1 (raw streams, sort scratch) is in the
//     half back(t) does not use, commit-side transients of t lie above
//     everything train t allocated, and train t+2 — same half as t — is
//     enqueued after the host synced ev_tail(t), behind commit t's
//     transients in loop-stream order.  This also keeps plans[].cnts and
//     plans[].offsets of tick t intact for an emit-overflow replay at its
//     publish: with both trains bumping from offset 0 of one half, as
//     before, probe(t+1) overwrote them ahead of the replay whenever the two
//     ticks had the same size.
//
// Counter hand-back: a train's delta sorts TAKE the flatmap's two ticket
// counters (L_RAW of the train's base): each sort block reads its counter,
// leaves the length at L_RAWN of the same base and writes 0 back.  So the
// next flatmap on that base is launched without a counter fill
// (dbsp_ctx::raw_zero says when that holds; every path that runs a plain
// sort behind its flatmap keeps the fill and leaves the flag clear).
// Ordering: flatmap(t) and the taking sort(t) are consecutive loop-stream
// launches.  Between that sort and the next flatmap on the same base — a
// later train's, or a single step's on base 0, loop-stream work behind it
// either way — nothing reads or writes the two counters: the back stream
// touches neither, the head readback copies the base's head range, where it finds the lengths at
// L_RAWN (the L_RAW words it also copies are dead), a lost speculation
// replays from H[L_RAWN], and no op scratch slot aliases L_RAW
// (static_assert above).  If the invariant broke anyway, the counters would
// overshoot: the flatmap stores nothing at or past its capacity, the taking
// sort poisons a count above the capacity, and the replay refuses a raw
// count above the tick's event count.
// Under DBSP_PROFILE (ScopedTimer's events assume one stream) and with
// DBSP_Q3_FORK=0 the back-stream work stays on the loop stream, in the order
// of the layout above, and no join is ever needed.
//
// Per-tick stepping (no next_ev), sharded ranks, oversized ticks and lost
// speculations all run the unpipelined body below: the same probe and join
// tail in order on the loop stream when chained, the explicit path otherwise.

static constexpr int64_t Q3_EMIT_CAP = 32768;

// Build the three bilinear join plans against the CURRENT spines (callers
// guarantee the spine state is the one tick t's probes must read) and
// enqueue the probe (spec: delta lengths still on device, L_DELTA of sb; the
// probe keeps the start positions for the join tail) or count+scan (host
// lengths) on stream s.
static dbsp_status q3_plan_count(dbsp_engine *e, hipStream_t s, DevBatch &dA,
                                 DevBatch &dP, bool spec, int sb,
                                 int64_t n_cap, Q3Plan plans[3], int &np,
                                 int &jca_np, bool &arena_ok) {
    dbsp_ctx *c = e->ctx;
    np = 0;
    arena_ok = true;
    const bool haveA = spec || dA.n > 0, haveP = spec || dP.n > 0;
    if (haveA && !e->p_int.batches.empty())
        plans[np++] = {0, trace_args_of(e->p_int), DBSP_PROJ_HI_V2_LO_V1,
                       nullptr, nullptr, nullptr, false, false, -1};
    if (haveP && !e->a_int.batches.empty())
        plans[np++] = {1, trace_args_of(e->a_int), DBSP_PROJ_HI_V1_LO_V2,
                       nullptr, nullptr, nullptr, false, false, -1};
    if (haveA && haveP) {
        TraceArgs t = trace_args_one(dP);
        if (spec) t.n[0] = 0;  // read from the device (tn_dev below)
        plans[np++] = {0, t, DBSP_PROJ_HI_V2_LO_V1, nullptr, nullptr, nullptr,
                       false, true, -1};
    }
    JoinCountArgs jca{};
    for (int i = 0; i < np; i++) {
        Q3Plan &pl = plans[i];
        pl.slot = -1;
        if (pl.t.nb == 0) continue;
        DevBatch &d = pl.which == 0 ? dA : dP;
        const int64_t nd_cap = spec ? n_cap : d.n;
        pl.cnts = (uint32_t *)arena_alloc(c, (size_t)nd_cap * pl.t.nb * 4 + 8);
        pl.offsets = (uint64_t *)arena_alloc(c, (size_t)(nd_cap + 1) * 8);
        pl.starts = nullptr;
        if (spec)
            pl.starts =
                (int64_t *)arena_alloc(c, (size_t)nd_cap * pl.t.nb * 8 + 8);
        const bool bufs = pl.cnts && pl.offsets && (!spec || pl.starts);
        if (spec && !bufs) {
            arena_ok = false;
            break;
        }
        if (bufs && (spec || nd_cap <= 8192)) {
            pl.small = true;
            pl.slot = jca.np;
            jca.dk[jca.np] = d.k;
            jca.nd[jca.np] = spec ? 0 : d.n;
            if (spec) jca.nd_dev[jca.np] = c->d_len + sb + L_DELTA + pl.which;
            if (spec && pl.dd) jca.tn_dev[jca.np] = c->d_len + sb + L_DELTA + 1;
            jca.t[jca.np] = pl.t;
            jca.cnts[jca.np] = pl.cnts;
            jca.starts[jca.np] = pl.starts;
            jca.offsets[jca.np] = pl.offsets;
            jca.np++;
        }
    }
    jca_np = jca.np;
    if (arena_ok) {
        jca.d_total = c->d_len + sb + L_PLAN;
        // a chained tick only probes here: its join tail scans the counts
        if (jca.np > 0 && spec) TRY(dbspk::join_probe_batch(s, jca));
        if (jca.np > 0 && !spec) TRY(dbspk::join_count_scan_batch(s, jca));
    }
    return DBSP_OK;
}

// the join tail behind a chained probe: scan + emit into a capacity buffer +
// output consolidate into the reused store, one launch on stream s.  Kernel
// only — the caller queues the tail readback (q3_read_tail) behind it.
// ok=false: arena exhausted, nothing was launched.
static dbsp_status q3_chain_tail(dbsp_engine *e, hipStream_t s, DevBatch &dA,
                                 DevBatch &dP, Q3Plan plans[3], int np, int sb,
                                 DevBatch &comb_chain, bool &ok) {
    dbsp_ctx *c = e->ctx;
    ok = false;
    DevBatch scr;
    if (alloc_batch(c, Q3_EMIT_CAP, comb_chain, true) != DBSP_OK ||
        alloc_batch(c, 8192, scr, true) != DBSP_OK)
        return DBSP_OK;  // arena exhausted: caller keeps the explicit path
    if (!e->out_store.k) {
        e->out_cap = 8192;
        TRY(alloc_batch(c, e->out_cap, e->out_store));
    }
    JoinTailArgs ta{};
    for (int i = 0; i < np; i++) {
        Q3Plan &pl = plans[i];
        if (pl.slot < 0) continue;
        DevBatch &d = pl.which == 0 ? dA : dP;
        const int s2 = pl.slot;
        ta.np = std::max(ta.np, s2 + 1);
        ta.dk[s2] = d.k;
        ta.dv[s2] = d.v;
        ta.dw[s2] = d.w;
        ta.nd_dev[s2] = c->d_len + sb + L_DELTA + pl.which;
        ta.t[s2] = pl.t;
        ta.tn_dev[s2] = pl.dd ? c->d_len + sb + L_DELTA + 1 : nullptr;
        ta.cnts[s2] = pl.cnts;
        ta.starts[s2] = pl.starts;
        ta.offsets[s2] = pl.offsets;
        ta.proj[s2] = pl.proj;
    }
    ta.totals = c->d_len + sb + L_PLAN;
    ta.cap = Q3_EMIT_CAP;
    ta.d_total = c->d_len + sb + L_EMIT_TOTAL;
    ta.d_flag = c->d_len + sb + L_EMIT_FLAG;
    ta.d_final = c->d_len + sb + L_FINAL;
    ta.ek = comb_chain.k;
    ta.ev = comb_chain.v;
    ta.ew = comb_chain.w;
    ta.tk = scr.k;
    ta.tv = scr.v;
    ta.tw = scr.w;
    ta.ok = e->out_store.k;
    ta.ov = e->out_store.v;
    ta.ow = e->out_store.w;
    TRY(dbspk::join_tail_small(s, ta));
    ok = true;
    return DBSP_OK;
}
// the tail readback on stream s: device L_PLAN..L_FINAL of base sb -> host
// LH_*
static inline dbsp_status q3_read_tail(dbsp_ctx *c, hipStream_t s, int sb) {
    return read_len_to(c, sb + LH_PLAN, sb + L_PLAN, LH_TAIL_N,
                       /*sync=*/false, s);
}

// explicit emits from prepared counts/offsets (the non-chained path and the
// emit-overflow replay)
static dbsp_status q3_emit_explicit(dbsp_engine *e, DevBatch &dA, DevBatch &dP,
                                    Q3Plan plans[3], int np,
                                    const int64_t slot_totals[3],
                                    std::vector<DevBatch> &outs) {
    dbsp_ctx *c = e->ctx;
    ScopedTimer timer(c, 2, 0.0);
    int64_t total_small = 0;
    for (int i = 0; i < np; i++)
        if (plans[i].t.nb > 0 && plans[i].small)
            total_small += slot_totals[plans[i].slot];
    DevBatch comb;
    if (total_small > 0) TRY(alloc_batch(c, total_small, comb, true));
    int64_t base = 0;
    for (int i = 0; i < np; i++) {
        Q3Plan &pl = plans[i];
        if (pl.t.nb == 0) continue;
        DevBatch &d = pl.which == 0 ? dA : dP;
        if (pl.small) {
            int64_t total = slot_totals[pl.slot];
            if (total <= 0) continue;
            TRY(dbspk::join_emit_prepared(
                c->stream, d, pl.t, pl.cnts, pl.offsets, total, pl.proj, 0,
                DevBatch{comb.k + base, comb.v + base, comb.w + base, total}));
            base += total;
        } else {
            DevBatch o;
            TRY(dbspk::join_spine_rows(c->stream, d, pl.t, pl.proj, 0, &o));
            if (o.n > 0) outs.push_back(o);
            else free_batch(c, o);
        }
    }
    if (total_small > 0) {
        comb.n = total_small;
        outs.push_back(comb);
    } else if (comb.k) {
        free_batch(c, comb);
    }
    return DBSP_OK;
}

static void q3_maybe_enqueue_train(dbsp_engine *e);

// ---- tick pieces shared by q3 / q5 / q8 ----

static inline void publish_store(dbsp_engine *e, int64_t n) {
    e->output = e->out_store;
    e->output.n = n;
    e->output_is_store = true;
}

// Asynchronous final consolidate, first half: when the tick's raw result
// rows fit one workgroup (and `allow`), gather them and launch the fused
// sort into the reused out_store, with its length copy queued but not
// waited for — the spine inserts that follow overlap it and their sync
// covers the copy.  Otherwise outs is left for final_finish.
static dbsp_status final_begin(dbsp_engine *e, std::vector<DevBatch> &outs,
                               bool allow, bool &async) {
    dbsp_ctx *c = e->ctx;
    int64_t cat_n = 0;
    for (auto &b : outs) cat_n += b.n;
    async = allow && cat_n > 0 && cat_n <= 8192;
    if (!async) return DBSP_OK;
    ScopedTimer t0(c, 0, (double)cat_n * 48.0);
    DevBatch cat, scratch;
    TRY(gather_raw(c, outs, cat));
    TRY(alloc_batch(c, cat_n, scratch, true));
    if (e->out_cap < cat_n) {
        if (e->out_store.k) free_batch(c, e->out_store);
        e->out_cap = std::max<int64_t>(2 * cat_n, 8192);
        TRY(alloc_batch(c, e->out_cap, e->out_store));
    }
    SortArgs sa{};
    sa.nb = 1;
    sort_slot(sa, 0, cat, scratch, e->out_store);
    sa.d_len = c->d_len + L_FINAL;
    TRY(dbspk::sort_cons_small_batch(c->stream, sa, false));
    return read_len(c, L_FINAL, 1, /*sync=*/false);
}
// second half, after the inserts: publish the store with the length that
// has landed by now, or consolidate outs through the sized paths
static dbsp_status final_finish(dbsp_engine *e, std::vector<DevBatch> &outs,
                                bool async) {
    if (!async) return finalize_raw(e->ctx, outs, e->output);
    publish_store(e, e->ctx->h_len[L_FINAL]);
    return DBSP_OK;
}

// speculation verdict of a chained q3 tick from its head readback (H = the
// host slots of its base): a delta overflowed the fused sort.  The plan
// totals are not in yet, and are not needed: a plan's total is negative only
// if a delta length it read was.
static bool q3_spec_lost(const int64_t *H) {
    return H[L_DELTA] < 0 || H[L_DELTA + 1] < 0;
}

// publish a chained q3 tick's output from its tail readback (host LH_*
// slots of base sb; the caller has waited past it)
static dbsp_status q3_publish_chained(dbsp_engine *e, int sb, DevBatch &dA,
                                      DevBatch &dP, Q3Plan plans[3], int np,
                                      DevBatch &comb_chain) {
    dbsp_ctx *c = e->ctx;
    int64_t H[LEN_BASE_N];  // the replay's sized ops reuse h_len
    memcpy(H, c->h_len + sb, sizeof(H));
    // Both replays below run sized ops, which borrow the LEN_OP slots: the
    // first offsets of base 0, where the join tail of a NEXT train already
    // enqueued at that base leaves its totals.  Join it first (overflow
    // ticks only).
    if (H[LH_EMIT_FLAG] != 0 || H[LH_FINAL] < 0) q3_join_back(c);
    if (H[LH_EMIT_FLAG] != 0) {
        // combined emits exceeded the capacity buffer: replay explicitly
        // from the tail kernel's counts/offsets/totals.  A plan whose total
        // came back negative although the delta lengths had passed has no
        // offsets: it is re-counted from scratch with the host lengths.
        int64_t slot_totals[3] = {0, 0, 0};
        for (int i = 0; i < np; i++) {
            if (plans[i].slot < 0) continue;
            slot_totals[plans[i].slot] = H[LH_PLAN + plans[i].slot];
            if (slot_totals[plans[i].slot] < 0) plans[i].small = false;
        }
        std::vector<DevBatch> outs;
        TRY(q3_emit_explicit(e, dA, dP, plans, np, slot_totals, outs));
        return finalize_raw(c, outs, e->output);
    }
    if (H[LH_FINAL] >= 0) {
        publish_store(e, H[LH_FINAL]);
        return DBSP_OK;
    }
    // the output overflowed the fused sort: sized sort of the emitted rows
    comb_chain.n = H[LH_EMIT_TOTAL];
    return sort_consolidate_batch(c, comb_chain, e->output);
}

// the unpipelined tick body (round-1 path): deltas are already built;
// plans/count/emits run in-step at slot base 0
static dbsp_status q3_body(dbsp_engine *e, const dbsp_event *d_ev, int64_t n,
                           DevBatch dA, DevBatch dP, DevBatch rawA,
                           DevBatch rawP, DevBatch recvA, DevBatch recvP,
                           bool chain, bool shard_chain) {
    dbsp_ctx *c = e->ctx;
    const int64_t *H = c->h_len + LEN_BASE0;
    std::vector<DevBatch> outs;
    bool chain_emits = false;
    DevBatch comb_chain{};
    int64_t slot_totals[3] = {0, 0, 0};
    Q3Plan plans[3];
    int np = 0;
    {
        ScopedTimer timer(c, 2, (double)n * 24.0);
        TRY(e->p_int.cap_batches(c));
        TRY(e->a_int.cap_batches(c));
        bool spec = chain;
        for (;;) {
            int jca_np = 0;
            bool arena_ok = true;
            TRY(q3_plan_count(e, c->stream, dA, dP, spec, LEN_BASE0, n, plans,
                              np, jca_np, arena_ok));
            // chained: the head readback carries the delta lengths; the
            // host wakes at an event recorded right after the copy, with
            // the join tail and its own readback queued behind it.
            // Explicit: one synced readback carries the plan totals.
            const bool emits = spec && arena_ok && jca_np > 0;
            if (emits) {
                TRY(read_len(c, LEN_BASE0 + L_HEAD, L_HEAD_N, /*sync=*/false));
                (void)hipEventRecord(c->ev_sync2, c->stream);
                TRY(q3_chain_tail(e, c->stream, dA, dP, plans, np, LEN_BASE0,
                                  comb_chain, chain_emits));
                if (chain_emits) TRY(q3_read_tail(c, c->stream, LEN_BASE0));
                (void)hipEventSynchronize(c->ev_sync2);
            } else {
                TRY(read_len(c, LEN_BASE0, LEN_TICK));
            }
            for (int i = 0; i < np && i < 3; i++)
                slot_totals[i] = H[L_PLAN + i];
            if (!spec) break;
            if (emits && !q3_spec_lost(H)) {
                dA.n = H[L_DELTA];
                dP.n = H[L_DELTA + 1];
                e->spec_fail = 0;
                if (chain_emits) break;
                // no room for the tail's buffers: nothing scanned the
                // probe's counts, so count again explicitly, host lengths
                spec = false;
                continue;
            }
            // lost: rebuild the deltas with host lengths from the furthest
            // stage that held (received frames, else the raw streams), then
            // go round once more without speculation
            e->spec_fail++;
            chain_emits = false;  // the chained emits bailed on the flag
            free_batch(c, dA);
            free_batch(c, dP);
            if (shard_chain && H[L_XCHG] >= 0 && H[L_XCHG + 1] >= 0) {
                recvA.n = H[L_XCHG];
                recvP.n = H[L_XCHG + 1];
                TRY(sort_consolidate_batch(c, recvA, dA));
                TRY(sort_consolidate_batch(c, recvP, dP));
            } else {
                rawA.n = H[L_RAW];
                rawP.n = H[L_RAW + 1];
                if (shard_chain) {
                    TRY(shard_exchange_pair(c, rawA, rawP, dA, dP));
                } else {
                    TRY(sort_consolidate_batch(c, rawA, dA));
                    TRY(sort_consolidate_batch(c, rawP, dP));
                }
            }
            rawA = rawP = recvA = recvP = DevBatch{};
            spec = false;
        }
        for (int i = 0; i < np; i++)
            if (plans[i].dd) plans[i].t.n[0] = dP.n;
    }
    engine_free_output(e);
    // The hook enqueues the NEXT tick's train mid-insert (after this tick's
    // merge launches, before their wait): probing the pre-cascade batch
    // list is Z-set-identical to the merged state, and the round's
    // replace_top2 joins the back stream before it frees that list (rule 2
    // above the q3 tick).  The insert's event sync
    // (recorded pre-hook) covers this tick's readbacks, so the length reads
    // after it are complete.  Sharded ranks run no trains.
    std::function<dbsp_status()> hook = [&]() -> dbsp_status {
        q3_maybe_enqueue_train(e);
        return DBSP_OK;
    };
    // a classic insert re-levels the spine: the accumulator identity is
    // lost (a train enqueued by the hook merges from empty)
    e->q3_acc[0] = e->q3_acc[1] = DevBatch{};
    if (chain_emits) {
        TRY(spines_insert_pair(c, e->a_int, dA, e->p_int, dP, &hook));
        return q3_publish_chained(e, LEN_BASE0, dA, dP, plans, np, comb_chain);
    }
    // explicit path (sharded ranks and lost speculations)
    TRY(q3_emit_explicit(e, dA, dP, plans, np, slot_totals, outs));
    bool async_final = false;
    TRY(final_begin(e, outs, true, async_final));
    if (!sharding_on(c)) {
        TRY(spines_insert_pair(c, e->a_int, dA, e->p_int, dP, &hook));
    } else {
        TRY(spines_insert_pair(c, e->a_int, dA, e->p_int, dP));
        // no hook, so no event wait that covers the length copy
        if (async_final) HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    }
    return final_finish(e, outs, async_final);
}

// enqueue the NEXT tick's full train (called after this tick's inserts have
// committed, so the spine state its probes bake in is final)
static dbsp_status q3_enqueue_train(dbsp_engine *e, const dbsp_event *d_ev,
                                    int64_t n) {
    dbsp_ctx *c = e->ctx;
    Q3Train &T = e->train;
    const int sb = T.next_sb;
    const int evi = T.next_evi;
    const size_t save_base = c->arena_base, save_off = c->arena_off;
    arena_other_half(c, save_base);
    auto bail = [&](void) {
        q3_train_drop(c, T);
        c->arena_base = save_base;
        c->arena_off = save_off;
        T.pending = false;
    };
    if (g_hook_prof) {
        memset(g_hook_us, 0, sizeof(g_hook_us));
        g_hook_t = host_us();
    }
    // the delta sorts TAKE the flatmap's counters (lengths to L_RAWN,
    // counters handed back zeroed), so this base's next flatmap needs no
    // counter fill: see "counter hand-back" above the q3 tick
    dbsp_status st = build_deltas_chain(e, d_ev, n, T.rawA, T.rawP, T.oA,
                                        T.oP, sb, /*take=*/c->q3_take);
    if (st != DBSP_OK) {
        bail();
        return st;
    }
    // consolidating frees every batch of the spine, which the previous
    // train's probe may still read, and its sized merges borrow the LEN_OP
    // slots that a join tail at base 0 writes: join the back stream first
    if ((int)e->p_int.batches.size() > MAX_TRACE_BATCHES) {
        q3_join_back(c);
        TRY(e->p_int.consolidate_all(c));
        e->q3_acc[1] = DevBatch{};
    }
    if ((int)e->a_int.batches.size() > MAX_TRACE_BATCHES) {
        q3_join_back(c);
        TRY(e->a_int.consolidate_all(c));
        e->q3_acc[0] = DevBatch{};
    }
    // in-train accumulator merge: fold this tick's deltas into the per-spine
    // memtable (one 2-pair launch; delta lengths read from the d_len slots
    // the chain just wrote, so nothing here waits).  The commit swaps the
    // spine top for the result — or, past the spill threshold, seals it as a
    // ladder batch.  The host waits for its lengths, so it stays on the loop
    // stream, followed there by the head readback the host wakes on; the
    // probe and the join tail, which nobody waits for until the commit's
    // end, fork to the back stream behind the sorts.
    const bool fork = c->q3_fork;
    hipStream_t back = fork ? c->side : c->stream;
    {
        MergeArgs ma{};
        for (int s = 0; s < 2; s++) {
            DevBatch &acc = e->q3_acc[s];
            if (alloc_batch(c, acc.n + n, T.res[s]) != DBSP_OK) {
                bail();
                return DBSP_OK;
            }
            // a delta has at most one row per event: res holds acc.n + n
            merge_pair(ma, s, acc, s == 0 ? T.oA : T.oP, T.res[s],
                       c->d_len + sb + L_DELTA + s, /*bcap=*/n);
            ma.np++;
        }
        hook_mark(HK_ALLOC);
        // result lengths ride in the base's L_XCHG pair (unused on the
        // unsharded train path), inside the head readback's range
        ma.d_len = c->d_len + sb + L_XCHG;
        ScopedTimer timer(c, 1, (double)(e->q3_acc[0].n + e->q3_acc[1].n +
                                         2 * n) * 48.0);
        // the fork point: behind the sorts, in front of the fold
        if (fork) HIP_CHECK_ST(hipEventRecord(c->ev_fork[evi], c->stream));
        hook_mark(HK_FORK);
        // the fold needs no scratch and no barrier between workgroups;
        // DBSP_Q3_FOLD=0 keeps the general merge here for comparison
        if (c->q3_fold)
            TRY(dbspk::acc_fold_batch(c->stream, ma, false));
        else
            TRY(dbspk::merge_mid_batch(c->stream, ma, c->d_mid, false));
        hook_mark(HK_MERGE);
    }
    TRY(read_len_to(c, sb + L_HEAD, sb + L_HEAD, L_HEAD_N, /*sync=*/false));
    HIP_CHECK_ST(hipEventRecord(c->ev_tick[evi], c->stream));
    hook_mark(HK_HEAD);
    // The loop stream's part ends here; the rest goes to the back stream.
    // A bail from here on puts the loop stream behind what the back stream
    // got: the next step's unpipelined body recycles the train's buffers.
    if (fork) HIP_CHECK_ST(hipStreamWaitEvent(back, c->ev_fork[evi], 0));
    auto bail_joined = [&](void) {
        if (fork) {
            (void)hipEventRecord(c->ev_tail[evi], back);
            c->back_live = evi;
            q3_join_back(c);
        }
        bail();
    };
    int jca_np = 0;
    bool arena_ok = true;
    {
        ScopedTimer timer(c, 2, (double)n * 24.0);
        TRY(q3_plan_count(e, back, T.oA, T.oP, true, sb, n, T.plans, T.np,
                          jca_np, arena_ok));
    }
    hook_mark(HK_PROBE);
    if (!arena_ok || jca_np == 0) {
        bail_joined();
        return DBSP_OK;  // fall back: next step runs the unpipelined body
    }
    bool tail_ok = false;
    TRY(q3_chain_tail(e, back, T.oA, T.oP, T.plans, T.np, sb, T.comb_chain,
                      tail_ok));
    if (!tail_ok) {
        bail_joined();
        return DBSP_OK;
    }
    hook_mark(HK_TAIL);
    TRY(q3_read_tail(c, back, sb));
    // tail barrier: the commit's output-length and plan-total reads (host
    // LH_* slots) wait this event just before consuming them, and it is
    // what a join on demand (q3_join_back) waits for
    (void)hipEventRecord(c->ev_tail[evi], back);
    if (fork) c->back_live = evi;
    hook_mark(HK_JOIN);
    T.arena_base = c->arena_base;
    T.arena_off = c->arena_off;
    c->arena_base = save_base;
    c->arena_off = save_off;
    T.pending = true;
    T.ev = d_ev;
    T.n = n;
    T.sb = sb;
    T.evi = evi;
    T.next_sb = sb == LEN_BASE0 ? LEN_BASE1 : LEN_BASE0;
    T.next_evi = evi ^ 1;
    return DBSP_OK;
}

static void q3_maybe_enqueue_train(dbsp_engine *e) {
    dbsp_ctx *c = e->ctx;
    static const bool train_on = []() {
        const char *v = getenv("DBSP_Q3_TRAIN");
        return !(v && v[0] == '0');
    }();
    if (!train_on || sharding_on(c) || e->train.pending || !e->next_ev ||
        e->next_n <= 0 || e->next_n > 131072 || e->spec_fail >= 3)
        return;
    (void)q3_enqueue_train(e, e->next_ev, e->next_n);
}

// commit a pipelined train: wait its event, read verdicts, insert, publish
static dbsp_status q3_commit_train(dbsp_engine *e) {
    const bool prof = g_hook_prof;
    static int prof_n = 0;
    double t0 = prof ? host_us() : 0;
    dbsp_ctx *c = e->ctx;
    Q3Train T = e->train;
    e->train.pending = false;  // T owns the batches now
    e->train.oA = e->train.oP = DevBatch{};
    e->train.res[0] = e->train.res[1] = DevBatch{};
    // arena rule: commit-side transients continue behind the train's own in
    // the train's half; the next train (hook below) takes the other half
    c->arena_base = T.arena_base;
    c->arena_off = T.arena_off;
    (void)hipEventSynchronize(c->ev_tick[T.evi]);
    double t1 = prof ? host_us() : 0;
    int64_t H[LEN_TICK];  // the train's head readback (later ones reuse h_len)
    memcpy(H, c->h_len + T.sb, sizeof(H));
    if (q3_spec_lost(H)) {
        e->spec_fail++;
        // the probe and the tail of this train bailed on the sentinel but
        // may not have run yet: they read the deltas dropped here and write
        // out_store and base-0 length slots that the replay reuses
        q3_join_back(c);
        q3_train_drop(c, T);
        // re-materialize the deltas from the raw flatmap outputs (arena of
        // the train's half, below what this commit bumps) and replay the
        // tick explicitly
        // The train's sorts took the counters, so the raw lengths are at
        // L_RAWN (L_RAW with DBSP_Q3_TAKE=0).  A count above the tick's
        // event count cannot come from a flatmap that started at zero (the
        // flatmap stored no row past the capacity either): refuse to sort
        // it.
        DevBatch dA, dP;
        const int l_raw = c->q3_take ? L_RAWN : L_RAW;
        T.rawA.n = H[l_raw];
        T.rawP.n = H[l_raw + 1];
        if (T.rawA.n < 0 || T.rawA.n > T.n || T.rawP.n < 0 || T.rawP.n > T.n)
            return DBSP_ERR_INTERNAL;
        TRY(sort_consolidate_batch(c, T.rawA, dA));
        TRY(sort_consolidate_batch(c, T.rawP, dP));
        return q3_body(e, T.ev, T.n, dA, dP, DevBatch{}, DevBatch{},
                       DevBatch{}, DevBatch{}, false, false);
    }
    e->spec_fail = 0;
    DevBatch dA = T.oA, dP = T.oP;
    dA.n = H[L_DELTA];
    dP.n = H[L_DELTA + 1];
    for (int i = 0; i < T.np; i++)
        if (T.plans[i].dd) T.plans[i].t.n[0] = dP.n;
    engine_free_output(e);
    double t2 = prof ? host_us() : 0;
    // --- accumulator swap (the spine insert ran inside the train) ---
    // The in-train merge produced res[s] = acc[s] ⋈ delta[s]; here we only
    // swap pointers: pop the consumed accumulator, publish the result, and
    // past the spill threshold seal it into the ladder.  No kernel launch
    // on the common path, so the next train (hook below) starts within a
    // few microseconds of the wake.
    // a deferred round's resolve frees the pre-cascade batches this train's
    // probe reads, and its cascade rounds borrow LEN_OP slots: join first
    if (c->pend_n) q3_join_back(c);
    TRY(resolve_pending_insert(c));
    constexpr int64_t Q3_ACC_SPILL = 32768;
    Spine *spill[2];
    int nspill = 0;
    DevBatch consumed[2];
    for (int s = 0; s < 2; s++) {
        Spine &sp = s == 0 ? e->a_int : e->p_int;
        DevBatch res = T.res[s];
        res.n = H[L_XCHG + s];  // the in-train accumulator merge's length
        DevBatch acc = e->q3_acc[s];
        if (acc.n > 0) {  // the top batch is the consumed accumulator
            sp.batches.pop_back();
            // this tick's plans probed it: an overflow replay at the publish
            // below still reads it, so it is freed after that
            consumed[s] = acc;
        }
        e->q3_acc[s] = DevBatch{};
        if (res.n > 0) {
            sp.batches.push_back(res);
            if (res.n > Q3_ACC_SPILL) {
                spill[nspill++] = &sp;
            } else {
                e->q3_acc[s] = res;
            }
        } else {
            free_batch(c, res);
        }
    }
    double th0 = 0, th1 = 0;
    bool fired = false;
    std::function<dbsp_status()> hook = [&]() -> dbsp_status {
        th0 = prof ? host_us() : 0;
        q3_maybe_enqueue_train(e);
        th1 = prof ? host_us() : 0;
        return DBSP_OK;
    };
    if (nspill > 0) {
        // sealed batches re-level through the classic rounds; the readback
        // is deferred (stash) so nothing blocks behind the new train.  A
        // pair past the batched merges' size is merged and freed at once,
        // under this train's probe: join first (spill ticks only)
        q3_join_back(c);
        TRY(spine_rounds(c, spill, nspill, &hook, &fired, /*defer=*/true));
    }
    if (!fired) TRY(hook());
    double t3 = prof ? host_us() : 0;
    if (prof && ++prof_n % 50 == 0)
        fprintf(stderr,
                "[commit] wait %.1f verdict %.1f swap+hook(total %.1f, hook %.1f) us\n"
                "[hook] flatmap %.1f sort %.1f alloc %.1f fork %.1f merge %.1f "
                "head %.1f probe %.1f tail %.1f join %.1f us\n",
                t1 - t0, t2 - t1, t3 - t2, th1 - th0, g_hook_us[HK_FLATMAP],
                g_hook_us[HK_SORT], g_hook_us[HK_ALLOC], g_hook_us[HK_FORK],
                g_hook_us[HK_MERGE], g_hook_us[HK_HEAD], g_hook_us[HK_PROBE],
                g_hook_us[HK_TAIL], g_hook_us[HK_JOIN]);
    // this tick's plan totals and output lengths land with the tail
    // readback, past ev_tick — wait the tail before consuming them
    (void)hipEventSynchronize(c->ev_tail[T.evi]);
    if (c->back_live == T.evi) c->back_live = -1;  // no train behind it
    TRY(q3_publish_chained(e, T.sb, dA, dP, T.plans, T.np, T.comb_chain));
    free_batch(c, consumed[0]);
    free_batch(c, consumed[1]);
    // the deltas were folded into res by the in-train merge (they are NOT
    // in the spine); free once the output paths above are done with them
    free_batch(c, dA);
    free_batch(c, dP);
    return DBSP_OK;
}

static dbsp_status q3_step(dbsp_engine *e, const dbsp_event *d_ev, int64_t n) {
    dbsp_ctx *c = e->ctx;
    if (e->train.pending) {
        if (e->train.ev == d_ev && e->train.n == n) return q3_commit_train(e);
        // stale train (out-of-band step): drain its enqueued work on both
        // streams, discard
        (void)hipStreamSynchronize(c->stream);
        q3_sync_back(c);
        q3_train_drop(c, e->train);
        e->train.pending = false;
    }
    const bool shard_chain =
        sharding_on(c) && c->world <= 8 && n <= 131072 && e->spec_fail < 3;
    const bool chain =
        shard_chain || (!sharding_on(c) && n <= 131072 && e->spec_fail < 3);
    DevBatch dA, dP, rawA, rawP, recvA, recvP;
    if (shard_chain) {
        TRY(build_deltas_chain_sharded(e, d_ev, n, rawA, rawP, recvA, recvP,
                                       dA, dP));
    } else if (chain) {
        TRY(build_deltas_chain(e, d_ev, n, rawA, rawP, dA, dP));
    } else {
        TRY(build_deltas(e, d_ev, n, dA, dP, true));
    }
    return q3_body(e, d_ev, n, dA, dP, rawA, rawP, recvA, recvP, chain,
                   shard_chain);
}

// ---- q5 / q8: pipelined front half, device watermark ----

// Take the pipelined front (launched during the previous tick's tail): true
// if it was built for exactly this tick.  A stale one (out-of-band step) is
// discarded; q5 fronts hold only arena transients, so only q8's sorted
// outputs need freeing.
static bool take_front(dbsp_engine *e, const dbsp_event *d_ev, int64_t n) {
    if (!e->front.pending) return false;
    e->front.pending = false;
    if (e->front.ev == d_ev && e->front.n == n) return true;
    free_batch(e->ctx, e->front.oA);
    free_batch(e->ctx, e->front.oB);
    return false;
}

// Run `build` — the launches of the NEXT tick's front half, filling
// e->front's batches — in the arena half this tick is not using, and mark
// the front pending for (next_ev, next_n) if it queued cleanly.  Called from
// the tail insert's hook, so the launches overlap this tick's host-side tail.
template <class Build>
static dbsp_status enqueue_front(dbsp_engine *e, Build build) {
    dbsp_ctx *c = e->ctx;
    const size_t save_base = c->arena_base, save_off = c->arena_off;
    arena_other_half(c, save_base);
    const dbsp_status st = build();
    e->front.arena_base = c->arena_base;
    e->front.arena_off = c->arena_off;
    c->arena_base = save_base;
    c->arena_off = save_off;
    if (st == DBSP_OK) {
        e->front.pending = true;
        e->front.ev = e->next_ev;
        e->front.n = e->next_n;
    }
    return st;
}

// readback (with sync) of the bounds the device watermark published
// {s0, e0, s1, e1, have_prev, err}
static dbsp_status read_bounds(dbsp_engine *e) {
    HIP_CHECK_ST(hipMemcpyAsync(e->h_bounds, e->d_bounds, 6 * sizeof(uint64_t),
                                hipMemcpyDeviceToHost, e->ctx->stream));
    HIP_CHECK_ST(hipStreamSynchronize(e->ctx->stream));
    return DBSP_OK;
}

// The tick's one watermark update (q5.rs:85-90 / q8.rs:63-65): the max event
// time is the last key of the time-keyed delta d, whose length is d.n or, when
// n_dev is given, still on the device.  Sharded ranks (host lengths only)
// reduce it across ranks ON THE STREAM first, an RCCL allreduce feeding the
// same kernel, so every mode advances the same state words in e->d_wm and
// flipping between them never desyncs the watermark.
static dbsp_status wm_update(dbsp_engine *e, const DevBatch &d,
                             const int64_t *n_dev, uint64_t width,
                             uint64_t tumble, uint64_t lag) {
    dbsp_ctx *c = e->ctx;
    WmSource src{d.k, d.n, n_dev, nullptr};
    if (sharding_on(c)) {
        unsigned long long *gslot = e->d_wm + 10;
        if (d.n > 0) {
            HIP_CHECK_ST(hipMemcpyAsync(gslot, d.k + d.n - 1, sizeof(uint64_t),
                                        hipMemcpyDeviceToDevice, c->stream));
        } else {
            HIP_CHECK_ST(hipMemsetAsync(gslot, 0, sizeof(uint64_t), c->stream));
        }
        if (ncclAllReduce(gslot, gslot, 1, ncclUint64, ncclMax, c->comm,
                          c->stream) != ncclSuccess)
            return DBSP_ERR_INTERNAL;
        src.gmax_dev = gslot;
    }
    return dbspk::wm_update(c->stream, src, width, tumble, lag, e->d_wm,
                            e->d_bounds);
}

// ---- q8 tick (queries/q8.rs:48-93) ----
static dbsp_status q8_step(dbsp_engine *e, const dbsp_event *d_ev, int64_t n) {
    dbsp_ctx *c = e->ctx;
    constexpr uint64_t TUMBLE_MS = 10000;
    const int64_t *H = c->h_len + LEN_BASE0;
    // Single-rank ticks chain flatmap -> sorts -> device watermark -> window
    // ranges with ONE sync; the watermark lives in e->d_wm so the bounds
    // never round-trip to the host.  Sharded ranks build their deltas
    // explicitly (the exchange needs host lengths) and run the same stage.
    const bool use_front = take_front(e, d_ev, n);
    const bool chain = use_front || (!sharding_on(c) && n <= 131072 &&
                                     e->spec_fail < 3);
    DevBatch dPT, dAT, rawP, rawA;
    WindowLeg legs[2] = {{&e->pt_int, &dPT, nullptr, L_WIN2},
                         {&e->at_int, &dAT, nullptr, L_WIN2 + 1}};
    if (chain) {
        if (use_front) {
            rawP = e->front.rawA;
            rawA = e->front.rawB;
            dPT = e->front.oA;
            dAT = e->front.oB;
        } else {
            TRY(build_deltas_chain(e, d_ev, n, rawP, rawA, dPT, dAT));
        }
        legs[0].n_dev = c->d_len + L_DELTA;
        legs[1].n_dev = c->d_len + L_DELTA + 1;
        TRY(wm_update(e, dAT, legs[1].n_dev, TUMBLE_MS, TUMBLE_MS, TUMBLE_MS));
        TRY(window_launch(e, legs, 2));
        TRY(read_len(c, LEN_BASE0, LEN_TICK, /*sync=*/false));
        TRY(read_bounds(e));
        const bool lost = e->h_bounds[5] != 0 || H[L_DELTA] < 0 ||
                          H[L_DELTA + 1] < 0 || H[L_WIN2] < 0 ||
                          H[L_WIN2 + 1] < 0;
        if (!lost) {
            dPT.n = H[L_DELTA];
            dAT.n = H[L_DELTA + 1];
            e->spec_fail = 0;
        } else {
            e->spec_fail++;
            // speculation lost (a delta overflowed the fused sort): re-sort
            // with the real lengths and launch the ranges again.  The
            // watermark stood still only if the auction delta was the one
            // that overflowed (err); otherwise its update has happened and
            // the published bounds are this tick's.
            rawP.n = H[L_RAW];
            rawA.n = H[L_RAW + 1];
            free_batch(c, dPT);
            free_batch(c, dAT);
            TRY(sort_consolidate_batch(c, rawP, dPT));
            TRY(sort_consolidate_batch(c, rawA, dAT));
            rawP = DevBatch{};
            rawA = DevBatch{};
            legs[0].n_dev = legs[1].n_dev = nullptr;
            if (e->h_bounds[5] != 0)
                TRY(wm_update(e, dAT, nullptr, TUMBLE_MS, TUMBLE_MS,
                              TUMBLE_MS));
            TRY(window_launch(e, legs, 2));
            TRY(read_len(c, L_WIN2, 2));
        }
    } else {
        TRY(build_deltas(e, d_ev, n, dPT, dAT, true));
        TRY(wm_update(e, dAT, nullptr, TUMBLE_MS, TUMBLE_MS, TUMBLE_MS));
        TRY(window_launch(e, legs, 2));
        TRY(read_len(c, LEN_BASE0, LEN_TICK));
    }
    std::vector<DevBatch> wp_raw, wa_raw;
    TRY(window_emit(c, legs[0], wp_raw));
    TRY(window_emit(c, legs[1], wa_raw));
    if (sharding_on(c)) {
        TRY(spines_insert_pair(c, e->pt_int, dPT, e->at_int, dAT));
    }  // single-rank: deferred into the tail multi-insert (the traces are
       // only read next tick, and one batched call saves a sync round)
    // map_index / map + consolidate
    DevBatch wpr, war, dWP, dWA;
    TRY(finalize_raw(c, wp_raw, wpr));
    TRY(finalize_raw(c, wa_raw, war));
    TRY(map_sorted(c, wpr, 0, dWP));
    TRY(map_sorted(c, war, 1, dWA));
    free_batch(c, wpr);
    free_batch(c, war);
    if (sharding_on(c)) {
        DevBatch t1, t2;
        TRY(shard_exchange_pair(c, dWP, dWA, t1, t2, 4 * n / 50 + 64,
                                12 * n / 50 + 64));
        dWP = t1;
        dWA = t2;
    }
    // bilinear expansion against PREVIOUS traces (as q3): joins independent
    // of the inserts, inserts paired into shared launches
    std::vector<DevBatch> outs;
    TRY(join_vs_spine(c, dWP, e->wa_int, DBSP_PROJ_HI_K_LO_V1RND, TUMBLE_MS, outs));
    TRY(join_vs_spine(c, dWA, e->wp_int, DBSP_PROJ_HI_K_LO_V2RND, TUMBLE_MS, outs));
    TRY(join_vs_batch(c, dWP, dWA, DBSP_PROJ_HI_K_LO_V1RND, TUMBLE_MS, outs));
    engine_free_output(e);
    // consolidate the joined output asynchronously (as q3): sort launched to
    // the reused store before the inserts, length read at their sync
    bool async_final = false;
    TRY(final_begin(e, outs, !sharding_on(c), async_final));
    if (!sharding_on(c)) {
        std::function<dbsp_status()> hook = [&]() -> dbsp_status {
            if (!e->next_ev || e->next_n < 0 || e->next_n > 131072 ||
                e->spec_fail >= 3)
                return DBSP_OK;
            return enqueue_front(e, [&] {
                return build_deltas_chain(e, e->next_ev, e->next_n,
                                          e->front.rawA, e->front.rawB,
                                          e->front.oA, e->front.oB);
            });
        };
        Spine *sps[4] = {&e->wp_int, &e->wa_int, &e->pt_int, &e->at_int};
        DevBatch bs[4] = {dWP, dWA, dPT, dAT};
        TRY(spines_insert_multi(c, sps, bs, 4, &hook));
    } else {
        TRY(spines_insert_pair(c, e->wp_int, dWP, e->wa_int, dWA));
    }
    return final_finish(e, outs, async_final);
}

// q5's front half: chained flatmap, then the min/max of the bid stream (the
// dense-sort probe) chained behind its device row counter into L_MINMAX
static dbsp_status q5_front(dbsp_engine *e, const dbsp_event *d_ev, int64_t n,
                            DevBatch &raw0, DevBatch &raw1) {
    dbsp_ctx *c = e->ctx;
    TRY(flatmap_chain(e, d_ev, n, raw0, raw1));
    // raw0.n is the capacity here; the length is still at d_len[L_RAW]
    return dbspk::minmax_rows_chain(
        c->stream, raw0, c->d_len + L_RAW,
        (unsigned long long *)(c->d_len + L_MINMAX));
}

// merge a delta (retained) into a consolidated single-batch integral
static dbsp_status integral_add(dbsp_ctx *c, DevBatch &integral,
                                const DevBatch &delta) {
    DevBatch m;
    TRY(merge_batches(c, integral, delta, m));
    free_batch(c, integral);
    integral = m;
    return DBSP_OK;
}

// ---- q5 tick (queries/q5.rs:77-121) ----
static dbsp_status q5_step(dbsp_engine *e, const dbsp_event *d_ev, int64_t n) {
    dbsp_ctx *c = e->ctx;
    constexpr uint64_t WIDTH_MS = 10000, TUMBLE_MS = 2000, WM_LAG_MS = 4000;
    const int64_t *H = c->h_len + LEN_BASE0;
    // Single-rank ticks: flatmap and the dense-range min/max probe chain into
    // ONE sync, the bid delta sorts through the dense path, and the
    // watermark/window-ranges run device-side as in q8.
    const bool chain = !sharding_on(c);
    DevBatch dBT;
    bool n_pending = false;  // dBT.n still on the device (L_DENSE)
    const bool use_front = take_front(e, d_ev, n);
    if (chain) {
        DevBatch raw0, raw1;
        if (use_front) {
            raw0 = e->front.rawA;
            raw1 = e->front.rawB;
        } else {
            TRY(q5_front(e, d_ev, n, raw0, raw1));
        }
        TRY(read_len(c, LEN_BASE0, LEN_TICK));
        free_batch(c, raw1);
        const int64_t n0 = H[L_RAW];
        raw0.n = n0;
        if (n0 == 0) {
            dBT = DevBatch{};
            free_batch(c, raw0);
        } else {
            const uint64_t *mm = (const uint64_t *)(H + L_MINMAX);
            const uint64_t kr = mm[2] - mm[0], vr = mm[3] - mm[1];
            const int64_t dense_cap =
                std::min<int64_t>((int64_t)1 << 22, 8 * n0);
            if (n0 > 8192 && kr < (uint64_t)dense_cap &&
                vr < (uint64_t)dense_cap &&
                (int64_t)((kr + 1) * (vr + 1)) <= dense_cap) {
                // chained: length stays on the device until the window sync
                ScopedTimer t(c, 0, (double)n0 * 48.0);
                DevBatch res;
                TRY(alloc_batch(c, n0, res));
                TRY(dbspk::sort_cons_dense_chain(
                    c->stream, raw0, mm[0], mm[1], (int64_t)(kr + 1),
                    (int64_t)(vr + 1), res, c->d_len + L_DENSE));
                free_batch(c, raw0);
                dBT = res;
                dBT.n = -1;
                n_pending = true;
            } else {
                TRY(sort_consolidate_batch(c, raw0, dBT));
            }
        }
    } else {
        // explicit deltas (sharded exchange)
        DevBatch dummy;
        TRY(build_deltas(e, d_ev, n, dBT, dummy, false));
    }
    // device watermark + chained window ranges (q5.rs:85-90)
    WindowLeg leg{&e->bt_int, &dBT, n_pending ? c->d_len + L_DENSE : nullptr,
                  L_WIN};
    TRY(wm_update(e, dBT, leg.n_dev, WIDTH_MS, TUMBLE_MS, WM_LAG_MS));
    TRY(window_launch(e, &leg, 1));
    TRY(read_len(c, LEN_BASE0, LEN_TICK));
    if (n_pending) dBT.n = H[L_DENSE];
    std::vector<DevBatch> wb_raw;
    TRY(window_emit(c, leg, wb_raw));
    if (sharding_on(c)) TRY(e->bt_int.insert(c, dBT));
    // single-rank: bt_int is only read next tick — inserted in the tail
    // multi-insert
    DevBatch wbr, dWB;
    TRY(finalize_raw(c, wb_raw, wbr));
    TRY(map_sorted(c, wbr, 1, dWB));  // (time,auction) -> (auction,()); weigh(|_|1)
    free_batch(c, wbr);
    if (sharding_on(c)) {
        DevBatch t1;
        TRY(shard_exchange(c, dWB, t1, 2 * n));
        dWB = t1;
    }
    // aggregate_linear: input trace includes this tick (trace.rs TraceAppend)
    TRY(e->wb_int.insert_copy(c, dWB));
    DevBatch dCounts;
    TRY(agg_linear_spine(c, dWB, e->wb_int, e->counts_int, dCounts));
    free_batch(c, dWB);
    // max side (tiny; consolidated single-batch traces)
    DevBatch dMaxIn;
    TRY(map_sorted(c, dCounts, 2, dMaxIn));
    if (sharding_on(c)) {
        DevBatch t1;
        TRY(shard_exchange(c, dMaxIn, t1, n / 8 + 64));  // unit key () on one rank
        dMaxIn = t1;
    }
    DevBatch dMaxOut;
    if (dMaxIn.n > 0) {
        TRY(integral_add(c, e->maxin_int, dMaxIn));
        free_batch(c, dMaxIn);
        // delta key is the unit key ()
        uint64_t *d_unit;
        HIP_CHECK_ST(dbspk::cache_malloc((void **)&d_unit, 8, c->stream));
        HIP_CHECK_ST(hipMemsetAsync(d_unit, 0, 8, c->stream));
        DevBatch raw;
        TRY(dbspk::agg_upsert_rows(c->stream, dbspk::AGG_MAX, d_unit, 1,
                                   e->maxin_int, e->maxout_int, &raw));
        HIP_CHECK_ST(dbspk::cache_free(d_unit, c->stream));
        TRY(sort_consolidate_batch(c, raw, dMaxOut));
        TRY(integral_add(c, e->maxout_int, dMaxOut));
    } else {
        free_batch(c, dMaxIn);
    }
    DevBatch dMaxZ, dBC;
    TRY(map_sorted(c, dMaxOut, 1, dMaxZ));  // ((),m) -> (m,())
    free_batch(c, dMaxOut);
    TRY(map_sorted(c, dCounts, 3, dBC));    // (auction,count) -> (count,auction)
    if (sharding_on(c)) {
        DevBatch t1, t2;
        TRY(shard_exchange_pair(c, dMaxZ, dBC, t1, t2, 64, n / 4 + 64));
        dMaxZ = t1;
        dBC = t2;
    }
    // final incremental join (q5.rs:118-120)
    std::vector<DevBatch> outs;
    TRY(join_vs_spine(c, dMaxZ, e->bc_int, DBSP_PROJ_HI_V2_LO_K, 0, outs));
    TRY(integral_add(c, e->maxz_int, dMaxZ));
    free_batch(c, dMaxZ);
    if (dBC.n > 0 && e->maxz_int.n > 0) {
        DevBatch o;
        TRY(dbspk::join_rows(c->stream, dBC, e->maxz_int, DBSP_PROJ_HI_V1_LO_K,
                             0, &o));
        if (o.n > 0) outs.push_back(o);
        else free_batch(c, o);
    }
    engine_free_output(e);
    bool async_final = false;
    TRY(final_begin(e, outs, !sharding_on(c), async_final));
    if (!sharding_on(c)) {
        std::function<dbsp_status()> hook = [&]() -> dbsp_status {
            if (!e->next_ev || e->next_n < 0) return DBSP_OK;
            return enqueue_front(e, [&] {
                e->front.oA = e->front.oB = DevBatch{};
                return q5_front(e, e->next_ev, e->next_n, e->front.rawA,
                                e->front.rawB);
            });
        };
        Spine *sps[3] = {&e->bc_int, &e->counts_int, &e->bt_int};
        DevBatch bs[3] = {dBC, dCounts, dBT};
        TRY(spines_insert_multi(c, sps, bs, 3, &hook));
    } else {
        TRY(e->bc_int.insert(c, dBC));
        TRY(e->counts_int.insert(c, dCounts));
    }
    return final_finish(e, outs, async_final);
}

// affected-key gather + keyed aggregate + upsert over a spine: the
// reference's eval_key discipline (aggregate/mod.rs:479-547) — gather the
// affected keys' value runs with a unit-weight key join (weights multiply by
// one, so the gather carries the trace weights), consolidate the slice (the
// aggregate needs per-val TOTAL weights), then run the MODE aggregate with
// upsert retractions against the consolidated output integral.
static dbsp_status agg_keyed_spine(dbsp_engine *e, const DevBatch &delta,
                                   Spine &in_sp, DevBatch &out_int, int mode,
                                   DevBatch &dOut) {
    dbsp_ctx *c = e->ctx;
    dOut = DevBatch{};
    if (delta.n == 0) return DBSP_OK;
    uint64_t *keys = nullptr;
    int64_t nk = 0;
    TRY(dbspk::unique_keys(c->stream, delta.k, delta.n, &keys, &nk));
    ScratchBuf keys_owner(c, keys);
    DevBatch kb;
    TRY(alloc_batch(c, nk, kb, true));
    HIP_CHECK_ST(hipMemcpyAsync(kb.k, keys, nk * 8, hipMemcpyDeviceToDevice,
                                c->stream));
    HIP_CHECK_ST(hipMemsetAsync(kb.v, 0, nk * 8, c->stream));
    dbspk::fill_u64(c->stream, (uint64_t *)kb.w, 1, nk);
    kb.n = nk;
    std::vector<DevBatch> gouts;
    TRY(join_vs_spine(c, kb, in_sp, DBSP_PROJ_HI_K_LO_V2, 0, gouts));
    DevBatch gathered;
    TRY(finalize_raw(c, gouts, gathered));
    DevBatch raw;
    {
        ScopedTimer timer(c, 3, 0.0);
        TRY(dbspk::agg_upsert_rows(
            c->stream, mode == 1 ? dbspk::AGG_MAX : dbspk::AGG_LAST10, keys,
            nk, gathered, out_int, &raw));
    }
    free_batch(c, gathered);
    keys_owner.reset();
    TRY(sort_consolidate_batch(c, raw, dOut));
    if (dOut.n > 0) {
        DevBatch cpy, m;
        TRY(copy_batch(c, dOut, cpy));
        TRY(merge_batches(c, out_int, cpy, m));
        free_batch(c, out_int);
        free_batch(c, cpy);
        out_int = m;
    }
    return DBSP_OK;
}

// the front q4 and q6 share: the tick's deltas, the winning-bid join under
// the query's projection pair, and Max per auction with upsert retractions
static dbsp_status winning_bids_front(dbsp_engine *e, int proj_bid_x_auc,
                                      int proj_auc_x_bid,
                                      const dbsp_event *d_ev, int64_t n,
                                      DevBatch &dA, DevBatch &dB,
                                      DevBatch &dWin) {
    dbsp_ctx *c = e->ctx;
    WinningBids &wb = e->win;
    engine_free_output(e);
    // auction / bid deltas, keyed by auction id
    TRY(build_deltas(e, d_ev, n, dA, dB, true));
    // bilinear expansion against PREVIOUS traces:
    //   dB ⋈ A_prev + dA ⋈ B_prev + dA ⋈ dB   (join.rs:217-292)
    std::vector<DevBatch> outs;
    TRY(join_vs_spine(c, dB, wb.a_int, proj_bid_x_auc, 0, outs));
    TRY(join_vs_spine(c, dA, wb.b_int, proj_auc_x_bid, 0, outs));
    TRY(join_vs_batch(c, dA, dB, proj_auc_x_bid, 0, outs));
    DevBatch dWinIn;
    TRY(finalize_raw(c, outs, dWinIn));
    dWin = DevBatch{};
    if (dWinIn.n > 0) {
        // max input lives in a SPINE (amortized log maintenance); the Max
        // aggregator re-reads only the AFFECTED keys' value runs each tick
        TRY(wb.maxin_sp.insert_copy(c, dWinIn));
        TRY(agg_keyed_spine(e, dWinIn, wb.maxin_sp, wb.maxout, 1, dWin));
    }
    free_batch(c, dWinIn);
    return DBSP_OK;
}

// the shared tail: TraceAppend both input deltas
static dbsp_status winning_bids_tail(dbsp_engine *e, DevBatch dA, DevBatch dB) {
    dbsp_ctx *c = e->ctx;
    TRY(e->win.a_int.insert(c, dA));
    TRY(e->win.b_int.insert(c, dB));
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    return DBSP_OK;
}

// ---------------------------------------------------------------------------
// q4 (queries/q4.rs): average winning-bid price per category.
//   auctions ⋈ bids on auction id with the bid-validity window applied in
//   the join_func (q4.rs:58-68; filtered pairs emit weight 0) →
//   Max per (auction, category) over the consolidated integral
//   (aggregate(Max), max.rs:36-55) with upsert retractions →
//   Average per category as ONE linear aggregate over the packed value
//   (sum<<20)+count (price < 2^20, per-category count < 2^20, so the packed
//   i64 weight sum is exact), divided at the output map (average.rs).
// Explicit per-op path (no chained speculation yet — q4 is not a headline
// config; correctness and coverage first).
// ---------------------------------------------------------------------------

static dbsp_status q4_step(dbsp_engine *e, const dbsp_event *d_ev, int64_t n) {
    dbsp_ctx *c = e->ctx;
    DevBatch dA, dB, dWin;
    TRY(winning_bids_front(e, DBSP_PROJ_Q4_BID_X_AUC, DBSP_PROJ_Q4_AUC_X_BID,
                           d_ev, n, dA, dB, dWin));
    // average per category: weigh into the packed (sum<<20)+count weight,
    // aggregate linearly over the integral spine, upsert, divide at output
    if (dWin.n > 0) {
        DevBatch wraw, dAvgIn;
        TRY(alloc_batch(c, dWin.n, wraw, true));
        TRY(dbspk::map_rows(c->stream, dWin, 5, wraw));
        TRY(sort_consolidate_batch(c, wraw, dAvgIn));
        free_batch(c, dWin);
        if (dAvgIn.n > 0) {
            TRY(e->q4_avg_int.insert_copy(c, dAvgIn));
            DevBatch upd;
            TRY(agg_linear_spine(c, dAvgIn, e->q4_avg_int, e->q4_avgout,
                                 upd));
            free_batch(c, dAvgIn);
            if (upd.n > 0) {
                TRY(e->q4_avgout.insert_copy(c, upd));
                // output: divide the packed sums (two packed values can map
                // to one average, so consolidate after the map)
                TRY(map_sorted(c, upd, 6, e->output));
            }
            free_batch(c, upd);
        }
    } else {
        free_batch(c, dWin);
    }
    return winning_bids_tail(e, dA, dB);
}

// ---------------------------------------------------------------------------
// q6 (queries/q6.rs): average winning-bid price of the last 10 closed
// auctions per seller.  Same join shape as q4 on (auction, seller), Max per
// (auction<<20|seller), then the VecDeque fold (q6.rs:96-110) as the MODE-2
// last-10 average over the seller-keyed integral whose vals
// (auction<<27)|price keep the reference's cursor order by auction id.
// ---------------------------------------------------------------------------

static dbsp_status q6_step(dbsp_engine *e, const dbsp_event *d_ev, int64_t n) {
    dbsp_ctx *c = e->ctx;
    DevBatch dA, dB, dWin;
    TRY(winning_bids_front(e, DBSP_PROJ_Q6_BID_X_AUC, DBSP_PROJ_Q6_AUC_X_BID,
                           d_ev, n, dA, dB, dWin));
    if (dWin.n > 0) {
        // map_index (q6.rs:92-94): key by seller, val (auction<<27)|price
        DevBatch fraw, dFoldIn;
        TRY(alloc_batch(c, dWin.n, fraw, true));
        TRY(dbspk::map_rows(c->stream, dWin, 7, fraw));
        TRY(sort_consolidate_batch(c, fraw, dFoldIn));
        free_batch(c, dWin);
        if (dFoldIn.n > 0) {
            TRY(e->q6_fold_sp.insert_copy(c, dFoldIn));
            TRY(agg_keyed_spine(e, dFoldIn, e->q6_fold_sp, e->q6_foldout, 2,
                                e->output));
        }
        free_batch(c, dFoldIn);
    } else {
        free_batch(c, dWin);
    }
    return winning_bids_tail(e, dA, dB);
}

// ---------------------------------------------------------------------------
// C5 (query 100): synthetic 1B-row OrdIndexedZSet x 10M-row delta incremental
// join with f64 sum aggregate (BASELINE configs[4]).  Per
// tick: delta ⋈ trace carrying the trace's f64 val (JoinTrace::eval,
// join.rs:732-863), weigh f(k,v)=f64(v) (aggregate/mod.rs:297-323),
// consolidate, fold into the f64-weighted integral spine, re-aggregate the
// affected keys with upsert retractions against the output trace
// (aggregate/mod.rs:479-547 + upsert.rs:161-208), then TraceAppend the delta
// into the join trace.  Both the trace and each tick's delta are generated
// ON DEVICE (no 24 GB host staging) by the counter-based splitmix64
// generator in kernels.hip (c5_gen_rows).
// ---------------------------------------------------------------------------

extern "C" dbsp_status dbsp_engine_c5_init(dbsp_engine *e, int64_t n_trace,
                                           int64_t n_delta, uint64_t seed) {
    if (!e || e->query != 100 || n_trace <= 0 || n_delta <= 0)
        return DBSP_ERR_INVALID;
    dbsp_ctx *c = e->ctx;
    // trace-scale workload: keep tick-scale buffers on the stream-ordered
    // pool so it can serve the per-tick multi-GB spine carves from retained
    // slabs (see cache_small_set)
    dbspk::cache_small_set(false, c->stream);
    e->c5_trace.clear(c);
    e->c5_wint.clear(c);
    e->c5_out.clear(c);
    e->c5_wint.wf64 = true;
    DevBatch tr;
    TRY(alloc_batch(c, n_trace, tr));
    // trace keys 5i + h%4 (sorted unique, ~0.8 keys/int density), f64 vals
    TRY(dbspk::c5_gen_rows(c->stream, tr, 5, 4, seed, 0));
    TRY(e->c5_trace.insert(c, tr));
    e->c5_n_delta = n_delta;
    e->c5_seed = seed;
    // delta keys span the same range as the trace's (5*n_trace)
    uint64_t stride = (uint64_t)((5 * n_trace) / n_delta);
    if (stride < 3) stride = 3;
    e->c5_delta_stride = stride;
    e->n_events = INT64_MAX;  // step ranges are delta-row ids, not events
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    return DBSP_OK;
}

static dbsp_status c5_step(dbsp_engine *e, int64_t lo, int64_t hi) {
    dbsp_ctx *c = e->ctx;
    engine_free_output(e);
    const int64_t nd = hi - lo;
    if (nd <= 0) return DBSP_OK;
    if (e->c5_n_delta <= 0) return DBSP_ERR_INVALID;  // c5_init not called
    const uint64_t tick = (uint64_t)(lo / e->c5_n_delta);
    // tick's delta: device-generated sorted-unique rows, v = 0, w = +1
    DevBatch delta;
    TRY(alloc_batch(c, nd, delta));
    TRY(dbspk::c5_gen_rows(c->stream, delta, e->c5_delta_stride,
                           e->c5_delta_stride - 1,
                           e->c5_seed + 0x9E3779B97F4A7C15ull * (tick + 1), 1));
    // 1. join vs the trace spine, carrying the trace-side f64 val
    std::vector<DevBatch> outs;
    TRY(join_vs_spine(c, delta, e->c5_trace, DBSP_PROJ_HI_K_LO_V2, 0, outs));
    // 2. weigh + consolidate into the tick's f64-weighted delta
    DevBatch dwb{};
    if (!outs.empty()) {
        DevBatch cat;
        TRY(concat_batches(c, outs, cat));
        for (auto &b : outs) free_batch(c, b);
        outs.clear();
        DevBatch weighed;
        TRY(alloc_batch(c, cat.n, weighed, true));
        {
            ScopedTimer t(c, 3, 0.0);
            TRY(dbspk::map_rows(c->stream, cat, 4, weighed));
        }
        free_batch(c, cat);
        dbsp_batch ob{};
        TRY(dbsp_sort_consolidate_f64(c, weighed.k, weighed.v,
                                      (const double *)weighed.w, weighed.n,
                                      &ob));
        free_batch(c, weighed);
        dwb = DevBatch{ob.k, ob.v, ob.w, ob.len};
    }
    // 3. aggregate the affected keys over the integral (including this
    // tick's weighted delta, which is inserted first) + upsert retractions
    DevBatch upd{};
    if (dwb.n > 0) {
        TRY(e->c5_wint.insert_copy(c, dwb));
        TRY(agg_linear_spine(c, dwb, e->c5_wint, e->c5_out, upd));
        free_batch(c, dwb);
    }
    // 4. output delta + TraceAppend on the output trace
    if (upd.n > 0) TRY(e->c5_out.insert_copy(c, upd));
    e->output = upd;
    e->output_is_store = false;
    // 5. TraceAppend the delta into the join trace
    TRY(e->c5_trace.insert(c, delta));
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    return DBSP_OK;
}

// query 19's tick, defined with its operator at the end of this file
static dbsp_status q19_step(dbsp_engine *e, const dbsp_event *d_ev,
                            int64_t n);
// query 103's tick, likewise
static dbsp_status q103_step(dbsp_engine *e, const dbsp_event *d_ev,
                             int64_t n);
// query 7's tick, likewise
static dbsp_status q7_step(dbsp_engine *e, const dbsp_event *d_ev, int64_t n);

extern "C" dbsp_status dbsp_engine_step_staged(dbsp_engine *e, int64_t lo,
                                               int64_t hi) {
    if (lo < 0 || hi > e->n_events || lo > hi) return DBSP_ERR_INVALID;
    {
        dbsp_ctx *cc = e->ctx;
        if (e->front.pending) {
            // continue in the half the pipelined front allocated from
            cc->arena_base = e->front.arena_base;
            cc->arena_off = e->front.arena_off;
        } else {
            cc->arena_base =
                cc->arena_half ? (cc->arena_base ? 0 : cc->arena_half) : 0;
            cc->arena_off = 0;
        }
    }
    if (e->query == 0) {
        q0_step_host(e, e->h_events.data() + lo, hi - lo);
        return DBSP_OK;
    }
    if (e->query == 100) return c5_step(e, lo, hi);
    const dbsp_event *d_ev = e->d_events + lo;
    switch (e->query) {
        case 3: return q3_step(e, d_ev, hi - lo);
        case 4: return q4_step(e, d_ev, hi - lo);
        case 6: return q6_step(e, d_ev, hi - lo);
        case 5: return q5_step(e, d_ev, hi - lo);
        case 8: return q8_step(e, d_ev, hi - lo);
        case 7: return q7_step(e, d_ev, hi - lo);
        case 19: return q19_step(e, d_ev, hi - lo);
        case 101:
        case 102: return q101_step(e, d_ev, hi - lo);
        case 103: return q103_step(e, d_ev, hi - lo);
    }
    return DBSP_ERR_INVALID;
}

extern "C" dbsp_status dbsp_engine_run_staged(dbsp_engine *e, int64_t lo,
                                              int64_t hi, int64_t tick) {
    // the benchmark hot loop: ticks run back-to-back inside one C call so the
    // per-tick host cost excludes the Python/ctypes round-trip
    if (tick <= 0) return DBSP_ERR_INVALID;
    for (int64_t t = lo; t < hi; t += tick) {
        const int64_t t_hi = std::min(hi, t + tick);
        const int64_t n_lo = t_hi, n_hi = std::min(hi, t_hi + tick);
        if (n_lo < hi && e->d_events) {
            e->next_ev = e->d_events + n_lo;
            e->next_n = n_hi - n_lo;
        } else {
            e->next_ev = nullptr;
            e->next_n = -1;
        }
        dbsp_status st = dbsp_engine_step_staged(e, t, t_hi);
        if (st != DBSP_OK) return st;
    }
    e->next_ev = nullptr;
    e->next_n = -1;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_engine_step(dbsp_engine *e, const dbsp_event *events,
                                        int64_t n) {
    if (e->query == 0) {
        q0_step_host(e, events, n);
        return DBSP_OK;
    }
    dbsp_ctx *c = e->ctx;
    c->arena_off = 0;
    dbsp_event *d_ev;
    HIP_CHECK_ST(dbspk::cache_malloc((void **)&d_ev, n * sizeof(dbsp_event) + 64, c->stream));
    HIP_CHECK_ST(hipMemcpyAsync(d_ev, events, n * sizeof(dbsp_event),
                                hipMemcpyHostToDevice, c->stream));
    dbsp_status st = DBSP_OK;
    switch (e->query) {
        case 3: st = q3_step(e, d_ev, n); break;
        case 4: st = q4_step(e, d_ev, n); break;
        case 6: st = q6_step(e, d_ev, n); break;
        case 5: st = q5_step(e, d_ev, n); break;
        case 8: st = q8_step(e, d_ev, n); break;
        case 7: st = q7_step(e, d_ev, n); break;
        case 19: st = q19_step(e, d_ev, n); break;
        case 101:
        case 102: st = q101_step(e, d_ev, n); break;
        case 103: st = q103_step(e, d_ev, n); break;
        default: st = DBSP_ERR_INVALID;
    }
    (void)dbspk::cache_free(d_ev, c->stream);
    return st;
}

extern "C" dbsp_status dbsp_engine_output(dbsp_engine *e, dbsp_row *out,
                                          int64_t cap, int64_t *n_out) {
    dbsp_ctx *c = e->ctx;
    *n_out = e->output.n;
    if (e->output.n > cap) return DBSP_ERR_OVERFLOW;
    if (e->output.n == 0) return DBSP_OK;
    std::vector<uint64_t> k(e->output.n), v(e->output.n);
    std::vector<int64_t> w(e->output.n);
    TRY(dbsp_d2h(c, k.data(), e->output.k, e->output.n * 8));
    TRY(dbsp_d2h(c, v.data(), e->output.v, e->output.n * 8));
    TRY(dbsp_d2h(c, w.data(), e->output.w, e->output.n * 8));
    for (int64_t i = 0; i < e->output.n; i++) out[i] = {k[i], v[i], w[i]};
    return DBSP_OK;
}

// q0's output is the consolidated event zset itself
extern "C" dbsp_status dbsp_engine_output_events(dbsp_engine *e, dbsp_event *out,
                                                 int64_t cap, int64_t *n_out) {
    *n_out = (int64_t)e->q0_output.size();
    if ((int64_t)e->q0_output.size() > cap) return DBSP_ERR_OVERFLOW;
    memcpy(out, e->q0_output.data(), e->q0_output.size() * sizeof(dbsp_event));
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_engine_kernel_stats(dbsp_engine *e, int kind,
                                                double *total_ms,
                                                double *algo_bytes,
                                                int64_t *launches) {
    if (kind < 0 || kind > 5) return DBSP_ERR_INVALID;
    *total_ms = e->ctx->stats[kind].ms;
    *algo_bytes = e->ctx->stats[kind].bytes;
    *launches = e->ctx->stats[kind].launches;
    return DBSP_OK;
}

// ---- incremental top-K per group (queries/q19.rs; fold.rs:83-92) ----
// Per tick, over a consolidated delta D:
//   classify  every row of D against in_sp BEFORE the tick: appear (absent ->
//             present), vanish (present -> absent) or neither; head flags
//             and one scan list the affected groups and their key ranges
//   current   out_sp rows inside those ranges, consolidated: Oc, at most K
//             rows per affected group, all of weight +1
//   verdict   a group refills iff one of its vanish rows r has
//             count(Oc_g) == K and r >= first(Oc_g): only a full top-K that
//             loses a member must look deeper.  A short Oc_g holds every
//             present row of its group, and a row below a full Oc_g's first
//             member was not in it.
//   insert    D into in_sp
//   slice     groups not refilled: Oc_g at +1, appear rows at +1, vanish rows
//             that are in Oc_g at -1; refilled groups: their whole run out of
//             in_sp with its real weights (rows_gathered), and none of Oc_g,
//             whose synthetic +1 would corrupt them.  Consolidated into S.
//   select    a row of S is kept iff at most K - 1 rows follow it in its group
//   output    consolidate(selected - Oc), appended to out_sp
// An append-only stream never refills: step cost follows the delta and K,
// not the group.  The explicit per-op path (a host length sync per phase, as
// q4/q6 and the rolling operator); no chaining.  No row is invalid, so
// nothing can fail after the first write to in_sp for a reason the caller
// controls.
dbsp_status TopKOp::step(dbsp_ctx *c, const DevBatch &delta, DevBatch &out) {
    out = DevBatch{};
    if (delta.n == 0) return DBSP_OK;
    ScopedTimer timer(c, 3, 0.0);
    const int64_t n = delta.n;
    TRY(in_sp.cap_batches(c));
    TRY(out_sp.cap_batches(c));
    uint64_t *pb = nullptr;
    int64_t ng = 0;
    TRY(dbspk::topk_classify(c->stream, delta, trace_args_of(in_sp),
                             group_shift, &pb, &ng));
    ScratchBuf plan(c, pb);
    DevBatch cur;
    {
        DevBatch raw;
        TRY(dbspk::keyrange_gather(c->stream, pb + 2 * n, pb + 3 * n, ng,
                                   trace_args_of(out_sp), 1, &raw));
        TRY(sort_consolidate_batch(c, raw, cur));
    }
    uint64_t *vb = nullptr;
    int64_t n_refill = 0;
    TRY(dbspk::topk_verdict(c->stream, delta, pb, ng, cur, K, refill_all, &vb,
                            &n_refill));
    ScratchBuf verdict(c, vb);
    TRY(in_sp.insert_copy(c, delta));
    TRY(in_sp.cap_batches(c));
    // the candidate slice
    std::vector<DevBatch> parts;
    int64_t gathered = 0;
    {
        DevBatch cand;
        TRY(dbspk::topk_candidates(c->stream, delta, pb, ng, vb, cur, &cand));
        if (cand.n > 0) parts.push_back(cand);
    }
    if (n_refill > 0) {
        DevBatch runs;
        TRY(dbspk::keyrange_gather(c->stream, vb + ng, vb + 2 * ng, n_refill,
                                   trace_args_of(in_sp), 1, &runs));
        gathered = runs.n;
        if (runs.n > 0) parts.push_back(runs);
    }
    DevBatch slice, sel;
    if (!parts.empty()) TRY(finalize_raw(c, parts, slice));
    TRY(dbspk::topk_select(c->stream, slice, K, group_shift, &sel));
    const int64_t moved = cur.n + gathered + slice.n + sel.n;
    free_batch(c, slice);
    // selected - Oc: Oc's weights are all +1, so -1 throughout negates it
    if (cur.n > 0) dbspk::fill_u64(c->stream, (uint64_t *)cur.w, ~0ull, cur.n);
    if (cur.n == 0) {
        out = sel;
    } else if (sel.n == 0) {
        out = cur;
    } else {
        TRY(merge_batches(c, sel, cur, out));
        free_batch(c, sel);
        free_batch(c, cur);
    }
    if (out.n == 0) free_batch(c, out);
    if (out.n > 0) TRY(out_sp.insert_copy(c, out));
    groups_seen += ng;
    groups_refilled += n_refill;
    rows_gathered += gathered;
    timer.bytes = 24.0 * (double)moved;
    return DBSP_OK;
}

struct dbsp_topk_op {
    dbsp_ctx *ctx = nullptr;
    TopKOp op;
};

static bool topk_args_valid(int64_t K, int group_shift) {
    return K >= 1 && K <= 65536 && group_shift >= 0 && group_shift <= 63;
}

// the select stage over a caller's batch: the recompute route
extern "C" dbsp_status dbsp_topk(dbsp_ctx *c, const dbsp_batch *in, int64_t K,
                                 int group_shift, dbsp_batch *out) {
    if (!c || !in || !out || in->len < 0 || !topk_args_valid(K, group_shift))
        return DBSP_ERR_INVALID;
    DevBatch res;
    {
        ScopedTimer t(c, 3, 0.0);
        TRY(dbspk::topk_select(c->stream, as_batch(in), K, group_shift, &res));
    }
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_topk_create(dbsp_ctx *c, int64_t K,
                                        int group_shift, uint32_t flags,
                                        dbsp_topk_op **out) {
    if (!c || !out || !topk_args_valid(K, group_shift) ||
        (flags & ~(uint32_t)DBSP_TOPK_REFILL_ALL))
        return DBSP_ERR_INVALID;
    dbsp_topk_op *t = new dbsp_topk_op();
    t->ctx = c;
    t->op.K = K;
    t->op.group_shift = group_shift;
    t->op.refill_all = (flags & DBSP_TOPK_REFILL_ALL) != 0;
    *out = t;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_topk_step(dbsp_topk_op *t, const uint64_t *k,
                                      const uint64_t *v, const int64_t *w,
                                      int64_t n, dbsp_batch *out) {
    if (!t || !out || n < 0) return DBSP_ERR_INVALID;
    dbsp_ctx *c = t->ctx;
    *out = dbsp_batch{nullptr, nullptr, nullptr, 0};
    if (n == 0) return DBSP_OK;
    DevBatch raw, delta, res;
    TRY(alloc_batch(c, n, raw));
    TRY(copy_cols(c, raw, 0, k, v, w, n));
    TRY(sort_consolidate_batch(c, raw, delta));
    const dbsp_status st = t->op.step(c, delta, res);
    free_batch(c, delta);
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    if (st != DBSP_OK) return st;
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_topk_stats(dbsp_topk_op *t, int64_t *in_rows,
                                       int *in_batches, int64_t *out_rows,
                                       int *out_batches, int64_t *groups_seen,
                                       int64_t *groups_refilled,
                                       int64_t *rows_gathered) {
    if (!t) return DBSP_ERR_INVALID;
    if (in_rows) *in_rows = t->op.in_sp.total();
    if (in_batches) *in_batches = (int)t->op.in_sp.batches.size();
    if (out_rows) *out_rows = t->op.out_sp.total();
    if (out_batches) *out_batches = (int)t->op.out_sp.batches.size();
    if (groups_seen) *groups_seen = t->op.groups_seen;
    if (groups_refilled) *groups_refilled = t->op.groups_refilled;
    if (rows_gathered) *rows_gathered = t->op.rows_gathered;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_topk_destroy(dbsp_topk_op *t) {
    if (!t) return DBSP_OK;
    t->op.clear(t->ctx);
    (void)hipStreamSynchronize(t->ctx->stream);
    delete t;
    return DBSP_OK;
}

// ---- query 19: the top K bids of every auction (queries/q19.rs) ----
// bids.flat_map_index(|b| (b.auction, (b.price, b))) into the top-K operator:
// rows k = auction << 27 | price, v = bidder << 32 | date_time with
// group_shift 27, so the group is the auction and the order inside it
// (price, bidder, date_time): the reference's (price, Bid) order restricted
// to the fields dbsp_event carries (channel, url and extra are not in the
// event row).  The output rows are the input rows.
// A field too wide for its place is caught on the device: the flatmap sends
// such a bid to its second stream, whose length build_deltas reads back with
// the other lengths; a non-empty second stream makes the step
// DBSP_ERR_INVALID before the operator runs, so its state is unchanged.
static dbsp_status q19_step(dbsp_engine *e, const dbsp_event *d_ev,
                            int64_t n) {
    dbsp_ctx *c = e->ctx;
    engine_free_output(e);
    e->topk_stepped = true;
    DevBatch d, dummy;
    int64_t n_wide = 0;
    TRY(build_deltas(e, d_ev, n, d, dummy, false, &n_wide));
    dbsp_status st = DBSP_ERR_INVALID;
    if (n_wide == 0) st = e->topk.step(c, d, e->output);
    free_batch(c, d);
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    return st;
}

extern "C" dbsp_status dbsp_engine_topk_init(dbsp_engine *e, int64_t K) {
    if (!e || e->query != 19 || e->topk_stepped || !topk_args_valid(K, 27))
        return DBSP_ERR_INVALID;
    e->topk.K = K;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_engine_topk_stats(dbsp_engine *e, int64_t *in_rows,
                                              int64_t *out_rows,
                                              int64_t *groups_seen,
                                              int64_t *groups_refilled,
                                              int64_t *rows_gathered) {
    if (!e || e->query != 19) return DBSP_ERR_INVALID;
    if (in_rows) *in_rows = e->topk.in_sp.total();
    if (out_rows) *out_rows = e->topk.out_sp.total();
    if (groups_seen) *groups_seen = e->topk.groups_seen;
    if (groups_refilled) *groups_refilled = e->topk.groups_refilled;
    if (rows_gathered) *rows_gathered = e->topk.rows_gathered;
    return DBSP_OK;
}

// ---- incremental antijoin / semijoin (Stream::antijoin, join.rs:294-320) ----
//   d(A |> B) = dA * [k not in B'] + A * ([k not in B'] - [k not in B])
// with A, B the integrals before the tick and B' the key set after it.  Per
// tick, over consolidated DA and DB:
//   flip     every key of DB against b_sp BEFORE the tick:
//            flip = [before + dw > 0] - [before > 0]; the flipped keys are
//            compacted with their multiplier (-flip antijoin, +flip semijoin)
//   gather   the flipped keys' runs out of a_sp, BEFORE DA goes in, weights
//            times the multiplier, consolidated: G.  No flip, no gather.
//   insert   DB into b_sp
//   filter   a row of DA is kept iff (antijoin) != (its key present in b_sp
//            now): F, rows_filtered counts the rest
//   insert   DA into a_sp
//   output   consolidate(F ++ G): both are consolidated, so one merge
// Nothing else of either trace is read: step cost follows the delta and the
// flipped keys' runs.  The explicit per-op path (a host length sync per
// phase, as q4/q6, the rolling operator and top-K); no chaining.  No row and
// no key is invalid, so nothing can fail after the first write to a spine
// for a reason the caller controls.
dbsp_status AntiJoinOp::step(dbsp_ctx *c, const DevBatch &da,
                             const DevBatch &db, DevBatch &out) {
    out = DevBatch{};
    if (da.n == 0 && db.n == 0) return DBSP_OK;
    ScopedTimer timer(c, 3, 0.0);
    TRY(a_sp.cap_batches(c));
    TRY(b_sp.cap_batches(c));
    DevBatch G, F;
    int64_t n_flip = 0, copied = 0;
    if (db.n > 0) {
        uint64_t *pb = nullptr;
        TRY(dbspk::anti_flip(c->stream, db, trace_args_of(b_sp), anti, &pb,
                             &n_flip));
        ScratchBuf plan(c, pb);
        if (n_flip > 0) {
            DevBatch raw;
            TRY(dbspk::keyrange_gather_mul(c->stream, pb,
                                           (const int64_t *)(pb + n_flip),
                                           n_flip, trace_args_of(a_sp), &raw));
            copied = raw.n;
            // a key's runs of several batches follow one another: sort them
            TRY(sort_consolidate_batch(c, raw, G));
        }
        TRY(b_sp.insert_copy(c, db));
        TRY(b_sp.cap_batches(c));
    }
    if (da.n > 0) {
        TRY(dbspk::anti_filter(c->stream, da, trace_args_of(b_sp), anti, &F));
        TRY(a_sp.insert_copy(c, da));
    }
    const int64_t moved = db.n + da.n + 2 * copied + F.n;
    keys_flipped += n_flip;
    rows_gathered += G.n;
    rows_filtered += da.n - F.n;
    if (G.n == 0) {
        free_batch(c, G);
        out = F;
    } else if (F.n == 0) {
        out = G;
    } else {
        TRY(merge_batches(c, F, G, out));
        free_batch(c, F);
        free_batch(c, G);
    }
    if (out.n == 0) free_batch(c, out);
    timer.bytes = 24.0 * (double)moved;
    return DBSP_OK;
}

struct dbsp_antijoin_op {
    dbsp_ctx *ctx = nullptr;
    AntiJoinOp op;
};

static bool antijoin_mode_valid(int mode) {
    return mode == DBSP_ANTIJOIN || mode == DBSP_SEMIJOIN;
}

// raw keys (k, w) as consolidated key rows (k, 0, w)
static dbsp_status key_rows(dbsp_ctx *c, const uint64_t *bk, const int64_t *bw,
                            int64_t nb, DevBatch &out) {
    out = DevBatch{};
    if (nb == 0) return DBSP_OK;
    DevBatch raw;
    TRY(alloc_batch(c, nb, raw));
    HIP_CHECK_ST(hipMemcpyAsync(raw.k, bk, nb * 8, hipMemcpyDeviceToDevice,
                                c->stream));
    HIP_CHECK_ST(hipMemsetAsync(raw.v, 0, nb * 8, c->stream));
    HIP_CHECK_ST(hipMemcpyAsync(raw.w, bw, nb * 8, hipMemcpyDeviceToDevice,
                                c->stream));
    return sort_consolidate_batch(c, raw, out);
}

// the filter alone over a caller's batch and key set: the recompute route
extern "C" dbsp_status dbsp_antijoin(dbsp_ctx *c, const dbsp_batch *a,
                                     const uint64_t *bk, const int64_t *bw,
                                     int64_t nb, int mode, dbsp_batch *out) {
    if (!c || !a || !out || a->len < 0 || nb < 0 || !antijoin_mode_valid(mode))
        return DBSP_ERR_INVALID;
    TraceArgs t{};
    if (nb > 0)
        trace_push(t, DevBatch{(uint64_t *)bk, (uint64_t *)bk, (int64_t *)bw,
                               nb});
    DevBatch res;
    {
        ScopedTimer timer(c, 3, 0.0);
        TRY(dbspk::anti_filter(c->stream, as_batch(a), t,
                               mode == DBSP_ANTIJOIN, &res));
        timer.bytes = 24.0 * (double)(a->len + nb + res.n);
    }
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_antijoin_create(dbsp_ctx *c, int mode,
                                            dbsp_antijoin_op **out) {
    if (!c || !out || !antijoin_mode_valid(mode)) return DBSP_ERR_INVALID;
    dbsp_antijoin_op *t = new dbsp_antijoin_op();
    t->ctx = c;
    t->op.anti = mode == DBSP_ANTIJOIN;
    *out = t;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_antijoin_step(dbsp_antijoin_op *t,
                                          const uint64_t *ak,
                                          const uint64_t *av,
                                          const int64_t *aw, int64_t na,
                                          const uint64_t *bk,
                                          const int64_t *bw, int64_t nb,
                                          dbsp_batch *out) {
    if (!t || !out || na < 0 || nb < 0) return DBSP_ERR_INVALID;
    dbsp_ctx *c = t->ctx;
    *out = dbsp_batch{nullptr, nullptr, nullptr, 0};
    if (na == 0 && nb == 0) return DBSP_OK;
    DevBatch da, db, res;
    if (na > 0) {
        DevBatch raw;
        TRY(alloc_batch(c, na, raw));
        TRY(copy_cols(c, raw, 0, ak, av, aw, na));
        TRY(sort_consolidate_batch(c, raw, da));
    }
    dbsp_status st = key_rows(c, bk, bw, nb, db);
    if (st == DBSP_OK) st = t->op.step(c, da, db, res);
    free_batch(c, da);
    free_batch(c, db);
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    if (st != DBSP_OK) return st;
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_antijoin_stats(dbsp_antijoin_op *t,
                                           int64_t *a_rows, int *a_batches,
                                           int64_t *b_rows, int *b_batches,
                                           int64_t *keys_flipped,
                                           int64_t *rows_gathered,
                                           int64_t *rows_filtered) {
    if (!t) return DBSP_ERR_INVALID;
    if (a_rows) *a_rows = t->op.a_sp.total();
    if (a_batches) *a_batches = (int)t->op.a_sp.batches.size();
    if (b_rows) *b_rows = t->op.b_sp.total();
    if (b_batches) *b_batches = (int)t->op.b_sp.batches.size();
    if (keys_flipped) *keys_flipped = t->op.keys_flipped;
    if (rows_gathered) *rows_gathered = t->op.rows_gathered;
    if (rows_filtered) *rows_filtered = t->op.rows_filtered;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_antijoin_destroy(dbsp_antijoin_op *t) {
    if (!t) return DBSP_OK;
    t->op.clear(t->ctx);
    (void)hipStreamSynchronize(t->ctx->stream);
    delete t;
    return DBSP_OK;
}

// ---- query 103: auctions nobody has bid on yet ----
// auctions.map_index(|a| (a.id, a.seller))
//     .antijoin(&bids.map_index(|b| (b.auction, ())))
// (Stream::antijoin, join.rs:294-320).  The flatmap's stream 0 carries the
// auctions as (id, seller, w), stream 1 the bids as key rows (auction, 0, w);
// the output rows are the auction rows, signed.
static dbsp_status q103_step(dbsp_engine *e, const dbsp_event *d_ev,
                             int64_t n) {
    dbsp_ctx *c = e->ctx;
    engine_free_output(e);
    DevBatch da, db;
    TRY(build_deltas(e, d_ev, n, da, db, true));
    const dbsp_status st = e->anti.step(c, da, db, e->output);
    free_batch(c, da);
    free_batch(c, db);
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    return st;
}

extern "C" dbsp_status dbsp_engine_antijoin_stats(dbsp_engine *e,
                                                  int64_t *a_rows,
                                                  int64_t *b_rows,
                                                  int64_t *keys_flipped,
                                                  int64_t *rows_gathered,
                                                  int64_t *rows_filtered) {
    if (!e || e->query != 103) return DBSP_ERR_INVALID;
    if (a_rows) *a_rows = e->anti.a_sp.total();
    if (b_rows) *b_rows = e->anti.b_sp.total();
    if (keys_flipped) *keys_flipped = e->anti.keys_flipped;
    if (rows_gathered) *rows_gathered = e->anti.rows_gathered;
    if (rows_filtered) *rows_filtered = e->anti.rows_filtered;
    return DBSP_OK;
}

// ---- incremental arg-max per group, ties kept (queries/q7.rs:82-93) ----
// Per tick, over a consolidated delta D:
//   classify  every row of D against in_sp BEFORE the tick (top-K's kernels):
//             appear, vanish or neither, the affected groups and their ranges
//   current   out_sp rows inside those ranges, consolidated: Oc, each
//             affected group's tie set at its real weights
//   verdict   with m the rank of Oc_g, the group KEEPS its maximum iff an
//             Oc_g row is not taken away by a vanish row of D, or a delta row
//             of rank >= m is present after the tick.  A group with rows in
//             Oc and neither refills: its maximum drops or it empties.
//             Proof that the others need nothing of in_sp: every present row
//             of rank m is in Oc_g and no row of rank > m was present, so
//             after the tick the present rows of rank >= m are Oc_g's
//             survivors and delta rows, and one of them exists.
//   insert    D into in_sp
//   slice     groups not refilled: Oc_g at its weights and the delta rows of
//             rank >= m at dw (all of them where Oc_g is empty), whose sums
//             are the new integral weights; refilled groups: their whole run
//             out of in_sp (rows_gathered) and none of Oc_g.  Consolidated
//             into S.
//   select    a row of S is kept iff its rank is that of its group's last row
//   output    consolidate(selected - Oc), appended to out_sp
// A stream on which no group's maximum ever decreases reads nothing of
// in_sp.  The explicit per-op path (a host length sync per phase, as top-K);
// no chaining.  No row is invalid, so nothing can fail after the first write
// to in_sp for a reason the caller controls.
dbsp_status ArgMaxOp::step(dbsp_ctx *c, const DevBatch &delta, DevBatch &out) {
    out = DevBatch{};
    if (delta.n == 0) return DBSP_OK;
    ScopedTimer timer(c, 3, 0.0);
    const int64_t n = delta.n;
    TRY(in_sp.cap_batches(c));
    TRY(out_sp.cap_batches(c));
    uint64_t *pb = nullptr;
    int64_t ng = 0;
    TRY(dbspk::topk_classify(c->stream, delta, trace_args_of(in_sp),
                             group_shift, &pb, &ng));
    ScratchBuf plan(c, pb);
    DevBatch cur;
    {
        DevBatch raw;
        TRY(dbspk::keyrange_gather(c->stream, pb + 2 * n, pb + 3 * n, ng,
                                   trace_args_of(out_sp), 1, &raw));
        TRY(sort_consolidate_batch(c, raw, cur));
    }
    uint64_t *vb = nullptr;
    int64_t n_refill = 0;
    TRY(dbspk::argmax_verdict(c->stream, delta, pb, ng, cur, rank_shift,
                              refill_all, &vb, &n_refill));
    ScratchBuf verdict(c, vb);
    TRY(in_sp.insert_copy(c, delta));
    TRY(in_sp.cap_batches(c));
    // the candidate slice
    std::vector<DevBatch> parts;
    int64_t gathered = 0;
    {
        DevBatch cand;
        TRY(dbspk::argmax_candidates(c->stream, delta, pb, ng, vb, cur,
                                     rank_shift, &cand));
        if (cand.n > 0) parts.push_back(cand);
    }
    if (n_refill > 0) {
        DevBatch runs;
        TRY(dbspk::keyrange_gather(c->stream, vb + ng, vb + 2 * ng, n_refill,
                                   trace_args_of(in_sp), 1, &runs));
        gathered = runs.n;
        if (runs.n > 0) parts.push_back(runs);
    }
    DevBatch slice, sel;
    if (!parts.empty()) TRY(finalize_raw(c, parts, slice));
    TRY(dbspk::argmax_select(c->stream, slice, group_shift, rank_shift, &sel));
    const int64_t moved = cur.n + gathered + slice.n + sel.n;
    free_batch(c, slice);
    // selected - Oc
    dbspk::negate_weights(c->stream, cur.w, cur.n);
    if (cur.n == 0) {
        out = sel;
    } else if (sel.n == 0) {
        out = cur;
    } else {
        TRY(merge_batches(c, sel, cur, out));
        free_batch(c, sel);
        free_batch(c, cur);
    }
    if (out.n == 0) free_batch(c, out);
    if (out.n > 0) TRY(out_sp.insert_copy(c, out));
    groups_seen += ng;
    groups_refilled += n_refill;
    rows_gathered += gathered;
    timer.bytes = 24.0 * (double)moved;
    return DBSP_OK;
}

struct dbsp_argmax_op {
    dbsp_ctx *ctx = nullptr;
    ArgMaxOp op;
};

static bool argmax_args_valid(int group_shift, int rank_shift) {
    return rank_shift >= 0 && rank_shift <= group_shift && group_shift <= 63;
}

// the select stage over a caller's batch: the recompute route
extern "C" dbsp_status dbsp_argmax(dbsp_ctx *c, const dbsp_batch *in,
                                   int group_shift, int rank_shift,
                                   dbsp_batch *out) {
    if (!c || !in || !out || in->len < 0 ||
        !argmax_args_valid(group_shift, rank_shift))
        return DBSP_ERR_INVALID;
    DevBatch res;
    {
        ScopedTimer t(c, 3, 0.0);
        TRY(dbspk::argmax_select(c->stream, as_batch(in), group_shift,
                                 rank_shift, &res));
    }
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_argmax_create(dbsp_ctx *c, int group_shift,
                                          int rank_shift, uint32_t flags,
                                          dbsp_argmax_op **out) {
    if (!c || !out || !argmax_args_valid(group_shift, rank_shift) ||
        (flags & ~(uint32_t)DBSP_ARGMAX_REFILL_ALL))
        return DBSP_ERR_INVALID;
    dbsp_argmax_op *t = new dbsp_argmax_op();
    t->ctx = c;
    t->op.group_shift = group_shift;
    t->op.rank_shift = rank_shift;
    t->op.refill_all = (flags & DBSP_ARGMAX_REFILL_ALL) != 0;
    *out = t;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_argmax_step(dbsp_argmax_op *t, const uint64_t *k,
                                        const uint64_t *v, const int64_t *w,
                                        int64_t n, dbsp_batch *out) {
    if (!t || !out || n < 0) return DBSP_ERR_INVALID;
    dbsp_ctx *c = t->ctx;
    *out = dbsp_batch{nullptr, nullptr, nullptr, 0};
    if (n == 0) return DBSP_OK;
    DevBatch raw, delta, res;
    TRY(alloc_batch(c, n, raw));
    TRY(copy_cols(c, raw, 0, k, v, w, n));
    TRY(sort_consolidate_batch(c, raw, delta));
    const dbsp_status st = t->op.step(c, delta, res);
    free_batch(c, delta);
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    if (st != DBSP_OK) return st;
    put_batch(out, res);
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_argmax_stats(dbsp_argmax_op *t, int64_t *in_rows,
                                         int *in_batches, int64_t *out_rows,
                                         int *out_batches,
                                         int64_t *groups_seen,
                                         int64_t *groups_refilled,
                                         int64_t *rows_gathered) {
    if (!t) return DBSP_ERR_INVALID;
    if (in_rows) *in_rows = t->op.in_sp.total();
    if (in_batches) *in_batches = (int)t->op.in_sp.batches.size();
    if (out_rows) *out_rows = t->op.out_sp.total();
    if (out_batches) *out_batches = (int)t->op.out_sp.batches.size();
    if (groups_seen) *groups_seen = t->op.groups_seen;
    if (groups_refilled) *groups_refilled = t->op.groups_refilled;
    if (rows_gathered) *rows_gathered = t->op.rows_gathered;
    return DBSP_OK;
}

extern "C" dbsp_status dbsp_argmax_destroy(dbsp_argmax_op *t) {
    if (!t) return DBSP_OK;
    t->op.clear(t->ctx);
    (void)hipStreamSynchronize(t->ctx->stream);
    delete t;
    return DBSP_OK;
}

// ---- query 7: the highest bids of the last tumbled window (queries/q7.rs:
// 45-94) ----
//   front      bids as k = date_time << 27 | price, v = auction << 32 |
//              bidder (q7.rs:47-54), so key order is time order.  A field too
//              wide for its place is caught on the device as for query 19:
//              a non-empty second stream makes the step DBSP_ERR_INVALID
//              before any state changes.
//   watermark  watermark_monotonic(date_time - 4000) (q7.rs:60-61,
//              WATERMARK_INTERVAL_SECONDS, queries/mod.rs:12) from the tick's
//              largest date_time, the last key of the sorted delta, on the
//              host; the precondition of q5 (max >= lag) applies and the
//              arithmetic is wm_advance's.  rounded = wm - wm % 10000, the
//              window [rounded saturating-minus 10000, rounded) (q7.rs:64-70).
//   window     the window stage by its host-bounds route over the
//              bid-by-time spine, bounds << 27 (q7.rs:73): k_wm_update and
//              the chained ranges launch of q5 and q8 are not involved
//   tail       rows mapped to k' = price << 32 | date_time (q7.rs:74-79),
//              sorted, into the arg-max operator with group_shift 59 and
//              rank_shift 32: k' < 2^59, one group, its rank the price.  The
//              operator's output is the tick's.
// Every tumble of the window retracts the old maximum, so it refills; the
// tick's delta is the whole window then anyway.  The bid-by-time spine grows
// as q5's and q8's do.
static dbsp_status q7_step(dbsp_engine *e, const dbsp_event *d_ev, int64_t n) {
    dbsp_ctx *c = e->ctx;
    constexpr uint64_t TUMBLE_MS = 10000, WM_LAG_MS = 4000;
    DevBatch d, dummy;
    int64_t n_wide = 0;
    TRY(build_deltas(e, d_ev, n, d, dummy, false, &n_wide));
    if (n_wide != 0) {
        free_batch(c, d);
        HIP_CHECK_ST(hipStreamSynchronize(c->stream));
        return DBSP_ERR_INVALID;
    }
    engine_free_output(e);
    if (d.n == 0) {  // no bids: the watermark and the window stand still
        free_batch(c, d);
        return DBSP_OK;
    }
    uint64_t last = 0;
    TRY(dbsp_d2h(c, &last, d.k + d.n - 1, sizeof(last)));
    const uint64_t gmax = last >> 27;
    uint64_t *st = e->q7_wm;
    uint64_t wm = st[0];
    if (gmax > 0) wm = std::max(wm, gmax - WM_LAG_MS);
    const uint64_t rounded = wm - wm % TUMBLE_MS;
    const uint64_t s1 = rounded >= TUMBLE_MS ? rounded - TUMBLE_MS : 0;
    const uint64_t e1 = rounded;
    WindowLeg leg{&e->q7_bt, &d, nullptr, L_WIN};
    TRY(e->q7_bt.cap_batches(c));
    leg.ta = trace_args_of(e->q7_bt);
    leg.nreg = 3 * leg.ta.nb + 1;
    TRY(leg.table.alloc(c, (size_t)leg.nreg * 5 * 8 + 8));
    std::vector<DevBatch> wb_raw;
    {
        ScopedTimer t(c, 4, 0.0);
        TRY(dbspk::window_ranges_multi(c->stream, leg.ta, d.k, d.n,
                                       (int)st[3], st[1] << 27, st[2] << 27,
                                       s1 << 27, e1 << 27,
                                       leg.table.as<int64_t>(),
                                       c->d_len + leg.slot));
        TRY(read_len(c, leg.slot, 1));
        TRY(window_emit(c, leg, wb_raw));
    }
    st[0] = wm;
    st[1] = s1;
    st[2] = e1;
    st[3] = 1;
    TRY(e->q7_bt.insert(c, d));
    DevBatch wbr, dBP;
    if (!wb_raw.empty()) TRY(finalize_raw(c, wb_raw, wbr));
    if (wbr.n > 0) {
        DevBatch raw;
        TRY(alloc_batch(c, wbr.n, raw));
        TRY(dbspk::map_price_time(c->stream, wbr, raw));
        TRY(sort_consolidate_batch(c, raw, dBP));
    }
    free_batch(c, wbr);
    const dbsp_status res = e->argmax.step(c, dBP, e->output);
    free_batch(c, dBP);
    HIP_CHECK_ST(hipStreamSynchronize(c->stream));
    return res;
}

extern "C" dbsp_status dbsp_engine_argmax_stats(dbsp_engine *e,
                                                int64_t *in_rows,
                                                int64_t *out_rows,
                                                int64_t *groups_seen,
                                                int64_t *groups_refilled,
                                                int64_t *rows_gathered) {
    if (!e || e->query != 7) return DBSP_ERR_INVALID;
    if (in_rows) *in_rows = e->argmax.in_sp.total();
    if (out_rows) *out_rows = e->argmax.out_sp.total();
    if (groups_seen) *groups_seen = e->argmax.groups_seen;
    if (groups_refilled) *groups_refilled = e->argmax.groups_refilled;
    if (rows_gathered) *rows_gathered = e->argmax.rows_gathered;
    return DBSP_OK;
}
