// kernels.hip — hand-written CDNA4 (gfx950) kernels for the DBSP Z-set hot path.
//
// MI355X-native design notes (see DESIGN.md for the full rationale):
//  * Every op here is HBM-bound integer/byte work (no dense contraction ⇒ no
//    MFMA).  The levers are coalescing (SoA u64 columns, 8B/lane loads),
//    LDS staging for the block-local sort/merge phases, and ≫256-workgroup
//    launches with grid-stride loops (256 CUs / 8 XCDs want >2048 blocks
//    before per-XCD L2 effects matter).
//  * Wave width is 64; block size 256 (4 waves) everywhere.
//  * Output sizes are data-dependent (zero-weight elimination,
//    trace/consolidation/mod.rs:32-51) ⇒ count→scan→emit two-phase kernels.
//
// Reference mapping:
//   radix sort + consolidate  <- consolidate_slice / quicksort
//                                (trace/consolidation/mod.rs:91-110, quicksort.rs)
//   merge-path merge          <- ColumnLayerBuilder::push_merge
//                                (trace/layers/column_layer/builders.rs:98-169)
//                                + OrderedBuilder::merge_step (ordered/mod.rs:344-396)
//   join probe/expand         <- Join::eval / JoinTrace::eval
//                                (operator/join.rs:436-473,751-787)
//   aggregate + upsert        <- aggregate/mod.rs:479-547 + upsert.rs:161-208
//   window                    <- time_series/window.rs:144-220
//   shard partition           <- communication/shard.rs:165-199 + hash.rs:9-13

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/dbsp_hip.h"
#include "kernels_iface.hpp"

// ---------------------------------------------------------------------------
// Big-buffer cache.  hipMallocAsync's pool hands a freed multi-GB block back
// to the SAME size-class only a couple of allocations later, so trace-scale
// merges (6.5 GB per output column at 1B rows) were re-carving physical
// pages on almost every call at ~9 GB/s — a 720 ms host stall per column
// (profiles/r01_merge_host_stall.txt).  All product allocations go through
// this free-list instead: blocks >= CACHE_MIN bytes are kept and reused
// best-fit (everything runs on the one ctx stream, so reuse is ordered by
// stream order alone); smaller ones pass through to the pool, which handles
// tick-scale buffers fine.  On allocation failure the cache is dropped and
// the carve retried.
// ---------------------------------------------------------------------------
#include <atomic>
#include <map>
#include <mutex>
#include <unordered_map>

namespace dbspk {
namespace {
// 64 KB: originally only trace-scale buffers (>= 32 MB) were cached, but the
// pipelined tick makes ~12 pool alloc/free calls per tick for ~0.1-3 MB
// buffers, and those hipMallocAsync round-trips (~2-4 us each) were the
// largest remaining host cost at the tick boundary — the free-list reuse is
// ~0.2 us.  Footprint cost is bounded by the pow2 rounding (<= 2x per size
// class) against 288 GB of HBM.
// Two cached bands: tick-scale blocks (64 KB .. small-ceiling) whose pool
// round-trips dominate the pipelined tick's host cost, and trace-scale
// blocks (>= 32 MB) whose pool re-carves cost ~100 ms/GB.  The band between
// stays on the stream-ordered pool: C5-scale ticks allocate many MB-range
// buffers and measured 2x slower with them free-listed.
const size_t CACHE_MIN = []() -> size_t {
    const char *v = getenv("DBSP_CACHE_MIN");  // diagnostic A/B knob
    return v ? (size_t)atoll(v) : (64u << 10);
}();
const size_t CACHE_SMALL_CEIL = []() -> size_t {
    const char *v = getenv("DBSP_CACHE_SMALL_CEIL");
    return v ? (size_t)atoll(v) : (4u << 20);
}();
constexpr size_t CACHE_BIG_MIN = 32u << 20;
// Small-band caching is SELF-DISABLING: if any carve fails (trace-scale
// workloads near the memory limit — the hoarded small blocks keep the pool
// from satisfying a multi-GB request), the failure path drops the free list
// and turns the small band off for the rest of the process, so the cost is
// one sync, not one per tick.  Tick-scale engines never fail and keep it.
std::atomic<bool> g_small_cache_on{true};
inline bool cacheable(size_t bytes) {
    if (bytes >= CACHE_BIG_MIN) return true;
    return bytes >= CACHE_MIN && bytes < CACHE_SMALL_CEIL &&
           g_small_cache_on.load(std::memory_order_relaxed);
}
std::mutex g_cache_mu;
std::unordered_map<void *, size_t> g_cache_live;
std::multimap<size_t, void *> g_cache_free;

void cache_drop_locked(hipStream_t s) {
    for (auto &e : g_cache_free) (void)hipFreeAsync(e.second, s);
    g_cache_free.clear();
}
}  // namespace

hipError_t cache_malloc(void **out, size_t bytes, hipStream_t s) {
    if (cacheable(bytes)) {
        // round carves up to the next power of two and accept cached blocks
        // up to 2x the request: a workload with growing buffers (spine
        // merges, trace cascades) then carves only log2(max/min) times
        // instead of once per size, at <= 2x footprint — cheap against
        // 288 GB of HBM, and the page-mapping stalls dominate otherwise
        size_t msb = (size_t)1 << (63 - __builtin_clzll(bytes));
        if (msb < bytes) bytes = msb << 1;
        std::lock_guard<std::mutex> g(g_cache_mu);
        auto it = g_cache_free.lower_bound(bytes);
        // small classes accept only <= 2x (a 64 MB slack there would let a
        // trace-scale block be wasted on a tick-scale request)
        const size_t slack = bytes >= (32u << 20) ? (64u << 20) : 0;
        if (it != g_cache_free.end() && it->first <= 2 * bytes + slack) {
            *out = it->second;
            g_cache_live.emplace(it->second, it->first);
            g_cache_free.erase(it);
            return hipSuccess;
        }
    }
    if (bytes >= CACHE_BIG_MIN) {
        // big-band carve: flush the small band back to the pool first —
        // stream-ordered frees are reusable by this very carve, and a
        // hoarded small band otherwise forces the pool to map fresh pages
        // per multi-GB request (~120 ms each at trace scale).  Tick-scale
        // engines do no big carves in steady state, so their band persists.
        std::lock_guard<std::mutex> g(g_cache_mu);
        for (auto it = g_cache_free.begin();
             it != g_cache_free.end() && it->first < CACHE_BIG_MIN;) {
            (void)hipFreeAsync(it->second, s);
            it = g_cache_free.erase(it);
        }
    }
    static const bool cstats = []() {
        const char *v = getenv("DBSP_CACHE_STATS");
        return v && v[0] == '1';
    }();
    double tc0 = 0;
    if (cstats && bytes >= CACHE_BIG_MIN) {
        struct timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        tc0 = ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
    }
    hipError_t e = hipMallocAsync(out, bytes, s);
    if (cstats && bytes >= CACHE_BIG_MIN) {
        struct timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        double dt = ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6 - tc0;
        size_t nsm = 0, live = 0;
        {
            std::lock_guard<std::mutex> g(g_cache_mu);
            for (auto &kv : g_cache_live)
                if (kv.second < CACHE_BIG_MIN) { nsm++; live += kv.second; }
        }
        fprintf(stderr, "[carve] %.1f MB in %.1f ms (small live: %zu blks %.1f MB)\n",
                bytes / 1048576.0, dt, nsm, live / 1048576.0);
    }
    if (e != hipSuccess) {
        g_small_cache_on.store(false, std::memory_order_relaxed);
        std::lock_guard<std::mutex> g(g_cache_mu);
        cache_drop_locked(s);
        (void)hipStreamSynchronize(s);
        e = hipMallocAsync(out, bytes, s);
    }
    if (e == hipSuccess && cacheable(bytes)) {
        std::lock_guard<std::mutex> g(g_cache_mu);
        g_cache_live.emplace(*out, bytes);
    }
    return e;
}

hipError_t cache_free(void *p, hipStream_t s) {
    if (!p) return hipSuccess;
    {
        std::lock_guard<std::mutex> g(g_cache_mu);
        auto it = g_cache_live.find(p);
        if (it != g_cache_live.end()) {
            const size_t sz = it->second;
            g_cache_live.erase(it);
            if (sz < CACHE_BIG_MIN &&
                !g_small_cache_on.load(std::memory_order_relaxed)) {
                // small band disabled: return to the pool instead of hoarding
            } else {
                g_cache_free.emplace(sz, p);
                return hipSuccess;
            }
        }
    }
    return hipFreeAsync(p, s);
}

void cache_trim(hipStream_t s) {
    std::lock_guard<std::mutex> g(g_cache_mu);
    cache_drop_locked(s);
}

// Explicit policy switch: trace-scale engines (C5's 1B-row spine) turn the
// small band OFF at init — measured on MI355X, routing their tick-scale
// churn away from the stream-ordered pool leaves the pool unable to serve
// the per-tick multi-GB spine carves from retained slabs (0.3 ms -> 240 ms
// per carve), tripling the step.  Tick-scale engines keep it on.
void cache_small_set(bool on, hipStream_t s) {
    if (getenv("DBSP_CACHE_STATS"))
        fprintf(stderr, "[cache] small band %s\n", on ? "on" : "off");
    g_small_cache_on.store(on, std::memory_order_relaxed);
    if (!on) {
        std::lock_guard<std::mutex> g(g_cache_mu);
        for (auto it = g_cache_free.begin();
             it != g_cache_free.end() && it->first < CACHE_BIG_MIN;) {
            (void)hipFreeAsync(it->second, s);
            it = g_cache_free.erase(it);
        }
    }
}
}  // namespace dbspk


#define WAVE 64
#define BLK 256
#define SORT_ITEMS 8
#define SORT_TILE (BLK * SORT_ITEMS)  // 2048 rows per block

#define HIP_CHECK(x)                                                      \
    do {                                                                  \
        hipError_t err_ = (x);                                            \
        if (err_ != hipSuccess) {                                         \
            fprintf(stderr, "HIP error %s at %s:%d\n",                    \
                    hipGetErrorString(err_), __FILE__, __LINE__);         \
            return DBSP_ERR_INTERNAL;                                     \
        }                                                                 \
    } while (0)

#define TRY_K(x)                                                          \
    do {                                                                  \
        dbsp_status st_ = (x);                                            \
        if (st_ != DBSP_OK) return st_;                                   \
    } while (0)

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------
// generic grid-stride helpers
// ---------------------------------------------------------------------------

static inline dim3 grid_for(int64_t n, int per_block = BLK) {
    int64_t b = ceil_div(n, per_block);
    if (b < 1) b = 1;
    if (b > 16384) b = 16384;  // grid-stride the rest (Guideline 11)
    return dim3((uint32_t)b);
}

__global__ void k_fill_u64(uint64_t *p, uint64_t v, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        p[i] = v;
}

// ---------------------------------------------------------------------------
// exclusive scan (u64) — 3-kernel recursive device scan
// ---------------------------------------------------------------------------

__device__ inline uint64_t wave_scan_excl(uint64_t x, uint64_t &total) {
    // inclusive shuffle scan over the 64-lane wave, then convert
    uint64_t v = x;
    for (int d = 1; d < WAVE; d <<= 1) {
        uint64_t up = __shfl_up(v, d, WAVE);
        if ((threadIdx.x & (WAVE - 1)) >= d) v += up;
    }
    total = __shfl(v, WAVE - 1, WAVE);
    return v - x;
}

// per-block scan of SORT_TILE elements; writes per-block total
__global__ void k_scan_block(const uint64_t *in, uint64_t *out,
                             uint64_t *block_totals, int64_t n) {
    __shared__ uint64_t wave_tot[BLK / WAVE];
    int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    uint64_t vals[SORT_ITEMS];
    uint64_t thread_sum = 0;
    for (int i = 0; i < SORT_ITEMS; i++) {
        int64_t idx = base + threadIdx.x * SORT_ITEMS + i;
        vals[i] = idx < n ? in[idx] : 0;
        thread_sum += vals[i];
    }
    uint64_t wave_total;
    uint64_t thread_off = wave_scan_excl(thread_sum, wave_total);
    int wid = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) wave_tot[wid] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t acc = 0;
        for (int w = 0; w < BLK / WAVE; w++) {
            uint64_t t = wave_tot[w];
            wave_tot[w] = acc;
            acc += t;
        }
        if (block_totals) block_totals[blockIdx.x] = acc;
    }
    __syncthreads();
    uint64_t off = wave_tot[wid] + thread_off;
    for (int i = 0; i < SORT_ITEMS; i++) {
        int64_t idx = base + threadIdx.x * SORT_ITEMS + i;
        if (idx < n) out[idx] = off;
        off += vals[i];
    }
}

__global__ void k_scan_add(uint64_t *out, const uint64_t *block_offsets,
                           int64_t n) {
    int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    uint64_t off = block_offsets[blockIdx.x];
    for (int i = threadIdx.x; i < SORT_TILE; i += BLK) {
        int64_t idx = base + i;
        if (idx < n) out[idx] += off;
    }
}

// host-side recursive exclusive scan; returns total via d_total (device, may be
// null).  in and out may alias.
struct ScanTemp {
    // enough levels for 2048^4 = 1.7e13 elements
    uint64_t *lvl[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t lvl_n[4] = {0, 0, 0, 0};
};

static dbsp_status scan_exclusive(hipStream_t s, const uint64_t *in,
                                  uint64_t *out, int64_t n, uint64_t *h_total) {
    if (n == 0) {
        if (h_total) *h_total = 0;
        return DBSP_OK;
    }
    // collect level sizes
    int64_t sizes[5];
    int levels = 0;
    int64_t m = n;
    while (true) {
        sizes[levels] = m;
        m = ceil_div(m, SORT_TILE);
        if (sizes[levels] <= SORT_TILE) break;
        levels++;
        if (levels >= 4) return DBSP_ERR_INVALID;
    }
    // allocate block-total arrays per level
    uint64_t *tot[5] = {nullptr};
    for (int l = 0; l <= levels; l++) {
        int64_t nb = ceil_div(sizes[l], SORT_TILE);
        HIP_CHECK(dbspk::cache_malloc((void **)&tot[l], (nb + 1) * sizeof(uint64_t), s));
    }
    // down-sweep: scan each level, producing block totals
    const uint64_t *src = in;
    uint64_t *dst = out;
    for (int l = 0; l <= levels; l++) {
        int64_t nb = ceil_div(sizes[l], SORT_TILE);
        k_scan_block<<<dim3((uint32_t)nb), BLK, 0, s>>>(src, dst, tot[l], sizes[l]);
        src = tot[l];
        dst = tot[l];  // scan totals in place at next level
    }
    // top level: tot[levels] has <= SORT_TILE entries, already scanned in the
    // loop? no — the loop scanned level l's DATA and wrote raw totals to tot[l].
    // The next iteration scans tot[l] (as data) into itself and writes raw
    // totals to tot[l+1].  After the loop, tot[levels] holds RAW totals of the
    // last scanned array; scan it with a single block.
    {
        int64_t nb_last = ceil_div(sizes[levels], SORT_TILE);
        k_scan_block<<<dim3(1), BLK, 0, s>>>(tot[levels], tot[levels], tot[levels] + nb_last,
                                             nb_last);
        // up-sweep: add scanned block offsets back down
        for (int l = levels; l >= 0; l--) {
            int64_t nb = ceil_div(sizes[l], SORT_TILE);
            uint64_t *data = (l == 0) ? out : tot[l - 1];
            if (nb > 1 || l > 0) {
                uint64_t *offs = tot[l];
                k_scan_add<<<dim3((uint32_t)nb), BLK, 0, s>>>(data, offs, sizes[l]);
            }
        }
        // total = tot[levels][nb_last] (one past the scanned entries)
        if (h_total) {
            HIP_CHECK(hipMemcpyAsync(h_total, tot[levels] + nb_last, sizeof(uint64_t),
                                     hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
    }
    for (int l = 0; l <= levels; l++) HIP_CHECK(dbspk::cache_free(tot[l], s));
    return DBSP_OK;
}

// ---------------------------------------------------------------------------
// LSD radix sort of (k, v, w) rows by composite (k major, v minor)
// 8-bit digits; bytes 0..7 = v, 8..15 = k; passes above the detected
// significant byte of max(v)/max(k) are skipped.
// ---------------------------------------------------------------------------

__global__ void k_minmax_u64(const uint64_t *a, const uint64_t *b, int64_t n,
                             uint64_t *out /* [4]: maxA,maxB,minA,minB */) {
    __shared__ uint64_t smax[2];
    __shared__ uint64_t smin[2];
    if (threadIdx.x == 0) {
        smax[0] = 0; smax[1] = 0;
        smin[0] = ~0ull; smin[1] = ~0ull;
    }
    __syncthreads();
    uint64_t ma = 0, mb = 0, na = ~0ull, nb = ~0ull;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        ma = max(ma, a[i]);
        mb = max(mb, b[i]);
        na = min(na, a[i]);
        nb = min(nb, b[i]);
    }
    atomicMax((unsigned long long *)&smax[0], (unsigned long long)ma);
    atomicMax((unsigned long long *)&smax[1], (unsigned long long)mb);
    atomicMin((unsigned long long *)&smin[0], (unsigned long long)na);
    atomicMin((unsigned long long *)&smin[1], (unsigned long long)nb);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax((unsigned long long *)&out[0], (unsigned long long)smax[0]);
        atomicMax((unsigned long long *)&out[1], (unsigned long long)smax[1]);
        atomicMin((unsigned long long *)&out[2], (unsigned long long)smin[0]);
        atomicMin((unsigned long long *)&out[3], (unsigned long long)smin[1]);
    }
}

__device__ inline uint32_t sort_digit(uint64_t k, uint64_t v, int byte,
                                      uint64_t kbase, uint64_t vbase) {
    uint64_t limb = byte < 8 ? v - vbase : k - kbase;
    int sh = (byte & 7) * 8;
    return (uint32_t)((limb >> sh) & 0xFF);
}

// histogram: counts[d * nblocks + blk] (digit-major so one exclusive scan of
// the flat array yields combined digit-base + block-offset)
__global__ void k_radix_hist(const uint64_t *k, const uint64_t *v, int64_t n,
                             int byte, uint64_t kbase, uint64_t vbase,
                             int64_t nblocks, uint64_t *counts) {
    __shared__ uint32_t hist[256];
    for (int i = threadIdx.x; i < 256; i += BLK) hist[i] = 0;
    __syncthreads();
    int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    for (int i = threadIdx.x; i < SORT_TILE; i += BLK) {
        int64_t idx = base + i;
        if (idx < n) atomicAdd(&hist[sort_digit(k[idx], v[idx], byte, kbase, vbase)], 1u);
    }
    __syncthreads();
    for (int d = threadIdx.x; d < 256; d += BLK)
        counts[(int64_t)d * nblocks + blockIdx.x] = hist[d];
}

// stable scatter: in-LDS 8 x 1-bit split of (digit, local idx) pairs, then
// rank within digit run + scanned global base.
__global__ void k_radix_scatter(const uint64_t *k_in, const uint64_t *v_in,
                                const int64_t *w_in, int64_t n, int byte,
                                uint64_t kbase, uint64_t vbase,
                                int64_t nblocks, const uint64_t *scanned,
                                uint64_t *k_out, uint64_t *v_out,
                                int64_t *w_out) {
    __shared__ uint32_t buf_a[SORT_TILE];
    __shared__ uint32_t buf_b[SORT_TILE];
    __shared__ uint32_t run_start[256];
    __shared__ uint64_t wave_tot[BLK / WAVE];

    int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    int64_t tile_n = min((int64_t)SORT_TILE, n - base);
    if (tile_n <= 0) return;

    // load packed (digit << 16 | idx)
    for (int i = threadIdx.x; i < SORT_TILE; i += BLK) {
        uint32_t d = 0xFF;  // pad with max digit so pads sort last
        if (i < tile_n) d = sort_digit(k_in[base + i], v_in[base + i], byte, kbase, vbase);
        buf_a[i] = (d << 16) | (uint32_t)i;
    }
    __syncthreads();

    uint32_t *src = buf_a, *dst = buf_b;
    for (int bit = 0; bit < 8; bit++) {
        // stable 1-bit split: zeros first (keep order), then ones
        // per-thread sequential items for stable ordering
        uint64_t flags[SORT_ITEMS];
        uint64_t tsum = 0;
        for (int i = 0; i < SORT_ITEMS; i++) {
            int idx = threadIdx.x * SORT_ITEMS + i;
            flags[i] = ((src[idx] >> (16 + bit)) & 1) ? 0 : 1;  // 1 == is-zero
            tsum += flags[i];
        }
        uint64_t wtotal;
        uint64_t toff = wave_scan_excl(tsum, wtotal);
        int wid = threadIdx.x / WAVE;
        if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) wave_tot[wid] = wtotal;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t acc = 0;
            for (int w = 0; w < BLK / WAVE; w++) {
                uint64_t t = wave_tot[w];
                wave_tot[w] = acc;
                acc += t;
            }
            run_start[0] = (uint32_t)acc;  // total zeros, reuse smem slot
        }
        __syncthreads();
        uint64_t zeros_before = wave_tot[wid] + toff;
        uint32_t total_zeros = run_start[0];
        __syncthreads();
        for (int i = 0; i < SORT_ITEMS; i++) {
            int idx = threadIdx.x * SORT_ITEMS + i;
            uint32_t e = src[idx];
            uint32_t pos;
            if (flags[i]) {
                pos = (uint32_t)zeros_before;
                zeros_before++;
            } else {
                pos = total_zeros + (uint32_t)(idx - zeros_before);
            }
            dst[pos] = e;
        }
        __syncthreads();
        uint32_t *t = src; src = dst; dst = t;
    }

    // run starts per digit
    for (int i = threadIdx.x; i < 256; i += BLK) run_start[i] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = threadIdx.x; i < tile_n; i += BLK) {
        uint32_t d = src[i] >> 16;
        if (i == 0 || (src[i - 1] >> 16) != d) run_start[d] = i;
    }
    __syncthreads();

    // scatter rows to scanned global positions
    for (int i = threadIdx.x; i < tile_n; i += BLK) {
        uint32_t e = src[i];
        uint32_t d = e >> 16;
        uint32_t local = (uint32_t)i - run_start[d];
        uint64_t pos = scanned[(int64_t)d * nblocks + blockIdx.x] + local;
        int64_t gi = base + (e & 0xFFFF);
        k_out[pos] = k_in[gi];
        v_out[pos] = v_in[gi];
        w_out[pos] = w_in[gi];
    }
}

// ---------------------------------------------------------------------------
// fused single-workgroup sort+consolidate for small batches (n <= 8192)
//
// A 40k-event tick produces per-stream deltas of a few thousand rows; the
// multi-kernel radix path costs ~30 launches + 3 host syncs there, which
// dominates the tick.  This kernel does the whole consolidate_slice job —
// LSD radix over a permutation held in LDS, then dedup-accumulate and
// zero-drop — in ONE launch with the output length left in device memory.
// 1024 threads = 16 waves on one CU; the permutation entry
// (key16 << 13 | idx, u32) carries the next 16 key bits so digit passes are
// LDS-only, ranks come from bit-sliced wave ballots over strided positions
// (stable by construction), and the entry arrays ping-pong between two
// 32 KiB LDS buffers.  See the kernel's own comment for the details.
// ---------------------------------------------------------------------------

#define FUSE_MAX 8192
#define FUSE_THREADS 1024
#define FUSE_ITEMS (FUSE_MAX / FUSE_THREADS)  // 8
#define FUSE_DIGITS 16                        // 4-bit digits, ranked per pass

// block-wide exclusive scan over FUSE_MAX u32 flags held per-thread
// (16 consecutive items per thread); returns thread's exclusive offset and
// writes the block total to *total (all threads).
__device__ inline uint32_t fuse_scan(uint32_t thread_sum, uint32_t *wave_tot,
                                     uint32_t *total) {
    uint32_t v = thread_sum;
    for (int d = 1; d < WAVE; d <<= 1) {
        uint32_t up = __shfl_up(v, d, WAVE);
        if ((threadIdx.x & (WAVE - 1)) >= d) v += up;
    }
    int wid = threadIdx.x / WAVE;  // 16 waves
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) wave_tot[wid] = v;
    __syncthreads();
    if (threadIdx.x < WAVE) {
        // wave 0 scans the 16 wave totals with shuffles (the serial
        // thread-0 loop cost ~1 us of LDS latency per call)
        const int nw = FUSE_THREADS / WAVE;
        uint32_t t = threadIdx.x < nw ? wave_tot[threadIdx.x] : 0;
        uint32_t sc = t;
        for (int d = 1; d < nw; d <<= 1) {
            uint32_t up = __shfl_up(sc, d, WAVE);
            if ((int)threadIdx.x >= d) sc += up;
        }
        if ((int)threadIdx.x < nw) wave_tot[threadIdx.x] = sc - t;
        if ((int)threadIdx.x == nw - 1) wave_tot[nw] = sc;
    }
    __syncthreads();
    uint32_t r = wave_tot[wid] + (v - thread_sum);
    *total = wave_tot[FUSE_THREADS / WAVE];
    __syncthreads();
    return r;
}

// LDS of the fused sort (~96 KiB): declared by the kernels and handed to
// sort_cons_body, so a kernel that runs other phases before the sort can use
// the buffers for them first
#define SORT_CONS_LDS                                                      \
    __shared__ alignas(16) uint32_t bufA[FUSE_MAX];                        \
    __shared__ alignas(16) uint32_t bufB[FUSE_MAX];                        \
    __shared__ uint32_t cnt[FUSE_MAX]; /* ballot cells / f64 head pos */   \
    __shared__ uint32_t wave_tot[FUSE_THREADS / WAVE + 1];                 \
    __shared__ uint64_t smax[2];                                           \
    __shared__ uint64_t smin[2];

// ---- small-batch path of the fused sort (integer weights, n <= 1024) ----
// One row per thread, held in registers.  Integer sums do not depend on the
// order of their terms, so the sort needs neither stability nor an index
// payload: it orders (k, v) and carries w along.  Threads past n hold the pad
// row (~0, ~0, w = 0); a pad either joins a real (~0, ~0) segment adding 0 or
// forms a zero-weight segment that the compaction drops, so the consolidation
// treats all 1024 rows alike.

// lane ^ JJ exchange inside the wave: quad permutes for 1 and 2, else bpermute
template <int JJ>
__device__ __forceinline__ uint32_t lane_xor32(uint32_t x) {
    if constexpr (JJ == 1)
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true);
    else if constexpr (JJ == 2)
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, true);
    else
        return (uint32_t)__shfl_xor((int)x, JJ, WAVE);
}
template <int JJ>
__device__ __forceinline__ uint64_t lane_xor64(uint64_t x) {
    const uint32_t lo = lane_xor32<JJ>((uint32_t)x);
    const uint32_t hi = lane_xor32<JJ>((uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// one compare-exchange of a bitonic network against the partner's row: the
// lower position of an ascending pair (and the upper of a descending one)
// keeps the smaller (k, v).  Equal keys never move, so both sides agree.
__device__ __forceinline__ void small_cmpx(uint64_t &k, uint64_t &v,
                                           int64_t &w, uint64_t pk,
                                           uint64_t pv, int64_t pw,
                                           bool keep_min) {
    const bool plt = pk < k || (pk == k && pv < v);
    const bool pgt = pk > k || (pk == k && pv > v);
    if (keep_min ? plt : pgt) {
        k = pk;
        v = pv;
        w = pw;
    }
}

// the compare distances JJ, JJ/2, .., 1 of one merge, all inside the wave
template <int JJ>
__device__ __forceinline__ void small_wave_merge(uint64_t &k, uint64_t &v,
                                                 int64_t &w, bool up,
                                                 int lane) {
    const uint64_t pk = lane_xor64<JJ>(k);
    const uint64_t pv = lane_xor64<JJ>(v);
    const int64_t pw = (int64_t)lane_xor64<JJ>((uint64_t)w);
    small_cmpx(k, v, w, pk, pv, pw, ((lane & JJ) == 0) == up);
    if constexpr (JJ > 1) small_wave_merge<JJ / 2>(k, v, w, up, lane);
}

// exclusive prefix of this wave and the total over the 16 per-wave counts in
// cells[0..16), computed by every wave for itself: one barrier (the
// caller's, after the cells were written) instead of fuse_scan's three
__device__ __forceinline__ uint32_t small_wave_base(const uint32_t *cells,
                                                    int wid, int lane,
                                                    uint32_t *total) {
    const int nw = FUSE_THREADS / WAVE;
    const uint32_t t = lane < nw ? cells[lane] : 0;
    uint32_t sc = t;
    for (int d = 1; d < nw; d <<= 1) {
        const uint32_t up = __shfl_up(sc, d, WAVE);
        if (lane >= d) sc += up;
    }
    *total = __shfl(sc, nw - 1, WAVE);
    return __shfl(sc - t, wid, WAVE);
}

// Sort + consolidate the block's rows (thread tid holds row tid, pads past
// n) into ok/ov/ow and *out_len.  0 < n <= FUSE_THREADS, block-uniform; all
// 1024 threads call it.  Global memory is touched by the final store only.
//
// Bitonic network over p2 = max(64, pow2 >= n) positions.  Distances below 64
// exchange across lanes; distances >= 64 go through LDS, double-buffered so
// each costs ONE block barrier (6 at p2 = 512, 10 at 1024).  Waves wholly
// past p2 hold pads only (already in place: pads are the maximum) and skip
// the compares but reach every barrier.  The consolidation adds 4 barriers.
//
// LDS: bufA = k[2][1024] + w[2][1024], bufB = v[2][1024] + sums[1024] +
// edge k/v[16]; cnt[0..16) holds the second scan's cells.
__device__ __forceinline__ void sort_cons_small_rows(
    uint64_t k, uint64_t v, int64_t w, int64_t n, uint64_t *ok, uint64_t *ov,
    int64_t *ow, int64_t *out_len, uint32_t *bufA, uint32_t *bufB,
    uint32_t *cnt, uint32_t *wave_tot) {
    const int tid = threadIdx.x;
    const int wid = tid / WAVE;
    const int lane = tid % WAVE;
    const uint64_t lt = ((uint64_t)1 << lane) - 1;
    uint64_t *xk = (uint64_t *)bufA;
    int64_t *xw = (int64_t *)bufA + 2 * FUSE_THREADS;
    uint64_t *xv = (uint64_t *)bufB;
    unsigned long long *sums =
        (unsigned long long *)bufB + 2 * FUSE_THREADS;
    uint64_t *edge_k = (uint64_t *)bufB + 3 * FUSE_THREADS;
    uint64_t *edge_v = edge_k + FUSE_THREADS / WAVE;

    sums[tid] = 0;  // ordered before the adds by the barriers below

    int p2 = WAVE;
    while (p2 < n) p2 <<= 1;
    const bool active = wid * WAVE < p2;  // wave-uniform

    // ---- sort ----
    if (active) {
        small_wave_merge<1>(k, v, w, (tid & 2) == 0, lane);
        small_wave_merge<2>(k, v, w, (tid & 4) == 0, lane);
        small_wave_merge<4>(k, v, w, (tid & 8) == 0, lane);
        small_wave_merge<8>(k, v, w, (tid & 16) == 0, lane);
        small_wave_merge<16>(k, v, w, (tid & 32) == 0, lane);
        small_wave_merge<32>(k, v, w, (tid & 64) == 0, lane);
    }
    int step = 0;
    for (int kk = 2 * WAVE; kk <= p2; kk <<= 1) {
        const bool up = (tid & kk) == 0;
        for (int jj = kk >> 1; jj >= WAVE; jj >>= 1, step++) {
            const int b = (step & 1) * FUSE_THREADS;
            if (active) {
                xk[b + tid] = k;
                xv[b + tid] = v;
                xw[b + tid] = w;
            }
            __syncthreads();
            if (active) {
                const int p = b + (tid ^ jj);  // < p2: jj < p2 and tid < p2
                small_cmpx(k, v, w, xk[p], xv[p], xw[p],
                           ((tid & jj) == 0) == up);
            }
        }
        if (active) small_wave_merge<32>(k, v, w, up, lane);
    }

    // ---- consolidate ----
    // head flags from the left neighbour; lane 0 takes the previous wave's
    // last row through LDS
    if (lane == WAVE - 1) {
        edge_k[wid] = k;
        edge_v[wid] = v;
    }
    __syncthreads();
    uint64_t lk_ = __shfl_up(k, 1, WAVE);
    uint64_t lv_ = __shfl_up(v, 1, WAVE);
    if (lane == 0 && wid > 0) {
        lk_ = edge_k[wid - 1];
        lv_ = edge_v[wid - 1];
    }
    const bool head = tid == 0 || lk_ != k || lv_ != v;
    const uint64_t hm = __ballot(head);
    if (lane == 0) wave_tot[wid] = (uint32_t)__popcll(hm);
    __syncthreads();
    uint32_t nseg;
    const uint32_t hbase = small_wave_base(wave_tot, wid, lane, &nseg);
    // heads at or before this row, minus 1: < 1024 by construction
    const uint32_t seg =
        hbase + (uint32_t)__popcll(hm & lt) + (head ? 1u : 0u) - 1u;
    if (w != 0) atomicAdd(&sums[seg], (unsigned long long)w);
    __syncthreads();
    const int64_t tot = head ? (int64_t)sums[seg] : 0;
    const bool nz = tot != 0;  // a nonzero segment holds a real row
    const uint64_t zm = __ballot(nz);
    if (lane == 0) cnt[wid] = (uint32_t)__popcll(zm);
    __syncthreads();
    uint32_t nout;
    const uint32_t zbase = small_wave_base(cnt, wid, lane, &nout);
    const uint32_t p = zbase + (uint32_t)__popcll(zm & lt);
    if (nz && (int64_t)p < n) {
        ok[p] = k;
        ov[p] = v;
        ow[p] = tot;
    }
    if (tid == 0) *out_len = (int64_t)nout;
}

template <typename W>
__device__ __forceinline__ void sort_cons_body(
    const uint64_t *kin, const uint64_t *vin, const W *win, int64_t n,
    uint64_t *tk, uint64_t *tv, W *tw, uint64_t *ok, uint64_t *ov, W *ow,
    int64_t *out_len, uint32_t *bufA, uint32_t *bufB, uint32_t *cnt,
    uint32_t *wave_tot, uint64_t *smax, uint64_t *smin) {
    // Fused sort+consolidate of one raw batch by one workgroup (n <= 8192).
    //
    // LSD radix over 4-bit digits of the concatenated (k - kmin, v - vmin)
    // key, restructured around the 64-wide wavefront:
    //  - positions are STRIDED (row i handled by lane i%64 of wave (i/64)%16
    //    in round i/1024), so every LDS access is conflict-free and ranks
    //    assigned in (digit, round, wave, lane) order equal position order —
    //    i.e. the sort is stable without per-thread counters;
    //  - ranks come from 4 bit-sliced wave ballots per round (no 16x1024
    //    counter array, no per-item LDS counter increments); per-(digit,
    //    round, wave) totals live in a 16*8*16-cell array scanned by the
    //    block scan;
    //  - entries carry the NEXT 16 key bits next to the row index
    //    (entry = key16 << 13 | idx), so digit passes never touch global
    //    memory: one gather per 4-pass group rebuilds the entries.
    // The consolidation reuses the same ballot machinery for head flags and
    // the nonzero compaction.
    const int tid = threadIdx.x;
    const int wid = tid / WAVE;
    const int lane = tid % WAVE;
    const uint64_t lt = ((uint64_t)1 << lane) - 1;

    if (n == 0) {
        if (tid == 0) *out_len = 0;
        return;
    }

    if constexpr (sizeof(W) == 8 && (W)0.5 == (W)0) {  // integer weights
        if (n <= FUSE_THREADS) {  // block-uniform: one row per thread
            const bool real = tid < n;
            const uint64_t k = real ? kin[tid] : ~0ull;
            const uint64_t v = real ? vin[tid] : ~0ull;
            const int64_t w = real ? (int64_t)win[tid] : 0;
            sort_cons_small_rows(k, v, w, n, ok, ov, (int64_t *)ow, out_len,
                                 bufA, bufB, cnt, wave_tot);
            return;
        }
    }

    const int rounds =(int)((n + FUSE_THREADS - 1) / FUSE_THREADS);  // <= 8
    const int nwaves = FUSE_THREADS / WAVE;
    uint32_t *src = bufA, *dst = bufB;

    if (n <= 2048) {
        // ---- bitonic fast path ----
        // (f64 weights, and integer batches of 1025..2048 rows: smaller
        // integer batches left through sort_cons_small_rows above)
        // Sub-2k tick batches (delta sides, tick outputs) are where the
        // radix path is pass-count-bound (~35 us regardless of n: ~16+
        // digit passes of block-wide ballots and syncs).  A stable LDS
        // bitonic over (k, v, idx) — idx as tiebreak keeps positions
        // identical to the stable radix, so the f64 position-ordered sums
        // stay bit-equal — runs them in ~10-20 us.  Pair-indexed so every
        // thread does a real compare.  bufA/bufB are reused as the u64 key
        // arrays and cnt as the index payload; the result lands in src in
        // the radix entry layout (idx in the low 13 bits) so the
        // consolidation below is shared by both paths.  Beyond 2k the pass
        // count (log^2) overtakes the radix and the radix path stays.
        uint64_t *lk = (uint64_t *)bufA;
        uint64_t *lv = (uint64_t *)bufB;
        uint32_t *lidx = cnt;
        int64_t p2 = 1;
        while (p2 < n) p2 <<= 1;
        for (int64_t i = tid; i < p2; i += FUSE_THREADS) {
            lk[i] = i < n ? kin[i] : ~0ull;
            lv[i] = i < n ? vin[i] : ~0ull;
            lidx[i] = (uint32_t)i;
        }
        __syncthreads();
        const int64_t npairs = p2 >> 1;
        for (int64_t kk = 2; kk <= p2; kk <<= 1) {
            for (int64_t jj = kk >> 1, s = 63 - __clzll(kk >> 1); jj > 0;
                 jj >>= 1, s--) {
                for (int64_t p = tid; p < npairs; p += FUSE_THREADS) {
                    const int64_t i = ((p >> s) << (s + 1)) | (p & (jj - 1));
                    const int64_t l = i + jj;
                    const bool up = (i & kk) == 0;
                    const uint64_t ka = lk[i], kb = lk[l];
                    const uint64_t va = lv[i], vb = lv[l];
                    const uint32_t ia = lidx[i], ib = lidx[l];
                    const bool gt =
                        ka > kb ||
                        (ka == kb && (va > vb || (va == vb && ia > ib)));
                    if (gt == up) {
                        lk[i] = kb; lk[l] = ka;
                        lv[i] = vb; lv[l] = va;
                        lidx[i] = ib; lidx[l] = ia;
                    }
                }
                __syncthreads();
            }
        }
        for (int64_t i = tid; i < n; i += FUSE_THREADS) src[i] = lidx[i];
        __syncthreads();
    } else {
    // ---- significant bits of (max-min) for k and v ----
    if (tid == 0) {
        smax[0] = 0; smax[1] = 0;
        smin[0] = ~0ull; smin[1] = ~0ull;
    }
    __syncthreads();
    {
        uint64_t mk = 0, mv = 0, nk = ~0ull, nv = ~0ull;
        for (int64_t i = tid; i < n; i += FUSE_THREADS) {
            mk = max(mk, kin[i]);
            mv = max(mv, vin[i]);
            nk = min(nk, kin[i]);
            nv = min(nv, vin[i]);
        }
        atomicMax((unsigned long long *)&smax[0], (unsigned long long)mk);
        atomicMax((unsigned long long *)&smax[1], (unsigned long long)mv);
        atomicMin((unsigned long long *)&smin[0], (unsigned long long)nk);
        atomicMin((unsigned long long *)&smin[1], (unsigned long long)nv);
    }
    __syncthreads();
    const uint64_t kbase = smin[0], vbase = smin[1];
    const uint64_t krange = smax[0] - kbase, vrange = smax[1] - vbase;
    int knibs = 0, vnibs = 0;
    while (knibs < 16 && (krange >> (4 * knibs)) != 0) knibs++;
    while (vnibs < 16 && (vrange >> (4 * vnibs)) != 0) vnibs++;
    const int total_nibs = vnibs + knibs;
    const int vbits = 4 * vnibs;

    // bits [s, s+16) of the concatenated key ((k-kbase) << vbits | (v-vbase))
    auto key16_at = [&](uint32_t idx, int s) -> uint32_t {
        const uint64_t vp = vin[idx] - vbase;
        const uint64_t kp = kin[idx] - kbase;
        uint64_t bits = 0;
        if (s < vbits) {
            bits = vp >> s;
            const int up = vbits - s;
            if (up < 64) bits |= kp << up;
        } else {
            bits = kp >> (s - vbits);
        }
        return (uint32_t)(bits & 0xFFFF);
    };

    // ---- digit passes in groups of 4 sharing one entry packing ----
    for (int base = 0; base < total_nibs; base += 4) {
        // (re)pack: entry = next-16-key-bits << 13 | idx  (one global gather)
        for (int64_t i = tid; i < n; i += FUSE_THREADS) {
            const uint32_t idx =
                base == 0 ? (uint32_t)i : (src[i] & 0x1FFFu);
            src[i] = (key16_at(idx, 4 * base) << 13) | idx;
        }
        __syncthreads();
        const int sub_max = min(4, total_nibs - base);
        for (int sub = 0; sub < sub_max; sub++) {
            const int sh = 13 + 4 * sub;
            const int cells_n = FUSE_DIGITS * rounds * nwaves;
            for (int c = tid; c < cells_n; c += FUSE_THREADS) cnt[c] = 0;
            __syncthreads();
            uint32_t myrank[FUSE_ITEMS];
            uint32_t mydig[FUSE_ITEMS];
#pragma unroll
            for (int j = 0; j < FUSE_ITEMS; j++) {
                if (j >= rounds) break;
                const int64_t i = (int64_t)j * FUSE_THREADS + tid;
                const bool act = i < n;
                const uint32_t e = act ? src[i] : 0;
                const uint32_t d = (e >> sh) & 0xF;
                const uint64_t am = __ballot(act);
                const uint64_t b0 = __ballot(d & 1);
                const uint64_t b1 = __ballot(d & 2);
                const uint64_t b2 = __ballot(d & 4);
                const uint64_t b3 = __ballot(d & 8);
                uint64_t m = am;
                m &= (d & 1) ? b0 : ~b0;
                m &= (d & 2) ? b1 : ~b1;
                m &= (d & 4) ? b2 : ~b2;
                m &= (d & 8) ? b3 : ~b3;
                myrank[j] = (uint32_t)__popcll(m & lt);
                mydig[j] = d;
                if (act && (m & lt) == 0)  // lowest lane of this digit group
                    cnt[(d * rounds + j) * nwaves + wid] =
                        (uint32_t)__popcll(m);
                if (!act) myrank[j] = 0xFFFFFFFFu;
            }
            __syncthreads();
            {   // exclusive scan of the (digit, round, wave) cells
                uint32_t local[2];
                const int cpt = (cells_n + FUSE_THREADS - 1) / FUSE_THREADS;
                uint32_t tsum = 0;
                for (int j = 0; j < cpt; j++) {
                    const int f = tid * cpt + j;
                    local[j] = f < cells_n ? cnt[f] : 0;
                    tsum += local[j];
                }
                uint32_t total_unused;
                uint32_t off = fuse_scan(tsum, wave_tot, &total_unused);
                for (int j = 0; j < cpt; j++) {
                    const int f = tid * cpt + j;
                    if (f < cells_n) cnt[f] = off;
                    off += local[j];
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < FUSE_ITEMS; j++) {
                if (j >= rounds) break;
                const int64_t i = (int64_t)j * FUSE_THREADS + tid;
                if (i < n) {
                    const uint32_t r =
                        cnt[(mydig[j] * rounds + j) * nwaves + wid] +
                        myrank[j];
                    dst[r] = src[i];
                }
            }
            __syncthreads();
            uint32_t *t = src; src = dst; dst = t;
        }
    }

    if (total_nibs == 0) {  // all rows share one (k,v): identity entries
        for (int64_t i = tid; i < n; i += FUSE_THREADS) src[i] = (uint32_t)i;
        __syncthreads();
    }
    }  // end radix path

    // ---- consolidate: head flags (full-key compares via one gather) ----
    // seg ids into dst (the free buffer); ballot cells per (round, wave)
    uint32_t headmask[FUSE_ITEMS];  // per round: this wave's head ballot
    uint32_t myhead[FUSE_ITEMS];
    {
        const int cells_n = rounds * nwaves;
        for (int c = tid; c < cells_n; c += FUSE_THREADS) cnt[c] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FUSE_ITEMS; j++) {
            if (j >= rounds) break;
            const int64_t i = (int64_t)j * FUSE_THREADS + tid;
            uint32_t h = 0;
            if (i < n) {
                const uint32_t idx = src[i] & 0x1FFFu;
                if (i == 0) h = 1;
                else {
                    const uint32_t pidx = src[i - 1] & 0x1FFFu;
                    h = (kin[idx] != kin[pidx]) || (vin[idx] != vin[pidx]);
                }
            }
            myhead[j] = h;
            const uint64_t m = __ballot(h != 0);
            headmask[j] = (uint32_t)__popcll(m & lt);  // rank among heads
            if (i < n && lane == 0)
                cnt[j * nwaves + wid] = (uint32_t)__popcll(m);
        }
        __syncthreads();
    }
    uint32_t nseg;
    {   // scan head cells
        const int cells_n = rounds * nwaves;
        uint32_t local[1];
        uint32_t tsum = 0;
        if (tid < cells_n) {
            local[0] = cnt[tid];
            tsum = local[0];
        }
        uint32_t off = fuse_scan(tsum, wave_tot, &nseg);
        if (tid < cells_n) cnt[tid] = off;
        __syncthreads();
    }
    // seg of row i = heads at-or-before i, minus 1
#pragma unroll
    for (int j = 0; j < FUSE_ITEMS; j++) {
        if (j >= rounds) break;
        const int64_t i = (int64_t)j * FUSE_THREADS + tid;
        if (i < n)
            dst[i] = cnt[j * nwaves + wid] + headmask[j] + myhead[j] - 1;
    }
    __syncthreads();
    if constexpr (sizeof(W) == 8 && (W)0.5 == (W)0) {  // integer weights
        for (uint32_t i = tid; i < nseg; i += FUSE_THREADS) tw[i] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FUSE_ITEMS; j++) {
            if (j >= rounds) break;
            const int64_t i = (int64_t)j * FUSE_THREADS + tid;
            if (i < n) {
                const uint32_t idx = src[i] & 0x1FFFu;
                const uint32_t seg = dst[i];
                atomicAdd((unsigned long long *)&tw[seg],
                          (unsigned long long)win[idx]);
                if (myhead[j]) {
                    tk[seg] = kin[idx];
                    tv[seg] = vin[idx];
                }
            }
        }
        __syncthreads();
    } else {
        // f64: deterministic segmented tree sum in sorted-position order
        // (identical order to the stable sort's positions, so results are
        // bit-equal to the previous per-thread-counter kernel).  cnt (8192
        // cells) now holds each segment's head position.
#pragma unroll
        for (int j = 0; j < FUSE_ITEMS; j++) {
            if (j >= rounds) break;
            const int64_t i = (int64_t)j * FUSE_THREADS + tid;
            if (i < n) {
                const uint32_t idx = src[i] & 0x1FFFu;
                tw[i] = win[idx];
                if (myhead[j]) {
                    const uint32_t seg = dst[i];
                    cnt[seg] = (uint32_t)i;
                    tk[seg] = kin[idx];
                    tv[seg] = vin[idx];
                }
            }
        }
        __syncthreads();
        for (int64_t d = 1; d < n; d <<= 1) {
#pragma unroll
            for (int j = 0; j < FUSE_ITEMS; j++) {
                if (j >= rounds) break;
                const int64_t i = (int64_t)j * FUSE_THREADS + tid;
                if (i < n && i + d < n && dst[i] == dst[i + d]) {
                    const uint32_t rel = (uint32_t)i - cnt[dst[i]];
                    if ((rel & (2 * d - 1)) == 0) tw[i] += tw[i + d];
                }
            }
            __syncthreads();
        }
        W my_tot[FUSE_ITEMS];
#pragma unroll
        for (int j = 0; j < FUSE_ITEMS; j++) {
            if (j >= rounds) break;
            const int64_t i = (int64_t)j * FUSE_THREADS + tid;
            my_tot[j] = (i < n && myhead[j]) ? tw[i] : (W)0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FUSE_ITEMS; j++) {
            if (j >= rounds) break;
            const int64_t i = (int64_t)j * FUSE_THREADS + tid;
            if (i < n && myhead[j]) tw[dst[i]] = my_tot[j];
        }
        __syncthreads();
    }
    // ---- drop zero-weight segments (ballot compaction over seg ids) ----
    {
        const int seg_rounds = (int)((nseg + FUSE_THREADS - 1) / FUSE_THREADS);
        const int cells_n = seg_rounds * nwaves;
        for (int c = tid; c < cells_n + 1; c += FUSE_THREADS) cnt[c] = 0;
        __syncthreads();
        uint32_t nzrank[FUSE_ITEMS];
        uint32_t mynz[FUSE_ITEMS];
#pragma unroll
        for (int j = 0; j < FUSE_ITEMS; j++) {
            if (j >= seg_rounds) break;
            const uint32_t i = (uint32_t)j * FUSE_THREADS + tid;
            const uint32_t nz = (i < nseg && tw[i] != (W)0) ? 1 : 0;
            mynz[j] = nz;
            const uint64_t m = __ballot(nz != 0);
            nzrank[j] = (uint32_t)__popcll(m & lt);
            if (i < nseg && lane == 0)
                cnt[j * nwaves + wid] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        uint32_t nout;
        {
            uint32_t local = 0;
            if (tid < cells_n) local = cnt[tid];
            uint32_t off = fuse_scan(local, wave_tot, &nout);
            if (tid < cells_n) cnt[tid] = off;
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < FUSE_ITEMS; j++) {
            if (j >= seg_rounds) break;
            const uint32_t i = (uint32_t)j * FUSE_THREADS + tid;
            if (i < nseg && mynz[j]) {
                const uint32_t p = cnt[j * nwaves + wid] + nzrank[j];
                ok[p] = tk[i];
                ov[p] = tv[i];
                ow[p] = tw[i];
            }
        }
        if (tid == 0) *out_len = (int64_t)nout;
    }
}

template <typename W>
__global__ __launch_bounds__(FUSE_THREADS, 4) void k_sort_cons_small(SortArgs args) {
    // one raw batch per workgroup through sort_cons_body
    const int batch = blockIdx.x;
    int64_t n = args.n[batch];
    int64_t *out_len = args.d_len + batch;
    SORT_CONS_LDS
    if (args.n_take[batch]) {
        // take the producer's counter: one thread reads it, records it in
        // the readback slot and hands the counter back zeroed; the block
        // learns the length through LDS, so no thread can read the zero
        __shared__ int64_t s_take;
        if (threadIdx.x == 0) {
            const int64_t seen = *args.n_take[batch];
            s_take = seen;
            *args.n_seen[batch] = seen;
            *args.n_take[batch] = 0;
        }
        __syncthreads();
        const int64_t n_take = s_take;
        if (n_take > FUSE_MAX || n_take < 0 || n_take > args.n_cap[batch]) {
            if (threadIdx.x == 0) *out_len = -1;  // speculation lost
            return;
        }
        n = n_take;
    } else if (args.n_dev[batch]) {
        const int64_t n_chain = *args.n_dev[batch];
        if (n_chain > FUSE_MAX || n_chain < 0) {  // speculation lost
            if (threadIdx.x == 0) *out_len = -1;
            return;
        }
        n = n_chain;
    }
    sort_cons_body<W>(args.kin[batch], args.vin[batch],
                      (const W *)args.win[batch], n, args.tk[batch],
                      args.tv[batch], (W *)args.tw[batch], args.ok[batch],
                      args.ov[batch], (W *)args.ow[batch], out_len, bufA, bufB,
                      cnt, wave_tot, smax, smin);
}

// ---------------------------------------------------------------------------
// dense-range sort+consolidate.  A Nexmark tick's delta usually has a TINY
// key box: q5 bids cover ~4-8 distinct ms timestamps x the ~100-auction
// in-flight window (generator/auctions.rs:112-123), so instead of sorting
// 37k rows we scatter weights into a (krange+1)*(vrange+1) histogram with
// many blocks and emit the nonzero cells in index order — already sorted and
// consolidated.  Integer weights only (atomic accumulation).
// ---------------------------------------------------------------------------

__global__ void k_minmax_rows(const uint64_t *k, const uint64_t *v, int64_t n,
                              unsigned long long *mm /* kmin,vmin,kmax,vmax */,
                              const int64_t *n_dev = nullptr) {
    if (n_dev) n = *n_dev;
    uint64_t mk = 0, mv = 0, nk = ~0ull, nv = ~0ull;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        mk = max(mk, k[i]);
        mv = max(mv, v[i]);
        nk = min(nk, k[i]);
        nv = min(nv, v[i]);
    }
    __shared__ unsigned long long s[4];
    if (threadIdx.x == 0) { s[0] = ~0ull; s[1] = ~0ull; s[2] = 0; s[3] = 0; }
    __syncthreads();
    atomicMin(&s[0], (unsigned long long)nk);
    atomicMin(&s[1], (unsigned long long)nv);
    atomicMax(&s[2], (unsigned long long)mk);
    atomicMax(&s[3], (unsigned long long)mv);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&mm[0], s[0]);
        atomicMin(&mm[1], s[1]);
        atomicMax(&mm[2], s[2]);
        atomicMax(&mm[3], s[3]);
    }
}

__global__ void k_hist_add(const uint64_t *k, const uint64_t *v,
                           const int64_t *w, int64_t n, uint64_t kbase,
                           uint64_t vbase, uint64_t vspan,
                           unsigned long long *wbuf) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&wbuf[(k[i] - kbase) * vspan + (v[i] - vbase)],
                  (unsigned long long)w[i]);
}

__global__ void k_hist_flags(const unsigned long long *wbuf, int64_t r,
                             uint64_t *flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < r;
         i += (int64_t)gridDim.x * blockDim.x)
        flags[i] = wbuf[i] != 0;
}

__global__ void k_hist_total(const unsigned long long *wbuf,
                             const uint64_t *flag_scan, int64_t r,
                             int64_t *out) {
    *out = (int64_t)(flag_scan[r - 1] + (wbuf[r - 1] != 0 ? 1 : 0));
}

__global__ void k_hist_emit(const unsigned long long *wbuf,
                            const uint64_t *flag_scan, int64_t r,
                            uint64_t kbase, uint64_t vbase, uint64_t vspan,
                            uint64_t *ok, uint64_t *ov, int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < r;
         i += (int64_t)gridDim.x * blockDim.x) {
        unsigned long long wv = wbuf[i];
        if (wv != 0) {
            uint64_t p = flag_scan[i];
            ok[p] = kbase + (uint64_t)i / vspan;
            ov[p] = vbase + (uint64_t)i % vspan;
            ow[p] = (int64_t)wv;
        }
    }
}

// ---------------------------------------------------------------------------
// consolidate sorted rows: head flags -> scan -> segment-sum -> nonzero compact
// ---------------------------------------------------------------------------

__global__ void k_head_flags(const uint64_t *k, const uint64_t *v, int64_t n,
                             uint64_t *flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        flags[i] = (i == 0) || k[i] != k[i - 1] || v[i] != v[i - 1];
}

// seg[i] implied by scanned flags; accumulate weights and write unique (k,v)
__global__ void k_seg_accum(const uint64_t *k, const uint64_t *v,
                            const int64_t *w, const uint64_t *flag_scan,
                            const uint64_t *flags, int64_t n, uint64_t *ok,
                            uint64_t *ov, int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t seg = flags[i] ? flag_scan[i] : flag_scan[i] - 1;
        atomicAdd((unsigned long long *)&ow[seg], (unsigned long long)w[i]);
        if (flags[i]) {
            ok[seg] = k[i];
            ov[seg] = v[i];
        }
    }
}

// f64 big-path consolidate support: deterministic segmented tree sum over the
// sorted weight array (fixed position order; |err| <= 2 ulp * ceil(log2 run)).
__device__ inline uint64_t seg_of(const uint64_t *fscan, const uint64_t *flags,
                                  int64_t i) {
    return flags[i] ? fscan[i] : fscan[i] - 1;
}

__global__ void k_seg_headpos(const uint64_t *flags, const uint64_t *fscan,
                              int64_t n, uint64_t *hp) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        if (flags[i]) hp[fscan[i]] = (uint64_t)i;
}

__global__ void k_seg_tree_round(double *w, const uint64_t *flags,
                                 const uint64_t *fscan, const uint64_t *hp,
                                 int64_t n, int64_t d) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (i + d < n) {
            uint64_t sg = seg_of(fscan, flags, i);
            if (sg == seg_of(fscan, flags, i + d) &&
                (((uint64_t)i - hp[sg]) & (uint64_t)(2 * d - 1)) == 0)
                w[i] += w[i + d];
        }
    }
}

__global__ void k_seg_collect_f64(const uint64_t *k, const uint64_t *v,
                                  const double *w, const uint64_t *flags,
                                  const uint64_t *fscan, int64_t n,
                                  uint64_t *ok, uint64_t *ov, double *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (flags[i]) {
            uint64_t sg = fscan[i];
            ok[sg] = k[i];
            ov[sg] = v[i];
            ow[sg] = w[i];  // tree total sits at the head position
        }
    }
}

template <typename W>
__global__ void k_nonzero_flags(const W *w, int64_t n, uint64_t *flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        flags[i] = w[i] != W(0);  // f64: -0.0 compares equal to 0.0: dropped
}

__global__ void k_compact(const uint64_t *k, const uint64_t *v, const int64_t *w,
                          const uint64_t *flags, const uint64_t *flag_scan,
                          int64_t n, uint64_t *ok, uint64_t *ov, int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (flags[i]) {
            uint64_t pos = flag_scan[i];
            ok[pos] = k[i];
            ov[pos] = v[i];
            ow[pos] = w[i];
        }
    }
}

// distinct keys of a sorted batch: the key-only head flags and compact
__global__ void k_key_head_flags(const uint64_t *k, int64_t n, uint64_t *flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        flags[i] = (i == 0) || k[i] != k[i - 1];
}

__global__ void k_compact_keys(const uint64_t *k, const uint64_t *flags,
                               const uint64_t *fscan, int64_t n, uint64_t *ok) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        if (flags[i]) ok[fscan[i]] = k[i];
}

// ---------------------------------------------------------------------------
// merge-path merge of two consolidated batches
// (the trace-merge hot kernel; replaces push_merge/merge_step)
// ---------------------------------------------------------------------------

__device__ inline bool row_lt(uint64_t ak, uint64_t av, uint64_t bk, uint64_t bv) {
    return ak != bk ? ak < bk : av < bv;
}
__device__ inline bool row_eq(uint64_t ak, uint64_t av, uint64_t bk, uint64_t bv) {
    return ak == bk && av == bv;
}

// merge-path split: find (ai, bi), ai + bi = diag, such that
// a[0..ai) and b[0..bi) are exactly the first `diag` outputs
// (tie-break: a before b).
__device__ inline void merge_path(const uint64_t *ak, const uint64_t *av,
                                  int64_t na, const uint64_t *bk,
                                  const uint64_t *bv, int64_t nb, int64_t diag,
                                  int64_t &ai, int64_t &bi) {
    int64_t lo = max((int64_t)0, diag - nb);
    int64_t hi = min(diag, na);
    while (lo < hi) {
        int64_t mid = (lo + hi) / 2;         // candidate ai
        int64_t j = diag - mid - 1;          // b index to compare
        // a[mid] vs b[j]: if a[mid] <= b[j] (tie to a), we can take more a
        if (!row_lt(bk[j], bv[j], ak[mid], av[mid]))  // b[j] >= a[mid]
            lo = mid + 1;
        else
            hi = mid;
    }
    ai = lo;
    bi = diag - lo;
}

// adjust a split so an equal (k,v) pair is never separated: with a-before-b
// tie-breaking, the pair (a[ai-1], b[bi]) is the only possible split pair.
__device__ inline void adjust_split(const uint64_t *ak, const uint64_t *av,
                                    const uint64_t *bk, const uint64_t *bv,
                                    int64_t na, int64_t nb, int64_t &ai,
                                    int64_t &bi) {
    if (ai > 0 && bi < nb && row_eq(ak[ai - 1], av[ai - 1], bk[bi], bv[bi])) bi++;
}


// ---------------------------------------------------------------------------
// join: delta x trace with projection (count/emit)
// ---------------------------------------------------------------------------

__device__ inline int64_t lower_bound_k(const uint64_t *k, int64_t n,
                                        uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        int64_t mid = (lo + hi) / 2;
        if (k[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ inline int64_t upper_bound_k(const uint64_t *k, int64_t n,
                                        uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        int64_t mid = (lo + hi) / 2;
        if (k[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_join_count(const uint64_t *dk, int64_t nd, const uint64_t *tk,
                             int64_t nt, uint64_t *counts, uint64_t *starts) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nd;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t key = dk[i];
        int64_t lo = lower_bound_k(tk, nt, key);
        int64_t hi = lo;
        // galloping upper bound (advance.rs:11-60 analog): trace runs per key
        // are usually short; probe forward before a full binary search
        if (lo < nt && tk[lo] == key) {
            int64_t step = 1;
            hi = lo;
            while (hi + step < nt && tk[hi + step] == key) { hi += step; step <<= 1; }
            hi = upper_bound_k(tk + hi, min(step, nt - hi), key) + hi;
        }
        counts[i] = hi - lo;
        starts[i] = lo;
    }
}

// Returns whether the pair is a real match (join_func filters, e.g. q4's
// bid-validity window): an invalid pair still occupies its counted output
// slot but emits weight 0, which the tick's consolidate then drops.
__device__ inline bool proj_out(int proj, uint64_t param, uint64_t k,
                                uint64_t v1, uint64_t v2, uint64_t &hi,
                                uint64_t &lo) {
    switch (proj) {
        case DBSP_PROJ_Q4_BID_X_AUC: {
            // delta = bid (v1 = bid_dt<<27 | price), trace = auction
            // (v2 = a_dt<<28 | (expires-a_dt)<<4 | category-10); emit
            // ((auction<<4)|cat, price) when the bid falls in the auction's
            // validity window (q4.rs:58-68)
            const uint64_t bid_dt = v1 >> 27, price = v1 & 0x7FFFFFFull;
            const uint64_t a_dt = v2 >> 28, dur = (v2 >> 4) & 0xFFFFFFull;
            hi = (k << 4) | (v2 & 0xFull);
            lo = price;
            return bid_dt >= a_dt && bid_dt <= a_dt + dur;
        }
        case DBSP_PROJ_Q6_BID_X_AUC: {
            // q6.rs:60-80: delta = bid (v1 = bid_dt<<27|price), trace =
            // auction (v2 = a_dt<<36 | (expires-a_dt)<<20 | seller); emit
            // ((auction<<20)|seller, price) in the validity window
            const uint64_t bid_dt = v1 >> 27, price = v1 & 0x7FFFFFFull;
            const uint64_t a_dt = v2 >> 36, dur = (v2 >> 20) & 0xFFFFull;
            hi = (k << 20) | (v2 & 0xFFFFFull);
            lo = price;
            return bid_dt >= a_dt && bid_dt <= a_dt + dur;
        }
        case DBSP_PROJ_Q6_AUC_X_BID: {
            const uint64_t bid_dt = v2 >> 27, price = v2 & 0x7FFFFFFull;
            const uint64_t a_dt = v1 >> 36, dur = (v1 >> 20) & 0xFFFFull;
            hi = (k << 20) | (v1 & 0xFFFFFull);
            lo = price;
            return bid_dt >= a_dt && bid_dt <= a_dt + dur;
        }
        case DBSP_PROJ_Q4_AUC_X_BID: {  // sides swapped
            const uint64_t bid_dt = v2 >> 27, price = v2 & 0x7FFFFFFull;
            const uint64_t a_dt = v1 >> 28, dur = (v1 >> 4) & 0xFFFFFFull;
            hi = (k << 4) | (v1 & 0xFull);
            lo = price;
            return bid_dt >= a_dt && bid_dt <= a_dt + dur;
        }
        case DBSP_PROJ_HI_V2_LO_V1: hi = v2; lo = v1; break;
        case DBSP_PROJ_HI_V1_LO_V2: hi = v1; lo = v2; break;
        case DBSP_PROJ_HI_K_LO_V1V2: hi = k; lo = (v1 << 32) | (v2 & 0xFFFFFFFFull); break;
        case DBSP_PROJ_HI_K_LO_V1RND: {
            uint64_t dt = v1 & 0xFFFFFFFFull;
            hi = k; lo = (v1 & 0xFFFFFFFF00000000ull) | (dt - dt % param);
            break;
        }
        case DBSP_PROJ_HI_K_LO_V2RND: {
            uint64_t dt = v2 & 0xFFFFFFFFull;
            hi = k; lo = (v2 & 0xFFFFFFFF00000000ull) | (dt - dt % param);
            break;
        }
        case DBSP_PROJ_HI_V2_LO_K: hi = v2; lo = k; break;
        case DBSP_PROJ_HI_V1_LO_K: hi = v1; lo = k; break;
        case DBSP_PROJ_HI_K_LO_V2V1: hi = k; lo = (v2 << 32) | (v1 & 0xFFFFFFFFull); break;
        case DBSP_PROJ_HI_K_LO_V2: hi = k; lo = v2; break;
        default: hi = 0; lo = 0; break;
    }
    return true;
}

// emit over the OUTPUT index space: balanced regardless of per-key skew
// (hot-seller keys have thousands of matches; one-thread-per-delta-row would
// serialize them)
__global__ void k_join_emit(const uint64_t *dk, const uint64_t *dv,
                            const int64_t *dw, int64_t nd, const uint64_t *tv,
                            const int64_t *tw, const uint64_t *offsets,
                            const uint64_t *starts, int64_t n_out, int proj,
                            uint64_t param, uint64_t *ok, uint64_t *ov,
                            int64_t *ow) {
    for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < n_out;
         o += (int64_t)gridDim.x * blockDim.x) {
        // find delta row: offsets is the exclusive scan of counts (length nd)
        int64_t lo = 0, hi = nd;
        while (lo < hi) {  // upper_bound(offsets, o) - 1
            int64_t mid = (lo + hi) / 2;
            if (offsets[mid] <= (uint64_t)o) lo = mid + 1; else hi = mid;
        }
        int64_t i = lo - 1;
        int64_t j = o - (int64_t)offsets[i];
        int64_t t = (int64_t)starts[i] + j;
        uint64_t hi_o, lo_o;
        const bool valid = proj_out(proj, param, dk[i], dv[i], tv[t], hi_o, lo_o);
        ok[o] = hi_o;
        ov[o] = lo_o;
        ow[o] = valid ? dw[i] * tw[t] : 0;
    }
}

// ---------------------------------------------------------------------------
// large-merge path (the HBM roofline kernel): per-BLOCK merge-path partition
// (one global binary search per 4096-row tile, not per thread), then
// LDS-staged count and emit passes — coalesced HBM streams in, per-thread
// merge walks entirely in LDS.  Replaces the naive per-thread global
// partitioning, which at 1B rows spent its time on ~14G random 8B probes
// (measured 53 GB/s).
// ---------------------------------------------------------------------------

#define MP_TILE 1024
#define MP_TILE_OP 2048  // single-pass lookback: wider tiles than the two-pass shorten the chain
#define MP_THREADS 256
#define MP_ITEMS (MP_TILE / MP_THREADS)  // 16 diagonals per thread

__global__ void k_mp_partition(const uint64_t *ak, const uint64_t *av,
                               int64_t na, const uint64_t *bk,
                               const uint64_t *bv, int64_t nb, int64_t nblocks,
                               int64_t tile, int64_t *pa, int64_t *pb) {
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i > nblocks) return;
    int64_t d = min(i * tile, na + nb);
    int64_t ai, bi;
    merge_path(ak, av, na, bk, bv, nb, d, ai, bi);
    adjust_split(ak, av, bk, bv, na, nb, ai, bi);
    pa[i] = ai;
    pb[i] = bi;
}

// local merge-path over the LDS-staged tile (a rows at [0,naL), b rows at
// [naL, naL+nbL) of the lk/lv arrays)
__device__ inline void merge_path_lds(const uint64_t *lk, const uint64_t *lv,
                                      int64_t naL, int64_t nbL, int64_t diag,
                                      int64_t &ai, int64_t &bi) {
    int64_t lo = max((int64_t)0, diag - nbL);
    int64_t hi = min(diag, naL);
    while (lo < hi) {
        int64_t mid = (lo + hi) / 2;
        int64_t j = naL + diag - mid - 1;
        if (!row_lt(lk[j], lv[j], lk[mid], lv[mid])) lo = mid + 1;
        else hi = mid;
    }
    ai = lo;
    bi = diag - lo;
}

__device__ inline void adjust_split_lds(const uint64_t *lk, const uint64_t *lv,
                                        int64_t naL, int64_t nbL, int64_t &ai,
                                        int64_t &bi) {
    if (ai > 0 && bi < nbL &&
        row_eq(lk[ai - 1], lv[ai - 1], lk[naL + bi], lv[naL + bi]))
        bi++;
}


// ---------------------------------------------------------------------------
// single-pass large merge: decoupled-lookback offsets replace the
// count->scan->emit pipeline (removes the 16 B/row count re-read, the device
// scan, and the mid-pipeline host sync).  Blocks take a ticket (atomic) so
// virtual block order equals launch order (forward progress for lookback);
// per-block state is one 8-byte {flag,value} granule written/read with
// agent-scope relaxed atomics (single-granule R2 form of the CDNA4
// inter-workgroup recipe — no fences needed for an 8-byte payload-is-flag).
// State layout: state[0] = ticket; state[1+vb] = granule
//   granule = value<<2 | flag;  flag: 0 invalid, 1 aggregate, 2 prefix
// ---------------------------------------------------------------------------


// stage `n` rows of (k,v[,w]) into LDS at base `off`: pairs of u64 move as
// ulonglong2 when both sides are 16 B aligned; odd head/tail go scalar
template <bool EMIT, typename W>
__device__ inline void stage_run(uint64_t *lk, uint64_t *lv, W *lw,
                                 int64_t off, const uint64_t *gk,
                                 const uint64_t *gv, const W *gw, int64_t n,
                                 int tid) {
    // align the GLOBAL side to 16 B (columns share base alignment, so one
    // parity covers k, v and w)
    const int64_t head = ((uintptr_t)gk & 15) != 0 ? 1 : 0;
    if (head && n > 0 && tid == 0) {
        lk[off] = gk[0];
        lv[off] = gv[0];
        if (EMIT) lw[off] = gw[0];
    }
    const int64_t pairs = n > head ? (n - head) >> 1 : 0;
    const ulonglong2 *gk2 = (const ulonglong2 *)(gk + head);
    const ulonglong2 *gv2 = (const ulonglong2 *)(gv + head);
    for (int64_t p = tid; p < pairs; p += MP_THREADS) {
        ulonglong2 kk = gk2[p];
        ulonglong2 vv = gv2[p];
        int64_t i = off + head + 2 * p;
        lk[i] = kk.x; lk[i + 1] = kk.y;
        lv[i] = vv.x; lv[i + 1] = vv.y;
    }
    if (EMIT) {
        const ulonglong2 *gw2 = (const ulonglong2 *)(gw + head);
        for (int64_t p = tid; p < pairs; p += MP_THREADS) {
            ulonglong2 ww = gw2[p];
            int64_t i = off + head + 2 * p;
            lw[i] = ((const W *)&ww)[0];
            lw[i + 1] = ((const W *)&ww)[1];
        }
    }
    const int64_t tail = head + 2 * pairs;
    if (tail < n && tid == 0) {
        lk[off + tail] = gk[tail];
        lv[off + tail] = gv[tail];
        if (EMIT) lw[off + tail] = gw[tail];
    }
}

typedef __attribute__((address_space(1))) unsigned long long gu64_t;

// ---------------------------------------------------------------------------
// single-pass merge v2.  One FUSED branchless walk per tile (the round-1
// variant walked the tile twice: once to count, once to emit); the walk
// captures per-step decisions (advance-a / equal-pair / keep) as mask bits in
// one register and the emit replays them with pure LDS reads — no compares.
// The decoupled lookback runs WAVE-wide: all 64 lanes of wave 0 load a
// 64-entry predecessor window per round instead of lane 0 walking the chain
// serially (the round-1 chain at ~1M tiles was the measured bottleneck of
// the one-pass variant).  Tile = MP_TILE (1024) -> 24.6 KB LDS -> 6
// blocks/CU, matching the two-pass emit's occupancy.
// State layout: state[0] = ticket; state[1] = poison; state[2+vb] = granule
//   granule = value<<2 | flag;  flag: 0 invalid, 1 aggregate, 2 prefix
// ---------------------------------------------------------------------------

// One merge-tile kernel, three offset modes (MODE):
//   0  single-pass: decoupled-lookback prefix (state = ticket/poison/granules)
//   1  count phase: write the tile's output count to state[vb], no emit
//   2  emit phase: read the tile's pre-scanned output offset from state[vb]
// Modes 1+2 form the default two-pass pipeline (count -> device scan ->
// emit); mode 0 reads each input byte once but its lookback protocol costs
// more than the count re-read at 1B-row scale (measured: granule-load
// throughput-bound — wider windows and preloading both made it slower).
template <typename W, int TILE, int MODE>
__global__ __launch_bounds__(MP_THREADS, 4) void k_mp_merge_onepass(
    const uint64_t *ak, const uint64_t *av, const W *aw, int64_t na,
    const uint64_t *bk, const uint64_t *bv, const W *bw, int64_t nb,
    const int64_t *pa, const int64_t *pb, unsigned long long *state,
    int64_t nblocks, uint64_t *ok, uint64_t *ov, W *ow) {
    // steps per thread: a split adjustment can grow a tile one row past TILE
    constexpr int OP_ITEMS = (TILE + MP_THREADS) / MP_THREADS;
    constexpr bool STAGE_W = MODE != 1;  // count phase: weights only on eq
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t *lk = (uint64_t *)smem;
    uint64_t *lv = lk + (TILE + 2);
    W *lw = (W *)(lv + (TILE + 2));
    __shared__ uint32_t wt[MP_THREADS / WAVE + 1];
    __shared__ unsigned long long sh_vb;
    __shared__ unsigned long long sh_prefix;
    const int tid = threadIdx.x;
    if (MODE == 0) {
        // ticket: virtual block id in launch order (lookback progress)
        if (tid == 0) sh_vb = atomicAdd(state, 1ull);
        __syncthreads();
    } else if (tid == 0) {
        sh_vb = (unsigned long long)blockIdx.x;
    }
    if (MODE != 0) __syncthreads();
    const int64_t vb = (int64_t)sh_vb;
    const int64_t pa0 = pa[vb], pa1 = pa[vb + 1];
    const int64_t pb0 = pb[vb], pb1 = pb[vb + 1];
    const int naL = (int)(pa1 - pa0), nbL = (int)(pb1 - pb0);
    const int totL = naL + nbL;
    stage_run<STAGE_W>(lk, lv, lw, 0, ak + pa0, av + pa0, aw + pa0, naL, tid);
    stage_run<STAGE_W>(lk, lv, lw, naL, bk + pb0, bv + pb0, bw + pb0, nbL,
                       tid);
    __syncthreads();
    const int items = (totL + MP_THREADS - 1) / MP_THREADS;
    const int d0 = min(tid * items, totL);
    const int d1 = min(d0 + items, totL);
    int64_t ai64, bi64, ae64, be64;
    merge_path_lds(lk, lv, naL, nbL, d0, ai64, bi64);
    adjust_split_lds(lk, lv, naL, nbL, ai64, bi64);
    merge_path_lds(lk, lv, naL, nbL, d1, ae64, be64);
    adjust_split_lds(lk, lv, naL, nbL, ae64, be64);
    const int ai = (int)ai64, bi = (int)bi64, ae = (int)ae64, be = (int)be64;
    // fused walk: predicated (no branches), OUTPUT ROWS captured in
    // registers (OP_ITEMS x 3 VGPR pairs) so the emit below is pure stores —
    // no second index-walk, no re-compares, no replay LDS reads.
    // Steps needed <= items: the range can hold items+1 input rows only when
    // the d1 split adjustment pulled in the b half of an equal pair, and that
    // pair is consumed in one step.
    // register capture fits the VGPR budget only at the small tile (5 steps
    // = 30 capture VGPRs); the 2048 tile (9 steps) spills and keeps the
    // decision-mask + replay form instead
    constexpr bool CAPTURE = MODE != 1 && OP_ITEMS <= 5;
    uint32_t m_take = 0, m_eq = 0, m_keep = 0;
    uint32_t cnt = 0;
    uint64_t cap_k[CAPTURE ? OP_ITEMS : 1], cap_v[CAPTURE ? OP_ITEMS : 1];
    W cap_w[CAPTURE ? OP_ITEMS : 1];
    {
        int i = ai, j = bi;
#pragma unroll
        for (int t = 0; t < OP_ITEMS; t++) {
            const bool a_ok = i < ae, b_ok = j < be;
            const bool act = a_ok | b_ok;
            // all indices stay inside the tile+2 LDS arrays even when a side
            // is exhausted (i <= naL, naL + j <= totL <= MP_TILE + 1)
            const uint64_t ka = lk[i], va = lv[i];
            const uint64_t kb = lk[naL + j], vB = lv[naL + j];
            const bool eq = a_ok & b_ok & row_eq(ka, va, kb, vB);
            const bool take_a = a_ok & ((!b_ok) | row_lt(ka, va, kb, vB) | eq);
            W sum;
            if (MODE == 1) {
                // count phase stages no weights: read both sides only at an
                // equal pair (rare; the cancellation test needs the sum)
                sum = (W)0;
                if (eq) sum = (W)(aw[pa0 + i] + bw[pb0 + j]);
            } else {
                const W wa = lw[i], wb2 = lw[naL + j];
                sum = eq ? (W)(wa + wb2) : (take_a ? wa : wb2);
            }
            const bool keep = act & ((!eq) | (sum != (W)0));
            if (CAPTURE) {
                cap_k[CAPTURE ? t : 0] = take_a ? ka : kb;
                cap_v[CAPTURE ? t : 0] = take_a ? va : vB;
                cap_w[CAPTURE ? t : 0] = sum;
            } else if (MODE != 1) {
                m_take |= (uint32_t)take_a << t;
                m_eq |= (uint32_t)eq << t;
            }
            m_keep |= (uint32_t)(keep & act) << t;
            cnt += keep & act;
            i += (int)(act & (take_a | eq));
            j += (int)(act & ((!take_a) | eq));
        }
    }
    // block-exclusive scan of thread counts
    uint32_t thread_off;
    uint32_t block_cnt;
    {
        uint32_t v = cnt;
        for (int d = 1; d < WAVE; d <<= 1) {
            uint32_t up = __shfl_up(v, d, WAVE);
            if ((tid & (WAVE - 1)) >= d) v += up;
        }
        if ((tid & (WAVE - 1)) == WAVE - 1) wt[tid / WAVE] = v;
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0;
            for (int w = 0; w < MP_THREADS / WAVE; w++) {
                uint32_t t = wt[w];
                wt[w] = acc;
                acc += t;
            }
            wt[MP_THREADS / WAVE] = acc;
        }
        __syncthreads();
        thread_off = wt[tid / WAVE] + (v - cnt);
        block_cnt = wt[MP_THREADS / WAVE];
    }
    if (MODE == 1) {
        // count phase: publish the tile's count, nothing else to do
        if (tid == 0) state[vb] = (unsigned long long)block_cnt;
        return;
    }
    if (MODE == 2) {
        // emit phase: the device scan already turned counts into offsets
        if (tid == 0) sh_prefix = state[vb];
    } else if (tid < WAVE) {
        gu64_t *g = (gu64_t *)(state + 2);
        if (tid == 0)
            __hip_atomic_store(&g[vb],
                               ((unsigned long long)block_cnt << 2) | 1ull,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // Flat wave-window lookback (64 granules/round).  Measured notes:
        // preloading 8 rounds of granules ahead (one round-trip for 512) and
        // 256-granule windows both came out SLOWER — the protocol is bound
        // by total granule-load throughput against the small hot region, not
        // per-round latency — so the minimal-load sequential window wins.
        unsigned long long running = 0;
        unsigned spins = 0;
        bool done = (vb == 0);
        int64_t wbase = vb - WAVE;
        while (!done) {
            const int64_t p = wbase + tid;
            const unsigned long long e =
                p >= 0 ? __hip_atomic_load(&g[p], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT)
                       : 2ull;  // virtual predecessor: prefix 0
            const unsigned flag = (unsigned)(e & 3ull);
            const uint64_t pmask = __ballot(flag == 2u);
            const uint64_t imask = __ballot(flag == 0u);
            bool retry;
            if (pmask != 0) {
                const int hi = 63 - __clzll(pmask);  // newest prefix lane
                retry = ((imask >> hi) >> 1) != 0;   // invalid above it
                if (!retry) {
                    unsigned long long c = tid >= hi ? (e >> 2) : 0;
                    for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d, WAVE);
                    running += c;
                    done = true;
                }
            } else {
                retry = imask != 0;
                if (!retry) {
                    unsigned long long c = e >> 2;
                    for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d, WAVE);
                    running += c;
                    wbase -= WAVE;
                }
            }
            if (retry) {
                ++spins;
                if (spins < 8) __builtin_amdgcn_s_sleep(1);
                else __builtin_amdgcn_s_sleep(4);
                if (spins > (1u << 23)) {  // bounded spin: poison, don't hang
                    if (tid == 0)
                        __hip_atomic_store((gu64_t *)(state + 1), 1ull,
                                           __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    done = true;
                }
            }
        }
        if (tid == 0) {
            __hip_atomic_store(&g[vb],
                               ((running + block_cnt) << 2) | 2ull,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sh_prefix = running;
        }
    }
    __syncthreads();
    // emit: pure stores from the register capture (small tile), or replay of
    // the decision masks with LDS reads (large tile)
    uint64_t gpos = (uint64_t)sh_prefix + thread_off;
    if (CAPTURE) {
#pragma unroll
        for (int t = 0; t < OP_ITEMS; t++) {
            if ((m_keep >> t) & 1u) {
                ok[gpos] = cap_k[CAPTURE ? t : 0];
                ov[gpos] = cap_v[CAPTURE ? t : 0];
                ow[gpos] = cap_w[CAPTURE ? t : 0];
                gpos++;
            }
        }
    } else {
        int i = ai, j = bi;
#pragma unroll
        for (int t = 0; t < OP_ITEMS; t++) {
            const bool take_a = (m_take >> t) & 1u;
            const bool eq = (m_eq >> t) & 1u;
            const bool keep = (m_keep >> t) & 1u;
            const bool act = (i < ae) | (j < be);
            const int sel = take_a ? i : naL + j;
            if (keep) {
                ok[gpos] = lk[sel];
                ov[gpos] = lv[sel];
                ow[gpos] = eq ? (W)(lw[i] + lw[naL + j]) : lw[sel];
                gpos++;
            }
            i += (int)(act & (take_a | eq));
            j += (int)(act & ((!take_a) | eq));
        }
    }
}

// single-workgroup merge for small inputs (na+nb <= FUSE_MAX): merge-path
// thread diagonals + LDS scan; one launch, no host sync, length on device
template <typename W>
__global__ __launch_bounds__(FUSE_THREADS, 4) void k_merge_small(MergeArgs args) {
    __shared__ uint32_t wave_tot[FUSE_THREADS / WAVE + 1];
    const int p = blockIdx.x;
    const uint64_t *ak = args.ak[p], *av = args.av[p];
    const W *aw = (const W *)args.aw[p];
    const int64_t na = args.na[p];
    const uint64_t *bk = args.bk[p], *bv = args.bv[p];
    const W *bw = (const W *)args.bw[p];
    const int64_t nb = args.dnb[p] ? *args.dnb[p] : args.nb[p];
    uint64_t *ok = args.ok[p], *ov = args.ov[p];
    W *ow = (W *)args.ow[p];
    int64_t *out_len = args.d_len + p;
    const int tid = threadIdx.x;
    if (nb < 0 || na < 0) {  // failed upstream speculation: poison the length
        if (tid == 0) *out_len = -1;
        return;
    }
    const int64_t total = na + nb;
    const int64_t items = (total + FUSE_THREADS - 1) / FUSE_THREADS;
    int64_t d0 = min((int64_t)tid * items, total);
    int64_t d1 = min(d0 + items, total);
    int64_t ai, bi, ae, be;
    merge_path(ak, av, na, bk, bv, nb, d0, ai, bi);
    adjust_split(ak, av, bk, bv, na, nb, ai, bi);
    merge_path(ak, av, na, bk, bv, nb, d1, ae, be);
    adjust_split(ak, av, bk, bv, na, nb, ae, be);
    uint32_t cnt = 0;
    {
        int64_t i = ai, j = bi;
        while (i < ae || j < be) {
            if (i < ae && j < be && row_eq(ak[i], av[i], bk[j], bv[j])) {
                if (aw[i] + bw[j] != (W)0) cnt++;
                i++; j++;
            } else if (j >= be || (i < ae && row_lt(ak[i], av[i], bk[j], bv[j]))) {
                cnt++; i++;
            } else {
                cnt++; j++;
            }
        }
    }
    uint32_t tot_out;
    uint32_t off = fuse_scan(cnt, wave_tot, &tot_out);
    {
        int64_t i = ai, j = bi;
        while (i < ae || j < be) {
            if (i < ae && j < be && row_eq(ak[i], av[i], bk[j], bv[j])) {
                W s = aw[i] + bw[j];
                if (s != (W)0) { ok[off] = ak[i]; ov[off] = av[i]; ow[off] = s; off++; }
                i++; j++;
            } else if (j >= be || (i < ae && row_lt(ak[i], av[i], bk[j], bv[j]))) {
                ok[off] = ak[i]; ov[off] = av[i]; ow[off] = aw[i]; off++; i++;
            } else {
                ok[off] = bk[j]; ov[off] = bv[j]; ow[off] = bw[j]; off++; j++;
            }
        }
    }
    if (tid == 0) *out_len = (int64_t)tot_out;
}

// fixed-grid multi-workgroup merge with DEVICE-side b length (the in-train
// accumulator fold: the tick's delta length is only known on device).  Two
// phases over MERGE_MID_WGS workgroups per pair: count writes per-WG output
// counts to scratch; emit computes each WG's prefix from the tiny counts
// array (no separate scan launch) and writes its segment.  Equal (k, v)
// pairs never split across WGs (adjust_split), so per-segment consolidation
// is exact.
#define MERGE_MID_WGS 32
static_assert(MERGE_MID_SCRATCH == MERGE_MID_WGS + 1,
              "scratch layout mismatch with kernels_iface.hpp");

// One launch: count, one-shot cross-WG barrier, emit.  The grid is tiny
// (MERGE_MID_WGS x np <= 128 workgroups, all co-resident), so every WG
// publishes its count tagged with the launch generation and spins for its
// pair's 32 peers — a single barrier between uniform-work peers, NOT a
// serial lookback chain.  Each thread keeps its merge-path bounds in
// registers across the barrier, so the emit phase recomputes no split.
// Generation tags make the persistent scratch self-cleaning (no memset
// launch); a stale match would need a pair row untouched for exactly 2^32
// launches.
template <typename W>
__global__ __launch_bounds__(FUSE_THREADS, 4) void k_merge_mid_fused(
        MergeArgs args, int64_t *scratch, uint32_t gen) {
    const int p = blockIdx.y;
    const int wg = blockIdx.x;
    int64_t *cnt_row = scratch + (int64_t)p * (MERGE_MID_WGS + 1);
    int64_t *out_len = args.d_len + p;
    const int tid = threadIdx.x;
    const int64_t na = args.na[p];
    const int64_t nb = args.dnb[p] ? *args.dnb[p] : args.nb[p];
    if (na < 0 || nb < 0) {  // whole pair bails uniformly: no spin to feed
        if (tid == 0 && wg == 0) *out_len = -1;
        return;
    }
    const uint64_t *ak = args.ak[p], *av = args.av[p];
    const W *aw = (const W *)args.aw[p];
    const uint64_t *bk = args.bk[p], *bv = args.bv[p];
    const W *bw = (const W *)args.bw[p];
    uint64_t *ok = args.ok[p], *ov = args.ov[p];
    W *ow = (W *)args.ow[p];
    const int64_t total = na + nb;
    const int64_t per_wg = (total + MERGE_MID_WGS - 1) / MERGE_MID_WGS;
    const int64_t w0 = min((int64_t)wg * per_wg, total);
    const int64_t w1 = min(w0 + per_wg, total);
    const int64_t items = (w1 - w0 + FUSE_THREADS - 1) / FUSE_THREADS;
    int64_t d0 = min(w0 + (int64_t)tid * items, w1);
    int64_t d1 = min(d0 + items, w1);
    int64_t ai, bi, ae, be;
    merge_path(ak, av, na, bk, bv, nb, d0, ai, bi);
    adjust_split(ak, av, bk, bv, na, nb, ai, bi);
    merge_path(ak, av, na, bk, bv, nb, d1, ae, be);
    adjust_split(ak, av, bk, bv, na, nb, ae, be);
    uint32_t cnt = 0;
    {
        int64_t i = ai, j = bi;
        while (i < ae || j < be) {
            if (i < ae && j < be && row_eq(ak[i], av[i], bk[j], bv[j])) {
                if (aw[i] + bw[j] != (W)0) cnt++;
                i++; j++;
            } else if (j >= be || (i < ae && row_lt(ak[i], av[i], bk[j], bv[j]))) {
                cnt++; i++;
            } else {
                cnt++; j++;
            }
        }
    }
    __shared__ uint32_t wave_tot[FUSE_THREADS / WAVE + 1];
    uint32_t wg_tot;
    uint32_t off32 = fuse_scan(cnt, wave_tot, &wg_tot);
    if (tid == 0)
        atomicExch((unsigned long long *)&cnt_row[wg],
                   ((unsigned long long)gen << 32) | wg_tot);
    __shared__ int64_t s_cnt[MERGE_MID_WGS];
    __shared__ int s_dead;
    if (tid == 0) s_dead = 0;
    __syncthreads();
    if (tid < MERGE_MID_WGS) {
        // bounded spin: the grid is co-resident by construction, so this
        // resolves in ~kernel-uniform time; the bound turns a scheduling
        // assumption failure into a poisoned length (host fails loudly /
        // the train replays) instead of a wedged GPU
        unsigned long long v = 0;
        for (long spins = 0;; spins++) {
            v = atomicAdd((unsigned long long *)&cnt_row[tid], 0ull);
            if ((uint32_t)(v >> 32) == (uint32_t)gen) break;
            if (spins > (1l << 26)) { s_dead = 1; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        s_cnt[tid] = (int64_t)(uint32_t)v;
    }
    __syncthreads();
    if (s_dead) {
        if (tid == 0) *out_len = -1;
        return;
    }
    int64_t base = 0, all = 0;
    for (int g = 0; g < MERGE_MID_WGS; g++) {
        if (g < wg) base += s_cnt[g];
        all += s_cnt[g];
    }
    if (wg == 0 && tid == 0) *out_len = all;
    int64_t off = base + (int64_t)off32;
    {
        int64_t i = ai, j = bi;
        while (i < ae || j < be) {
            if (i < ae && j < be && row_eq(ak[i], av[i], bk[j], bv[j])) {
                W s = aw[i] + bw[j];
                if (s != (W)0) { ok[off] = ak[i]; ov[off] = av[i]; ow[off] = s; off++; }
                i++; j++;
            } else if (j >= be || (i < ae && row_lt(ak[i], av[i], bk[j], bv[j]))) {
                ok[off] = ak[i]; ov[off] = av[i]; ow[off] = aw[i]; off++; i++;
            } else {
                ok[off] = bk[j]; ov[off] = bv[j]; ow[off] = bw[j]; off++; j++;
            }
        }
    }
}

// Accumulator fold (the in-train merge's special case): A is a consolidated
// accumulator whose length the host knows, B a consolidated delta of at most
// FUSE_MAX rows whose length is on the device.  With so small a B every
// output position follows from B's lower bounds in A alone:
//   lb[j]  = lower bound of B[j] in A (nondecreasing: B is sorted)
//   s[j]   = +1 if B[j] matches no A row, 0 if it matches A[lb[j]] and the
//            summed weight survives, -1 if the sum is zero
//   S      = exclusive prefix of s, S[nb] its total
//   A[i]   goes to i + S[J], J = #{j : lb[j] <= i}; it is B[J-1]'s partner
//          iff lb[J-1] == i and B[J-1] matched (B's rows are distinct, so at
//          most one does, and of a run sharing one lower bound only the last)
//   B[j]   unmatched goes to lb[j] + S[j]
//   length = na + S[nb]
// Every workgroup computes lb, the flags and S for ALL of B redundantly (one
// global binary search per row; A is cache-resident) and keeps them in LDS —
// 4 + 4 + 1 bytes per row, 72 KiB at FUSE_MAX plus the scan's cells, so two
// workgroups fit a CU's 160 KiB — then emits its own slice of A and the
// unmatched B rows whose lower bound falls in it (lb == na: the last
// workgroup).  No count pass, no scratch and no inter-workgroup traffic.
// Stores are guarded by the output capacity na + bcap, so rows that are not
// consolidated (a caller's error) give a wrong batch, never a stray store.
#define FOLD_EQ 1u      // B[j] equals A[lb[j]]
#define FOLD_CANCEL 2u  // ... and the weights sum to zero
template <typename W>
__global__ __launch_bounds__(FUSE_THREADS, 4) void k_acc_fold(MergeArgs args) {
    __shared__ uint32_t s_lb[FUSE_MAX];
    __shared__ uint32_t s_S[FUSE_MAX + 1];  // int32 sums carried mod 2^32
    __shared__ uint8_t s_fl[FUSE_MAX];
    __shared__ uint32_t wave_tot[FUSE_THREADS / WAVE + 1];
    const int p = blockIdx.y;
    const int wg = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t na = args.na[p];
    const int nwg = dbspk::acc_fold_wgs(na);
    if (wg >= nwg) return;  // the grid is sized for the launch's longest A
    const int64_t nb64 = args.dnb[p] ? *args.dnb[p] : args.nb[p];
    const int64_t bcap = args.bcap[p];
    int64_t *out_len = args.d_len + p;
    if (na < 0 || na > ACC_FOLD_NA_MAX || nb64 < 0 || nb64 > FUSE_MAX ||
        nb64 > bcap) {  // failed upstream speculation: poison the length
        if (tid == 0 && wg == 0) *out_len = -1;
        return;
    }
    const int nb = (int)nb64;
    const uint64_t *ak = args.ak[p], *av = args.av[p];
    const W *aw = (const W *)args.aw[p];
    const uint64_t *bk = args.bk[p], *bv = args.bv[p];
    const W *bw = (const W *)args.bw[p];
    uint64_t *ok = args.ok[p], *ov = args.ov[p];
    W *ow = (W *)args.ow[p];
    const uint64_t ocap = (uint64_t)(na + bcap);

    // classify all of B (strided: coalesced B reads)
    for (int j = tid; j < nb; j += FUSE_THREADS) {
        const uint64_t k = bk[j], v = bv[j];
        int64_t lo = 0, hi = na;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const uint64_t mk = ak[mid];
            if (mk < k || (mk == k && av[mid] < v)) lo = mid + 1;
            else hi = mid;
        }
        uint32_t f = 0;
        if (lo < na && ak[lo] == k && av[lo] == v)
            f = (aw[lo] + bw[j] == (W)0) ? (FOLD_EQ | FOLD_CANCEL) : FOLD_EQ;
        s_lb[j] = (uint32_t)lo;
        s_fl[j] = (uint8_t)f;
    }
    __syncthreads();
    // S: consecutive items per thread, one block scan
    {
        const int items = (nb + FUSE_THREADS - 1) / FUSE_THREADS;  // <= 8
        const int j0 = min(tid * items, nb), j1 = min(j0 + items, nb);
        uint32_t sum = 0;
        for (int j = j0; j < j1; j++) {
            const uint32_t f = s_fl[j];
            sum += f == 0 ? 1u : (f & FOLD_CANCEL) ? ~0u : 0u;
        }
        uint32_t tot;
        uint32_t run = fuse_scan(sum, wave_tot, &tot);
        for (int j = j0; j < j1; j++) {
            s_S[j] = run;
            const uint32_t f = s_fl[j];
            run += f == 0 ? 1u : (f & FOLD_CANCEL) ? ~0u : 0u;
        }
        if (tid == 0) s_S[nb] = tot;
    }
    __syncthreads();

    const int64_t per = (na + nwg - 1) / nwg;
    const int64_t a0 = min((int64_t)wg * per, na);
    const int64_t a1 = min(a0 + per, na);
    // B rows whose lower bound falls in [a0, a1): [jlo, jhi)
    int jlo, jhi;
    {
        int lo = 0, hi = nb;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)s_lb[mid] < a0) lo = mid + 1; else hi = mid;
        }
        jlo = lo;
        hi = nb;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)s_lb[mid] < a1) lo = mid + 1; else hi = mid;
        }
        jhi = lo;
    }
    // the slice of A: J lies in [jlo, jhi]
    for (int64_t i = a0 + tid; i < a1; i += FUSE_THREADS) {
        int lo = jlo, hi = jhi;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)s_lb[mid] <= i) lo = mid + 1; else hi = mid;
        }
        const int J = lo;
        W w = aw[i];
        bool keep = true;
        if (J > 0 && (int64_t)s_lb[J - 1] == i && (s_fl[J - 1] & FOLD_EQ)) {
            if (s_fl[J - 1] & FOLD_CANCEL) keep = false;
            else w = w + bw[J - 1];
        }
        const uint64_t o = (uint64_t)(i + (int64_t)(int32_t)s_S[J]);
        if (keep && o < ocap) {
            ok[o] = ak[i];
            ov[o] = av[i];
            ow[o] = w;
        }
    }
    // the unmatched B rows of the slice; those past the end of A (lb == na)
    // belong to the last workgroup
    if (wg == nwg - 1) jhi = nb;
    for (int j = jlo + tid; j < jhi; j += FUSE_THREADS) {
        if (s_fl[j] != 0) continue;
        const uint64_t o =
            (uint64_t)((int64_t)s_lb[j] + (int64_t)(int32_t)s_S[j]);
        if (o < ocap) {
            ok[o] = bk[j];
            ov[o] = bv[j];
            ow[o] = bw[j];
        }
    }
    if (wg == 0 && tid == 0) *out_len = na + (int64_t)(int32_t)s_S[nb];
}

// ---------------------------------------------------------------------------
// multi-batch spine join: the reference reads a spine through a k-way
// CursorList (trace/cursor/cursor_list.rs); join is linear in the trace, so
// one kernel probes every spine batch (descriptors passed by value as kernel
// arguments) — one count+emit pair per tick per side regardless of spine depth.
// ---------------------------------------------------------------------------

__device__ inline int64_t gallop_run(const uint64_t *tk, int64_t nt, uint64_t key,
                                     int64_t lo) {
    // length of the key's run starting at lo (gallop + bounded binary search,
    // the advance.rs:11-60 idiom)
    if (lo >= nt || tk[lo] != key) return 0;
    int64_t hi = lo, step = 1;
    while (hi + step < nt && tk[hi + step] == key) { hi += step; step <<= 1; }
    int64_t rem = min(step, nt - hi);
    // upper bound within (hi, hi+rem)
    int64_t a = 0, b = rem;
    while (a < b) {
        int64_t m = (a + b) / 2;
        if (tk[hi + m] <= key) a = m + 1; else b = m;
    }
    return hi + a - lo;
}

__global__ void k_join_count_multi(const uint64_t *dk, int64_t nd, TraceArgs t,
                                   uint32_t *cnts /* nd*nb */,
                                   uint64_t *counts /* nd */) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nd;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t key = dk[i];
        uint64_t total = 0;
        for (int b = 0; b < t.nb; b++) {
            int64_t lo = lower_bound_k(t.k[b], t.n[b], key);
            int64_t c = gallop_run(t.k[b], t.n[b], key, lo);
            cnts[i * t.nb + b] = (uint32_t)c;
            total += c;
        }
        counts[i] = total;
    }
}


__global__ void k_join_emit_multi(const uint64_t *dk, const uint64_t *dv,
                                  const int64_t *dw, int64_t nd, TraceArgs t,
                                  const uint32_t *cnts, const uint64_t *offsets,
                                  int64_t n_out, int proj, uint64_t param,
                                  uint64_t *ok, uint64_t *ov, int64_t *ow) {
    for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < n_out;
         o += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = nd;
        while (lo < hi) {
            int64_t mid = (lo + hi) / 2;
            if (offsets[mid] <= (uint64_t)o) lo = mid + 1; else hi = mid;
        }
        int64_t i = lo - 1;
        int64_t j = o - (int64_t)offsets[i];
        int b = 0;
        while (j >= (int64_t)cnts[i * t.nb + b]) {
            j -= cnts[i * t.nb + b];
            b++;
        }
        uint64_t key = dk[i];
        int64_t start = lower_bound_k(t.k[b], t.n[b], key);
        int64_t ti = start + j;
        uint64_t hi_o, lo_o;
        const bool valid =
            proj_out(proj, param, key, dv[i], t.v[b][ti], hi_o, lo_o);
        ok[o] = hi_o;
        ov[o] = lo_o;
        ow[o] = valid ? dw[i] * t.w[b][ti] : 0;
    }
}

// small join count + scan (nd <= 8192), split in two chained launches: a
// multi-block probe phase (the round-1 single-WG version serialized ~2M
// dependent probe loads on ONE CU — 44 us of a 280 us q3 tick) and a
// single-WG scan that re-sums the per-row counts from cnts.
#define JPROBE_BLOCKS 8

__global__ __launch_bounds__(BLK, 8) void k_join_probe_multi(
    JoinCountArgs args) {
    const int plan = blockIdx.x / JPROBE_BLOCKS;
    const int slice = blockIdx.x % JPROBE_BLOCKS;
    const uint64_t *dk = args.dk[plan];
    const int64_t nd =
        args.nd_dev[plan] ? *args.nd_dev[plan] : args.nd[plan];
    const TraceArgs &t = args.t[plan];
    const int64_t tn0 = args.tn_dev[plan] ? *args.tn_dev[plan] : t.n[0];
    if (nd < 0 || nd > FUSE_MAX || tn0 < 0) return;  // scan flags the total
    uint32_t *cnts = args.cnts[plan];
    int64_t *starts = args.starts[plan];  // null: the caller re-searches
    for (int64_t i = (int64_t)slice * BLK + threadIdx.x; i < nd;
         i += (int64_t)JPROBE_BLOCKS * BLK) {
        const uint64_t key = dk[i];
        for (int b = 0; b < t.nb; b++) {
            const int64_t tb_n = b == 0 ? tn0 : t.n[b];
            int64_t lo = lower_bound_k(t.k[b], tb_n, key);
            const uint32_t c = (uint32_t)gallop_run(t.k[b], tb_n, key, lo);
            cnts[(int64_t)i * t.nb + b] = c;
            if (starts && c) starts[(int64_t)i * t.nb + b] = lo;
        }
    }
}

__global__ __launch_bounds__(FUSE_THREADS, 4) void k_join_scan_small(
    JoinCountArgs args) {
    __shared__ uint32_t wave_tot[FUSE_THREADS / WAVE + 1];
    const int plan = blockIdx.x;
    const int64_t nd =
        args.nd_dev[plan] ? *args.nd_dev[plan] : args.nd[plan];
    const TraceArgs &t = args.t[plan];
    const int64_t tn0 = args.tn_dev[plan] ? *args.tn_dev[plan] : t.n[0];
    if (nd < 0 || nd > FUSE_MAX || tn0 < 0) {
        if (threadIdx.x == 0) args.d_total[plan] = -1;
        return;
    }
    uint32_t *cnts = args.cnts[plan];
    uint64_t *offsets = args.offsets[plan];
    int64_t *d_total = args.d_total + plan;
    const int tid = threadIdx.x;
    uint32_t row_tot[FUSE_ITEMS];
    uint32_t tsum = 0;
    for (int j = 0; j < FUSE_ITEMS; j++) {
        int i = tid * FUSE_ITEMS + j;
        uint32_t rt = 0;
        if (i < nd)
            for (int b = 0; b < t.nb; b++)
                rt += cnts[(int64_t)i * t.nb + b];
        row_tot[j] = rt;
        tsum += rt;
    }
    uint32_t total;
    uint32_t off = fuse_scan(tsum, wave_tot, &total);
    for (int j = 0; j < FUSE_ITEMS; j++) {
        int i = tid * FUSE_ITEMS + j;
        if (i < nd) offsets[i] = off;
        off += row_tot[j];
    }
    if (tid == 0) *d_total = (int64_t)total;
}

// ---------------------------------------------------------------------------
// join tail: everything of a chained join tick behind the probe, in ONE
// single-workgroup launch — scan of the probe's counts, capacity check, emit
// into the capacity buffer, sort+consolidate into the output store.  At tick
// scale (a few hundred delta and output rows) these were three dependent
// launches of one workgroup each plus a length copy between them; here the
// phases are separated by block barriers only.
//
// The delta rows of all (<= 3) plans form ONE row sequence, plan after plan
// (R <= 3 * 8192 rows), scanned once: row r's exclusive offset is at once its
// first position in the capacity buffer, plan-major as the per-plan emits
// wrote it.  The offsets stay in LDS — the sort's three buffers, free until
// the sort phase — and the emit binary-searches them there.  The probe left,
// per delta row i and trace batch b, the match count cnts[i*nb+b] and, where
// that is nonzero, the run's first position starts[i*nb+b]: the emit
// searches neither the trace nor global memory.  Loops over a row's batches
// are unrolled to MAX_TRACE_BATCHES predicated loads, so they are issued
// together instead of one load latency per batch.
//
// A combined total within one row per thread (<= 1024) never reaches the
// capacity buffer: thread o keeps emitted row o in registers and the sort's
// small-batch path takes it from there.  d_final is then >= 0, and the host
// reads the capacity buffer only when d_final < 0.
//
// Verdicts (the host reads them after the tail readback):
//   totals[p]  plan p's row total, -1 if one of its lengths is a lost
//              speculation; offsets[p][] (plan-local) is written for every
//              plan whose total is >= 0, whatever the other plans did, so
//              the host's explicit replay can emit from them
//   d_flag     1: nothing usable in the capacity buffer (negative plan, or
//              combined total > cap); rows are only ever written below cap
//   d_total    combined total, -1 if flagged
//   d_final    consolidated length in the output store, -1 if flagged or if
//              the combined total exceeds the fused sort (then the emitted
//              rows wait in the capacity buffer for a sized sort)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(FUSE_THREADS, 4) void k_join_tail_small(
    JoinTailArgs a) {
    SORT_CONS_LDS
    // row r's offset cell: three 8192-cell buffers back to back
    auto cell = [&](int r) -> uint32_t * {
        return r < FUSE_MAX ? cnt + r
                            : (r < 2 * FUSE_MAX ? bufA + (r - FUSE_MAX)
                                                : bufB + (r - 2 * FUSE_MAX));
    };
    const int tid = threadIdx.x;
    // per-plan constants in registers (np <= 3; absent plans have no rows)
    int rb[4] = {0, 0, 0, 0};  // first row of plan p; rb[3] = R
    int nbp[3] = {0, 0, 0};
    const uint32_t *cp[3] = {nullptr, nullptr, nullptr};
    int neg = 0;  // bit p: plan p read a lost speculation's length
#pragma unroll
    for (int p = 0; p < 3; p++) {
        int n = 0;
        if (p < a.np) {
            const int64_t nd = *a.nd_dev[p];
            const int64_t tn0 = a.tn_dev[p] ? *a.tn_dev[p] : a.t[p].n[0];
            if (nd < 0 || nd > FUSE_MAX || tn0 < 0) {
                neg |= 1 << p;
            } else {
                n = (int)nd;
            }
            nbp[p] = a.t[p].nb;
            cp[p] = a.cnts[p];
        }
        rb[p + 1] = rb[p] + n;
    }
    const int R = rb[3];
    auto plan_of = [&](int r) -> int { return (r >= rb[1]) + (r >= rb[2]); };

    // ---- scan: row totals into their cells, then exclusive offsets ----
    const int ipt = (R + FUSE_THREADS - 1) / FUSE_THREADS;  // rows per thread
    uint32_t tsum = 0;
    for (int j = 0; j < ipt; j++) {
        const int r = tid * ipt + j;
        if (r >= R) break;
        const int p = plan_of(r);
        const int nb = p == 0 ? nbp[0] : (p == 1 ? nbp[1] : nbp[2]);
        const uint32_t *c =
            (p == 0 ? cp[0] : (p == 1 ? cp[1] : cp[2])) +
            (int64_t)(r - (p == 0 ? rb[0] : (p == 1 ? rb[1] : rb[2]))) * nb;
        uint32_t rt = 0;
#pragma unroll
        for (int b = 0; b < MAX_TRACE_BATCHES; b++)
            rt += b < nb ? c[b] : 0;
        *cell(r) = rt;
        tsum += rt;
    }
    uint32_t total;
    uint32_t off = fuse_scan(tsum, wave_tot, &total);
    for (int j = 0; j < ipt; j++) {
        const int r = tid * ipt + j;
        if (r >= R) break;
        uint32_t *q = cell(r);
        const uint32_t rt = *q;
        *q = off;
        off += rt;
    }
    __syncthreads();

    // ---- per-plan totals and plan-local offsets for the explicit replay ----
    uint32_t pb[4];  // plan p's first output position; pb[3] = total
#pragma unroll
    for (int p = 0; p < 4; p++) pb[p] = rb[p] < R ? *cell(rb[p]) : total;
    if (tid == 0) {
#pragma unroll
        for (int p = 0; p < 3; p++)
            if (p < a.np)
                a.totals[p] =
                    (neg >> p) & 1 ? -1 : (int64_t)(pb[p + 1] - pb[p]);
    }
    for (int r = tid; r < R; r += FUSE_THREADS) {
        const int p = plan_of(r);
        const int r0 = p == 0 ? rb[0] : (p == 1 ? rb[1] : rb[2]);
        const uint32_t b0 = p == 0 ? pb[0] : (p == 1 ? pb[1] : pb[2]);
        a.offsets[p][r - r0] = *cell(r) - b0;
    }

    // ---- emit: only if the combined rows fit the capacity buffer ----
    const int64_t acc = total;
    const bool okf = !neg && acc <= a.cap;
    // within one row per thread the rows go to the sort in registers and
    // skip the capacity buffer: the host reads that buffer only when
    // d_final < 0, and this branch always leaves d_final >= 0
    const bool onchip = okf && total <= FUSE_THREADS;
    uint64_t rk = ~0ull, rv = ~0ull;  // pad row for threads past the total
    int64_t rw = 0;
    if (okf) {
        for (uint32_t o = tid; o < total; o += FUSE_THREADS) {
            int lo = 0, hi = R;
            while (lo < hi) {
                const int mid = (lo + hi) / 2;
                if (*cell(mid) <= o) lo = mid + 1; else hi = mid;
            }
            const int r = lo - 1;
            const int p = plan_of(r);
            const TraceArgs &t = a.t[p];
            const int nb = t.nb;
            const int64_t i = r - (p == 0 ? rb[0] : (p == 1 ? rb[1] : rb[2]));
            const uint32_t *c = a.cnts[p] + i * nb;
            uint32_t j = o - *cell(r);
            int b = 0;
#pragma unroll
            for (int bb = 0; bb < MAX_TRACE_BATCHES; bb++) {
                // past nb nothing is taken: j is below the row's total
                const uint32_t cb = bb < nb ? c[bb] : 0xFFFFFFFFu;
                const bool take = b == bb && j >= cb;
                j -= take ? cb : 0;
                b += take ? 1 : 0;
            }
            const int64_t ti = a.starts[p][i * nb + b] + j;
            const uint64_t key = a.dk[p][i];
            uint64_t hi_o, lo_o;
            const bool valid = proj_out(a.proj[p], 0, key, a.dv[p][i],
                                        t.v[b][ti], hi_o, lo_o);
            const int64_t wo = valid ? a.dw[p][i] * t.w[b][ti] : 0;
            if (onchip) {  // o == tid: this thread's only row
                rk = hi_o;
                rv = lo_o;
                rw = wo;
            } else {
                a.ek[o] = hi_o;
                a.ev[o] = lo_o;
                a.ew[o] = wo;
            }
        }
    }
    __syncthreads();  // the cells are the sort's buffers from here on
    if (tid == 0) {
        *a.d_total = okf ? acc : -1;
        *a.d_flag = okf ? 0 : 1;
    }
    if (!okf || acc > FUSE_MAX) {
        if (tid == 0) *a.d_final = -1;
        return;
    }
    if (onchip) {  // block-uniform
        if (acc == 0) {
            if (tid == 0) *a.d_final = 0;
            return;
        }
        sort_cons_small_rows(rk, rv, rw, acc, a.ok, a.ov, a.ow, a.d_final,
                             bufA, bufB, cnt, wave_tot);
        return;
    }
    // the emitted rows were stored by this workgroup; the barrier above
    // orders them before the sort's loads
    sort_cons_body<int64_t>(a.ek, a.ev, a.ew, acc, a.tk, a.tv, a.tw, a.ok,
                            a.ov, a.ow, a.d_final, bufA, bufB, cnt, wave_tot,
                            smax, smin);
}

// ---------------------------------------------------------------------------
// incremental distinct (operator/distinct.rs:273,404-462 at root scope):
// for each delta pair (k,v):  out = [w_before + dw > 0] - [w_before > 0]
// where w_before is the pair's total weight in the delayed integral.  NOT
// linear in the trace (the indicator needs the total), so one kernel probes
// every spine batch.  Output positions via flags+scan keep delta order, so
// the result is consolidated by construction.
// ---------------------------------------------------------------------------

__device__ inline int64_t find_pair_weight(const uint64_t *tk,
                                           const uint64_t *tv,
                                           const int64_t *tw, int64_t n,
                                           uint64_t key, uint64_t val) {
    int64_t lo = lower_bound_k(tk, n, key);
    int64_t hi = lo + gallop_run(tk, n, key, lo);
    // binary search the val within the key's run
    while (lo < hi) {
        int64_t mid = (lo + hi) / 2;
        if (tv[mid] < val) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n && tk[lo] == key && tv[lo] == val) return tw[lo];
    return 0;
}

__global__ void k_distinct_count(const uint64_t *dk, const uint64_t *dv,
                                 const int64_t *dw, int64_t nd, TraceArgs t,
                                 uint64_t *flags, int64_t *outw) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nd;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t before = 0;
        for (int b = 0; b < t.nb; b++)
            before += find_pair_weight(t.k[b], t.v[b], t.w[b], t.n[b], dk[i],
                                       dv[i]);
        int64_t after = before + dw[i];
        int64_t o = (int64_t)(after > 0) - (int64_t)(before > 0);
        flags[i] = o != 0;
        outw[i] = o;
    }
}

// ---------------------------------------------------------------------------
// aggregate (linear / max) + upsert  (count/emit over delta keys)
// ---------------------------------------------------------------------------

// MODE: 0 = linear weight-sum (WeightedCount, aggregate/mod.rs:129-156),
// 1 = Max (max.rs:36-55), 2 = q6's fold: average of the last <= 10 vals in
// the key's run (queries/q6.rs:96-110 VecDeque fold in cursor order, every
// val of non-zero weight counting whatever its sign, fold.rs:87; the price
// lives in the low 27 bits of the val)
template <int MODE>
__global__ void k_agg_count(const uint64_t *keys, int64_t nd,
                            const uint64_t *ik, const int64_t *iw, int64_t ni,
                            const uint64_t *ok_, int64_t no,
                            uint64_t *counts, uint64_t *istart, uint64_t *ostart,
                            uint64_t *newval, uint64_t *has_new) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nd;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t key = keys[i];
        int64_t ilo = lower_bound_k(ik, ni, key);
        int64_t ihi = upper_bound_k(ik, ni, key);
        uint64_t nv = 0;
        uint64_t hn = 0;
        if (MODE != 0) {
            // consolidated trace: any present val has w != 0; max = last val
            if (ihi > ilo) { nv = 1; hn = 1; }
            if (hn) nv = 0;  // placeholder; real val read in emit via istart/iend
        } else {
            int64_t s = 0;
            for (int64_t t = ilo; t < ihi; t++) s += iw[t];
            if (s != 0) { nv = (uint64_t)s; hn = 1; }
        }
        int64_t olo = lower_bound_k(ok_, no, key);
        int64_t ohi = upper_bound_k(ok_, no, key);
        counts[i] = (hn ? 1 : 0) + (ohi - olo);
        istart[i] = (uint64_t)ilo;
        ostart[i] = (uint64_t)olo;
        newval[i] = MODE != 0 ? (ihi > ilo ? /* iend */ (uint64_t)ihi : 0) : nv;
        has_new[i] = hn;
    }
}

template <int MODE>
__global__ void k_agg_emit(const uint64_t *keys, int64_t nd,
                           const uint64_t *iv, const uint64_t *ov_,
                           const int64_t *ow_, const uint64_t *offsets,
                           const uint64_t *counts, const uint64_t *istart,
                           const uint64_t *ostart, const uint64_t *newval,
                           const uint64_t *has_new, uint64_t *rk, uint64_t *rv,
                           int64_t *rw) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nd;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t key = keys[i];
        uint64_t pos = offsets[i];
        uint64_t cnt = counts[i];
        uint64_t emitted = 0;
        if (has_new[i]) {
            uint64_t nv;
            if (MODE == 1) {
                nv = iv[newval[i] - 1];  // last val of key's run (max.rs:40-52)
            } else if (MODE == 2) {
                // q6.rs:96-110: the VecDeque fold keeps the last <= 10 vals
                // of the seller's cursor-ordered run; avg of their prices
                // (val = (auction<<27)|price: low 27 bits), integer division
                const uint64_t ihi = newval[i], ilo = istart[i];
                const uint64_t n10 =
                    ihi - ilo < 10 ? ihi - ilo : (uint64_t)10;
                uint64_t sum = 0;
                for (uint64_t t = ihi - n10; t < ihi; t++)
                    sum += iv[t] & 0x7FFFFFFull;
                nv = sum / n10;
            } else {
                nv = newval[i];
            }
            rk[pos] = key; rv[pos] = nv; rw[pos] = 1;
            pos++; emitted++;
        }
        // retractions from the output trace (upsert.rs:180-195)
        for (uint64_t t = ostart[i]; emitted < cnt; t++, emitted++, pos++) {
            rk[pos] = key; rv[pos] = ov_[t]; rw[pos] = -ow_[t];
        }
    }
}

// multi-batch linear aggregate (spine batches summed; linear op): per-key
// weight sums of one batch added into acc.  f64 sums run in batch-position
// order (deterministic).
template <typename W>
__global__ void k_agg_sum(const uint64_t *keys, int64_t nd, const uint64_t *ik,
                          const W *iw, int64_t ni, W *acc) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nd;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t key = keys[i];
        int64_t lo = lower_bound_k(ik, ni, key);
        int64_t hi = upper_bound_k(ik, ni, key);
        W sum = 0;
        for (int64_t t = lo; t < hi; t++) sum += iw[t];
        acc[i] += sum;
    }
}

// emit (key, bits(sum), +1) for sum != 0 (f64: WeightedCount returns None for
// a zero aggregate — aggregate/mod.rs:129-156 with R = F64)
template <typename W>
__global__ void k_emit_nonzero(const uint64_t *keys, const W *acc, int64_t nd,
                               uint64_t *ctr, uint64_t *ok, uint64_t *ov,
                               int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nd;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (acc[i] != W(0)) {
            uint64_t p = atomicAdd((unsigned long long *)ctr, 1ull);
            ok[p] = keys[i];
            W a = acc[i];
            ov[p] = *(const uint64_t *)&a;
            ow[p] = 1;
        }
    }
}

// ---------------------------------------------------------------------------
// device-resident watermark (q5.rs:85-90 / q8.rs:63-65 waterline): a single
// thread advances the persistent watermark state by the tick's max event
// time and publishes the window bounds for the chained ranges launch.
// state = {wm, s0, e0, have_prev}; bounds = {s0, e0, s1, e1, have_prev, err}.
// ---------------------------------------------------------------------------

// gmax: the tick's max event time, 0 when it has none
__device__ void wm_advance(uint64_t gmax, uint64_t width, uint64_t tumble,
                           uint64_t lag, unsigned long long *state,
                           unsigned long long *bounds) {
    uint64_t wm = state[0];
    if (gmax > 0) wm = max(wm, gmax - lag);
    uint64_t rounded = wm - wm % tumble;
    uint64_t s1 = rounded >= width ? rounded - width : 0;
    uint64_t e1 = rounded;
    bounds[0] = state[1];
    bounds[1] = state[2];
    bounds[2] = s1;
    bounds[3] = e1;
    bounds[4] = state[3];
    bounds[5] = 0;
    state[0] = wm;
    state[1] = s1;
    state[2] = e1;
    state[3] = 1;
}

// err=1 when the delta length is the speculative-sort overflow sentinel: the
// state is left untouched and the host runs the update again with the real
// length once it has re-sorted
__global__ void k_wm_update(WmSource src, uint64_t width, uint64_t tumble,
                            uint64_t lag, unsigned long long *state,
                            unsigned long long *bounds) {
    uint64_t gmax = 0;
    if (src.gmax_dev) {
        gmax = *src.gmax_dev;
    } else {
        const int64_t n = src.n_dev ? *src.n_dev : src.n;
        if (n < 0) {
            bounds[5] = 1;
            return;
        }
        if (n > 0) gmax = src.ak[n - 1];
    }
    wm_advance(gmax, width, tumble, lag, state, bounds);
}

// ---------------------------------------------------------------------------
// window (window.rs:144-220): all three regions of every spine batch plus the
// tick's batch region in one ranges launch + one emit launch (evaluated per
// spine batch; the trace excludes the current tick).
// Region table rows: [src_batch(-1 = tick batch), lo, len, sign, goff]
// ---------------------------------------------------------------------------

__global__ void k_window_ranges_multi(TraceArgs t, const uint64_t *bk,
                                      int64_t bn, int have_prev, uint64_t s0,
                                      uint64_t e0, uint64_t s1, uint64_t e1,
                                      int64_t *table, int64_t *d_total,
                                      const int64_t *bn_dev,
                                      const unsigned long long *bounds) {
    if (bounds) {  // chained: bounds from k_wm_update, delta length from sort
        if (bounds[5] != 0 || (bn_dev && *bn_dev < 0)) {
            if (threadIdx.x == 0) *d_total = -1;
            return;
        }
        s0 = bounds[0];
        e0 = bounds[1];
        s1 = bounds[2];
        e1 = bounds[3];
        have_prev = (int)bounds[4];
        if (bn_dev) bn = *bn_dev;
    }
    const int nreg = 3 * t.nb + 1;
    for (int r = threadIdx.x; r < nreg; r += blockDim.x) {
        int64_t src = -1, lo = 0, len = 0, sign = 1;
        if (r < 3 * t.nb) {
            int b = r / 3, which = r % 3;
            const uint64_t *k = t.k[b];
            int64_t n = t.n[b];
            src = b;
            if (have_prev) {
                if (which == 0) {  // region 1: [s0, min(s1,e0)) retract
                    uint64_t end = min(s1, e0);
                    lo = lower_bound_k(k, n, s0);
                    len = max((int64_t)0, lower_bound_k(k, n, end) - lo);
                    sign = -1;
                } else if (which == 1) {  // shrink: [e1, e0) retract
                    if (e1 < e0) {
                        lo = lower_bound_k(k, n, e1);
                        len = max((int64_t)0, lower_bound_k(k, n, e0) - lo);
                    }
                    sign = -1;
                } else {  // region 3: [max(e0,s1), e1) insert
                    uint64_t st = max(e0, s1);
                    lo = lower_bound_k(k, n, st);
                    len = max((int64_t)0, lower_bound_k(k, n, e1) - lo);
                }
            }
        } else {  // batch region: [s1, e1) insert
            lo = lower_bound_k(bk, bn, s1);
            len = max((int64_t)0, lower_bound_k(bk, bn, e1) - lo);
        }
        table[r * 5 + 0] = src;
        table[r * 5 + 1] = lo;
        table[r * 5 + 2] = len;
        table[r * 5 + 3] = sign;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int r = 0; r < nreg; r++) {
            table[r * 5 + 4] = acc;
            acc += table[r * 5 + 2];
        }
        *d_total = acc;
    }
}

__global__ void k_window_emit_multi(TraceArgs t, const uint64_t *bk,
                                    const uint64_t *bv, const int64_t *bw,
                                    const int64_t *table, int nreg,
                                    int64_t total, uint64_t *ok, uint64_t *ov,
                                    int64_t *ow) {
    for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < total;
         o += (int64_t)gridDim.x * blockDim.x) {
        // binary search the region by goff
        int lo = 0, hi = nreg;
        while (lo < hi) {
            int mid = (lo + hi) / 2;
            if (table[mid * 5 + 4] <= o) lo = mid + 1; else hi = mid;
        }
        int r = lo - 1;
        int64_t src = table[r * 5 + 0];
        int64_t i = table[r * 5 + 1] + (o - table[r * 5 + 4]);
        int64_t sign = table[r * 5 + 3];
        const uint64_t *k = src < 0 ? bk : t.k[src];
        const uint64_t *v = src < 0 ? bv : t.v[src];
        const int64_t *w = src < 0 ? bw : t.w[src];
        ok[o] = k[i];
        ov[o] = v[i];
        ow[o] = sign * w[i];
    }
}

// ---------------------------------------------------------------------------
// shard partition: xxh3(key) % nshards (shard.rs:165-199, hash.rs:9-13)
// ---------------------------------------------------------------------------

__device__ inline uint64_t dev_xxh3_u64(uint64_t key, uint64_t seed) {
    const uint64_t SEC8_16 = 0x1cad21f72c81017cull ^ 0xdb979083e96dd4deull;
    // read64(kSecret+8) = 0x1cad21f72c81017c, read64(kSecret+16) = 0xdb979083e96dd4de
    uint64_t s = seed ^ ((uint64_t)__builtin_bswap32((uint32_t)seed) << 32);
    uint32_t in_lo = (uint32_t)key;
    uint32_t in_hi = (uint32_t)(key >> 32);
    uint64_t bitflip = SEC8_16 - s;
    uint64_t input64 = (uint64_t)in_hi + ((uint64_t)in_lo << 32);
    uint64_t h = input64 ^ bitflip;
    uint64_t r49 = (h << 49) | (h >> 15);
    uint64_t r24 = (h << 24) | (h >> 40);
    h ^= r49 ^ r24;
    h *= 0x9FB21C651E98DF25ull;
    h ^= (h >> 35) + 8;
    h *= 0x9FB21C651E98DF25ull;
    h ^= h >> 28;
    return h;
}

#define DBSP_HASH_SEED 0x7f95ef85be33c337ull  /* hash.rs:6 */

__global__ void k_shard_hist(const uint64_t *k, int64_t n, int nshards,
                             uint64_t *hist) {
    __shared__ uint64_t sh[64];
    for (int i = threadIdx.x; i < nshards; i += BLK) sh[i] = 0;
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        atomicAdd((unsigned long long *)&sh[dev_xxh3_u64(k[i], DBSP_HASH_SEED) % nshards], 1ull);
    __syncthreads();
    for (int i = threadIdx.x; i < nshards; i += BLK)
        atomicAdd((unsigned long long *)&hist[i], (unsigned long long)sh[i]);
}

// unstable within a shard (receivers re-consolidate; Z-set semantics are
// order-invariant — shard.rs re-assembles via Spine + consolidate anyway)
__global__ void k_shard_scatter(const uint64_t *k, const uint64_t *v,
                                const int64_t *w, int64_t n, int nshards,
                                uint64_t *cursor, uint64_t *ok, uint64_t *ov,
                                int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        int s = (int)(dev_xxh3_u64(k[i], DBSP_HASH_SEED) % nshards);
        uint64_t pos = atomicAdd((unsigned long long *)&cursor[s], 1ull);
        ok[pos] = k[i];
        ov[pos] = v[i];
        ow[pos] = w[i];
    }
}

// ---------------------------------------------------------------------------
// Nexmark flat_map_index kernels (ingress: input.rs:591-721 + per-query
// flat_map_index in queries/q{3,5,8}.rs); ticket-append (order-free, the
// consolidate that follows sorts)
// ---------------------------------------------------------------------------

// block-aggregated ticket append for both output streams at once: wave
// ballots rank the lanes, the block's first wave scans the per-wave counts
// and takes ONE ticket per stream per block from the global counters (none
// for a stream without a match), and LDS hands every wave its base.  The
// per-wave atomics this replaces serialised on the two counter words: at
// q3's ~1 % selectivity nearly every matching row paid its own.  Every
// thread of the block calls it (two barriers).
#define FLATMAP_BLK 1024
#define FLATMAP_WAVES (FLATMAP_BLK / WAVE)
__device__ inline void block_append2(unsigned long long *c0,
                                     unsigned long long *c1, bool p0, bool p1,
                                     uint32_t (*s_cnt)[FLATMAP_WAVES],
                                     unsigned long long (*s_base)[FLATMAP_WAVES],
                                     uint64_t &pos0, uint64_t &pos1) {
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1), wid = tid / WAVE;
    const uint64_t m0 = __ballot(p0), m1 = __ballot(p1);
    if (lane == 0) {
        s_cnt[0][wid] = (uint32_t)__popcll(m0);
        s_cnt[1][wid] = (uint32_t)__popcll(m1);
    }
    __syncthreads();
    if (tid < 2 * FLATMAP_WAVES) {  // one 16-lane group per stream
        const int st = tid / FLATMAP_WAVES, w = tid % FLATMAP_WAVES;
        const uint32_t c = s_cnt[st][w];
        uint32_t inc = c;
        for (int d = 1; d < FLATMAP_WAVES; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, FLATMAP_WAVES);
            if (w >= d) inc += up;
        }
        const uint32_t total = __shfl(inc, FLATMAP_WAVES - 1, FLATMAP_WAVES);
        unsigned long long base = 0;
        if (w == 0 && total > 0)
            base = atomicAdd(st ? c1 : c0, (unsigned long long)total);
        base = (unsigned long long)__shfl((long long)base, 0, FLATMAP_WAVES);
        s_base[st][w] = base + (inc - c);
    }
    __syncthreads();
    const uint64_t lt = ((uint64_t)1 << lane) - 1;
    pos0 = s_base[0][wid] + (uint64_t)__popcll(m0 & lt);
    pos1 = s_base[1][wid] + (uint64_t)__popcll(m1 & lt);
}

__global__ void k_columnize(const dbsp_event *ev, int64_t n, uint64_t *kind,
                            uint64_t *f0, uint64_t *f1, uint64_t *f2,
                            uint64_t *f3, uint64_t *f4, int64_t *w) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const dbsp_event e = ev[i];
        kind[i] = e.kind;
        f0[i] = e.f0;
        f1[i] = e.f1;
        f2[i] = e.f2;
        f3[i] = e.f3;
        f4[i] = e.f4;
        w[i] = e.w;
    }
}

// cap0/cap1: rows of the output columns.  A ticket at or past the capacity
// advances the counter but stores nothing, so a counter that did not start
// at zero shows as an impossible length downstream, never as a stray store.
__global__ __launch_bounds__(FLATMAP_BLK) void k_flatmap(
        const dbsp_event *ev, dbspk::EventCols cols, int64_t n, int query,
        uint64_t *c0, uint64_t *k0, uint64_t *v0, int64_t *w0, int64_t cap0,
        uint64_t *c1, uint64_t *k1, uint64_t *v1, int64_t *w1, int64_t cap1) {
    __shared__ uint32_t s_cnt[2][FLATMAP_WAVES];
    __shared__ unsigned long long s_base[2][FLATMAP_WAVES];
    // block-uniform outer loop (base is the block's first row) so the
    // barriers in block_append2 see every thread
    const int64_t stride = (int64_t)gridDim.x * FLATMAP_BLK;
    for (int64_t base = blockIdx.x * (int64_t)FLATMAP_BLK; base < n;
         base += stride) {
        const int64_t i = base + threadIdx.x;
        dbsp_event e{};
        const bool act = i < n;
        if (act) {
            if (cols.kind) {  // columnized staging: 7 coalesced 8 B streams
                e.kind = cols.kind[i]; e.f0 = cols.f0[i]; e.f1 = cols.f1[i];
                e.f2 = cols.f2[i]; e.f3 = cols.f3[i]; e.f4 = cols.f4[i];
                e.w = cols.w[i];
            } else {
                e = ev[i];
            }
        }
        // per query: the predicate and the row of each stream
        bool p0 = false, p1 = false;
        uint64_t rk0 = 0, rv0 = 0, rk1 = 0, rv1 = 0;
        int64_t rw0 = e.w, rw1 = e.w;
        if (query == 3) {
            // q3.rs:37-49
            p0 = act && e.kind == 1 && e.f2 == 10;
            rk0 = e.f1; rv0 = e.f0;
            p1 = act && e.kind == 0 &&
                 (e.f3 == 1 || e.f3 == 2 || e.f3 == 3);  // CA,ID,OR
            rk1 = e.f0;
            rv1 = (e.f1 << 8) | ((e.f2 & 0xF) << 4) | (e.f3 & 0xF);
        } else if (query == 4) {
            // q4.rs:45-56: auctions by id (validity window + category packed
            // into the val), bids by auction (dt + price packed)
            p0 = act && e.kind == 1;
            rk0 = e.f0;
            rv0 = (e.f3 << 28) | (((e.f4 - e.f3) & 0xFFFFFFull) << 4) |
                  (e.f2 & 0xFull);
            p1 = act && e.kind == 2;
            rk1 = e.f0;
            rv1 = (e.f3 << 27) | (e.f2 & 0x7FFFFFFull);
        } else if (query == 6) {
            // q6.rs:46-57: auctions by id (seller + validity window packed:
            // dt 28 bits from bit 36, duration 16 bits, seller 20 bits),
            // bids by auction as q4
            p0 = act && e.kind == 1;
            rk0 = e.f0;
            rv0 = (e.f3 << 36) | (((e.f4 - e.f3) & 0xFFFFull) << 20) |
                  (e.f1 & 0xFFFFFull);
            p1 = act && e.kind == 2;
            rk1 = e.f0;
            rv1 = (e.f3 << 27) | (e.f2 & 0x7FFFFFFull);
        } else if (query == 5) {
            // q5.rs:79-83: bids by time
            p0 = act && e.kind == 2;
            rk0 = e.f3; rv0 = e.f0;
        } else if (query == 8) {
            // q8.rs:50-60
            p0 = act && e.kind == 0;
            // (id, name) packed ORDER-PRESERVING as id*1024+name: the
            // name dictionary is the generator's ~1000-value space
            // (people.rs name draw), so 10 bits suffice — and the packed
            // range stays ~2^20 per tick instead of id<<32 spanning 2^42,
            // which halves the delta sort's digit passes
            rk0 = e.f4; rv0 = (e.f0 << 10) | (e.f1 & 0x3FFull);
            p1 = act && e.kind == 1;
            rk1 = e.f3; rv1 = e.f1;
        } else if (query == 101) {
            // bids.map_index(|b| (b.auction, (b.date_time, b.price))) with
            // the price weighed into the weight (aggregate/mod.rs:297-323):
            // the input of partitioned_rolling_aggregate_linear
            p0 = act && e.kind == 2;
            rk0 = e.f0; rv0 = e.f3;
            rw0 = e.w * (int64_t)e.f2;
        }
        uint64_t pos0, pos1;
        block_append2((unsigned long long *)c0, (unsigned long long *)c1, p0,
                      p1, s_cnt, s_base, pos0, pos1);
        if (p0 && pos0 < (uint64_t)cap0) {
            k0[pos0] = rk0; v0[pos0] = rv0; w0[pos0] = rw0;
        }
        if (p1 && pos1 < (uint64_t)cap1) {
            k1[pos1] = rk1; v1[pos1] = rv1; w1[pos1] = rw1;
        }
    }
}

// Query 102's front, a kernel of its own so that k_flatmap (on q3's measured
// path) stays as it is: bids.map_index(|b| (b.auction, (b.date_time,
// b.price))) with the price kept as the value, v = date_time << 32 | price:
// the input of partitioned_rolling_aggregate(Max | Min).  A date_time or
// price that does not fit its half of v goes out under a partition >= 2^32,
// which the operator's precondition rejects.  One stream; counter and
// capacity as k_flatmap's stream 0 (block_append2 numbers both streams and
// leaves the counter of one without a match alone).
__global__ __launch_bounds__(FLATMAP_BLK) void k_flatmap_bid_tv(
        const dbsp_event *ev, dbspk::EventCols cols, int64_t n, uint64_t *c0,
        uint64_t *k0, uint64_t *v0, int64_t *w0, int64_t cap0, uint64_t *c1) {
    __shared__ uint32_t s_cnt[2][FLATMAP_WAVES];
    __shared__ unsigned long long s_base[2][FLATMAP_WAVES];
    const int64_t stride = (int64_t)gridDim.x * FLATMAP_BLK;
    for (int64_t base = blockIdx.x * (int64_t)FLATMAP_BLK; base < n;
         base += stride) {
        const int64_t i = base + threadIdx.x;
        uint64_t kind = 0, auction = 0, price = 0, dt = 0;
        int64_t w = 0;
        if (i < n) {
            if (cols.kind) {
                kind = cols.kind[i]; auction = cols.f0[i]; price = cols.f2[i];
                dt = cols.f3[i]; w = cols.w[i];
            } else {
                const dbsp_event e = ev[i];
                kind = e.kind; auction = e.f0; price = e.f2; dt = e.f3;
                w = e.w;
            }
        }
        const bool p0 = i < n && kind == 2;
        uint64_t pos0, pos1;
        block_append2((unsigned long long *)c0, (unsigned long long *)c1, p0,
                      false, s_cnt, s_base, pos0, pos1);
        if (p0 && pos0 < (uint64_t)cap0) {
            k0[pos0] = ((price | dt) >> 32) ? ~0ull : auction;
            v0[pos0] = (dt << 32) | (price & 0xFFFFFFFFull);
            w0[pos0] = w;
        }
    }
}

// generic per-row map for the small derived streams (q5/q8):
// mode 0: (k,v) -> (v>>10, (v&0x3FF)<<32 | (k&lo32))  [q8 people_by_id map_index]
// mode 1: (k,v) -> (v, 0)                             [q8 auctions map / q5 windowed-bids map]
// mode 2: (k,v) -> (0, v)                             [q5 map_index ((),count)]
// mode 3: (k,v) -> (v, k)                             [q5 by_count map_index]
// mode 5: (k=auction<<4|cat, v=price) -> (cat, 0) with w' = w*(price<<18|1)
//         [q4 average weigh: one linear pass accumulates (sum<<20)+count
//          exactly — price < 2^27 (price.rs) and count < 2^18]
// mode 6: (k=cat, v=(sum<<18)|count) -> (cat, sum/count)  [q4 average output,
//          integer division as the reference's isize avg (average.rs)]
__global__ void k_map(const uint64_t *k, const uint64_t *v, const int64_t *w,
                      int64_t n, int mode, uint64_t *ok, uint64_t *ov,
                      int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t kk = k[i], vv = v[i];
        uint64_t rk, rv;
        int64_t rw = w[i];
        switch (mode) {
            case 0: rk = vv >> 10; rv = ((vv & 0x3FFull) << 32) | (kk & 0xFFFFFFFFull); break;
            case 1: rk = vv; rv = 0; break;
            case 2: rk = 0; rv = vv; break;
            case 4: {  // weigh (aggregate/mod.rs:297-323): f(k,v)=f64(v); w' = f(k,v)*w
                rk = kk; rv = 0;
                double f = *(const double *)&vv;
                double wp = f * (double)w[i];
                rw = *(const int64_t *)&wp;
                break;
            }
            case 5:
                // (sum<<18)+count packed weight: price <= 10^8 (price.rs),
                // per-category sum <= ~1.2e13 -> sum<<18 < 2^62; count
                // (auctions per category) < 2^18
                rk = kk & 0xFull;
                rv = 0;
                rw = w[i] * (int64_t)((vv << 18) | 1ull);
                break;
            case 6: {
                const int64_t cnt = (int64_t)(vv & 0x3FFFFull);
                rk = kk;
                rv = cnt > 0 ? (vv >> 18) / (uint64_t)cnt : 0;
                break;
            }
            case 7:  // q6 map_index (q6.rs:92-94): winning bids keyed by
                     // seller, val (auction<<20)|price keeps cursor order
                     // by auction id for the last-10 fold
                rk = kk & 0xFFFFFull;
                rv = ((kk >> 20) << 27) | (vv & 0x7FFFFFFull);
                break;
            default: rk = vv; rv = kk; break;
        }
        ok[i] = rk;
        ov[i] = rv;
        ow[i] = rw;
    }
}

// ===========================================================================
// host-side primitive layer (exported via engine.cpp which owns dbsp_ctx);
// the functions below are internal helpers shared with engine.cpp
// ===========================================================================

#include "kernels_iface.hpp"

namespace dbspk {

// ---------------------------------------------------------------------------
// Scoped scratch: device buffers from the big-buffer cache, bound to a stream
// and returned to it in allocation order when the scope ends — on every
// return path, so an error return leaks nothing into the free-list
// accounting.  Result columns are carved through the scope too and stay its
// property until the wrapper hands them over (keep / give_rows).
// ---------------------------------------------------------------------------
class Scratch {
  public:
    explicit Scratch(hipStream_t s) : s_(s) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() {
        for (int i = 0; i < n_; i++) (void)cache_free(p_[i], s_);
    }
    template <typename T>
    hipError_t get(T **out, size_t bytes) {
        if (n_ == CAP) return hipErrorOutOfMemory;
        hipError_t e = cache_malloc((void **)out, bytes, s_);
        if (e == hipSuccess) p_[n_++] = *out;
        return e;
    }
    // free p now: an early release that later allocations count on
    hipError_t release(void *p) { return cache_free(take(p), s_); }
    // the caller owns p from here on
    void keep(void *p) { (void)take(p); }
    hipStream_t stream() const { return s_; }

  private:
    void *take(void *p) {
        for (int i = 0; i < n_; i++)
            if (p_[i] == p) p_[i] = nullptr;
        return p;
    }
    // the most: truncate_spine's counts plus three columns per spine batch
    static constexpr int CAP = 3 * MAX_TRACE_BATCHES + 8;
    hipStream_t s_;
    void *p_[CAP];
    int n_ = 0;
};

// the result carve: three columns of n rows (8 B pad each), the scope's until
// give_rows
static dbsp_status alloc_rows(Scratch &sc, int64_t n, Rows *r) {
    HIP_CHECK(sc.get(&r->k, n * sizeof(uint64_t) + 8));
    HIP_CHECK(sc.get(&r->v, n * sizeof(uint64_t) + 8));
    HIP_CHECK(sc.get(&r->w, n * sizeof(int64_t) + 8));
    r->n = n;
    return DBSP_OK;
}
// success: the caller takes r's columns
static dbsp_status give_rows(Scratch &sc, const Rows &r, Rows *out) {
    sc.keep(r.k);
    sc.keep(r.v);
    sc.keep(r.w);
    *out = r;
    return DBSP_OK;
}
// the empty result
static dbsp_status no_rows(Rows *out) {
    *out = Rows{};
    return DBSP_OK;
}

dbsp_status scan_excl(hipStream_t s, const uint64_t *in, uint64_t *out,
                      int64_t n, uint64_t *h_total) {
    return scan_exclusive(s, in, out, n, h_total);
}

void fill_u64(hipStream_t s, uint64_t *p, uint64_t v, int64_t n) {
    k_fill_u64<<<grid_for(n), BLK, 0, s>>>(p, v, n);
}

// ---------------------------------------------------------------------------
// C5 synthetic operand generator (BASELINE configs[4]: 1B-row OrdIndexedZSet
// x 10M-row delta).  Counter-based splitmix64 keeps keys strictly increasing
// by construction (k_i = stride*i + h(i) % jitter, jitter < stride), so the
// generated batch is sorted-unique with no device scan or sort — the trace
// never stages through the host (24 GB at 1B rows).
// ---------------------------------------------------------------------------

__device__ __host__ inline uint64_t c5_mix(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void k_c5_gen(int64_t n, uint64_t stride, uint64_t jitter,
                         uint64_t seed, int val_mode, uint64_t *k, uint64_t *v,
                         int64_t *w) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += gridDim.x * (int64_t)blockDim.x) {
        const uint64_t h = c5_mix(seed + (uint64_t)i * 0x9E3779B97F4A7C15ull);
        k[i] = stride * (uint64_t)i + (jitter ? h % jitter : 0);
        if (val_mode == 0) {
            // uniform f64 in [0,1) as bit pattern (f64 vals)
            const double u = (double)(c5_mix(h) >> 11) * 0x1.0p-53;
            v[i] = __double_as_longlong(u);
        } else {
            v[i] = 0;
        }
        w[i] = 1;
    }
}

dbsp_status c5_gen_rows(hipStream_t s, const Rows &out, uint64_t stride,
                        uint64_t jitter, uint64_t seed, int val_mode) {
    if (out.n <= 0) return DBSP_OK;
    k_c5_gen<<<grid_for(out.n), BLK, 0, s>>>(out.n, stride, jitter, seed,
                                             val_mode, out.k, out.v, out.w);
    return DBSP_OK;
}

// sort rows by (k major, v minor); ping-pong scratch must hold rows.n rows.
// Skips byte passes above the significant bytes of max(k)/max(v).
dbsp_status sort_rows(hipStream_t s, const Rows &rows, const Rows &scratch,
                      bool *result_in_scratch) {
    *result_in_scratch = false;
    const int64_t n = rows.n;
    if (n <= 1) return DBSP_OK;
    // significant bytes from max values
    uint64_t h_max[4];
    {
        // its own scope: d_max is back in the list before counts is carved
        Scratch sc(s);
        uint64_t *d_max;
        HIP_CHECK(sc.get(&d_max, 4 * sizeof(uint64_t)));
        HIP_CHECK(hipMemsetAsync(d_max, 0, 2 * sizeof(uint64_t), s));
        HIP_CHECK(hipMemsetAsync(d_max + 2, 0xFF, 2 * sizeof(uint64_t), s));
        k_minmax_u64<<<grid_for(n), BLK, 0, s>>>(rows.k, rows.v, n, d_max);
        HIP_CHECK(hipMemcpyAsync(h_max, d_max, 4 * sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    const uint64_t kbase = h_max[2], vbase = h_max[3];
    const uint64_t krange = h_max[0] - kbase, vrange = h_max[1] - vbase;
    int kbytes = 0, vbytes = 0;
    while (kbytes < 8 && (krange >> (8 * kbytes)) != 0) kbytes++;
    while (vbytes < 8 && (vrange >> (8 * vbytes)) != 0) vbytes++;

    int64_t nblocks = ceil_div(n, SORT_TILE);
    Scratch sc(s);
    uint64_t *counts;
    HIP_CHECK(sc.get(&counts, (int64_t)256 * nblocks * sizeof(uint64_t)));

    Rows src = rows, dst = scratch;
    for (int byte = 0; byte < 16; byte++) {
        bool is_v = byte < 8;
        if (is_v && (byte & 7) >= vbytes) continue;
        if (!is_v && (byte & 7) >= kbytes) continue;
        k_radix_hist<<<dim3((uint32_t)nblocks), BLK, 0, s>>>(
            src.k, src.v, n, byte, kbase, vbase, nblocks, counts);
        TRY_K(scan_exclusive(s, counts, counts, 256 * nblocks, nullptr));
        k_radix_scatter<<<dim3((uint32_t)nblocks), BLK, 0, s>>>(
            src.k, src.v, src.w, n, byte, kbase, vbase, nblocks, counts, dst.k,
            dst.v, dst.w);
        std::swap(src, dst);
    }
    *result_in_scratch = (src.k != rows.k);
    return DBSP_OK;
}

// consolidate SORTED rows into freshly allocated output; returns exact length.
// The segment reduction is the weight type's: i64 sums with atomics; f64 runs
// the deterministic segmented tree IN PLACE over in.w (position-fixed order;
// tolerance 2 ulp * ceil(log2 run) vs sequential).
dbsp_status consolidate_sorted(hipStream_t s, const Rows &in, bool wf64,
                               Rows *out) {
    const int64_t n = in.n;
    if (n == 0) return no_rows(out);
    Scratch sc(s);
    uint64_t *flags, *fscan;
    HIP_CHECK(sc.get(&flags, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, n * sizeof(uint64_t)));
    k_head_flags<<<grid_for(n), BLK, 0, s>>>(in.k, in.v, n, flags);
    uint64_t nseg = 0;
    TRY_K(scan_exclusive(s, flags, fscan, n, &nseg));
    Rows seg;
    TRY_K(alloc_rows(sc, (int64_t)nseg, &seg));
    if (wf64) {
        uint64_t *hp;
        double *ww = (double *)in.w;
        HIP_CHECK(sc.get(&hp, nseg * sizeof(uint64_t) + 8));
        k_seg_headpos<<<grid_for(n), BLK, 0, s>>>(flags, fscan, n, hp);
        for (int64_t d = 1; d < n; d <<= 1)
            k_seg_tree_round<<<grid_for(n), BLK, 0, s>>>(ww, flags, fscan, hp,
                                                         n, d);
        k_seg_collect_f64<<<grid_for(n), BLK, 0, s>>>(
            in.k, in.v, ww, flags, fscan, n, seg.k, seg.v, (double *)seg.w);
    } else {
        HIP_CHECK(hipMemsetAsync(seg.w, 0, nseg * sizeof(int64_t), s));
        k_seg_accum<<<grid_for(n), BLK, 0, s>>>(in.k, in.v, in.w, fscan, flags,
                                                n, seg.k, seg.v, seg.w);
    }
    // drop zero-weight segments
    uint64_t *nzflags, *nzscan;
    HIP_CHECK(sc.get(&nzflags, nseg * sizeof(uint64_t) + 8));
    HIP_CHECK(sc.get(&nzscan, nseg * sizeof(uint64_t) + 8));
    if (wf64)
        k_nonzero_flags<double><<<grid_for(nseg), BLK, 0, s>>>(
            (const double *)seg.w, nseg, nzflags);
    else
        k_nonzero_flags<int64_t><<<grid_for(nseg), BLK, 0, s>>>(seg.w, nseg,
                                                                nzflags);
    uint64_t nout = 0;
    TRY_K(scan_exclusive(s, nzflags, nzscan, nseg, &nout));
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)nout, &r));
    // k_compact copies the weight column bitwise (8 B) — valid for f64
    k_compact<<<grid_for(nseg), BLK, 0, s>>>(seg.k, seg.v, seg.w, nzflags,
                                             nzscan, nseg, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

template <typename W>
static dbsp_status merge_rows_t(hipStream_t s, const Rows &a, const Rows &b,
                                Rows *out) {
    const uint64_t *ak = a.k, *av = a.v, *bk = b.k, *bv = b.v;
    const W *aw = (const W *)a.w, *bw = (const W *)b.w;
    const int64_t na = a.n, nb = b.n;
    int64_t total = na + nb;
    if (total == 0) return no_rows(out);
    // Default: two-pass count -> device scan -> emit (k_mp_merge_onepass
    // modes 1+2 — branchless capture walk in both phases).  The single-pass
    // decoupled-lookback variant (mode 0) reads each input byte once but its
    // lookback protocol measures SLOWER than the count re-read at 1B rows
    // (granule-load throughput-bound; see the kernel comment) — opt in with
    // DBSP_MERGE_ONEPASS=1; a poisoned lookback falls back to two-pass.
    static const bool twopass = []() {
        const char *e = getenv("DBSP_MERGE_ONEPASS");
        return !(e && e[0] == '1');
    }();
    static const int op_tile = []() {
        const char *e = getenv("DBSP_MERGE_OP_TILE");
        return (e && atoi(e) == 2048) ? 2048 : MP_TILE;
    }();
    const int64_t tile = op_tile;
    int64_t nblocks = ceil_div(total, tile);
    Scratch sc(s);
    int64_t *pa, *pb;
    HIP_CHECK(sc.get(&pa, (nblocks + 1) * sizeof(int64_t)));
    HIP_CHECK(sc.get(&pb, (nblocks + 1) * sizeof(int64_t)));
    k_mp_partition<<<grid_for(nblocks + 1), BLK, 0, s>>>(ak, av, na, bk, bv, nb,
                                                         nblocks, tile, pa, pb);
    Rows r;
    const dim3 g((uint32_t)nblocks);
    if (!twopass) {
        unsigned long long *state;
        HIP_CHECK(sc.get(&state, (nblocks + 2) * sizeof(uint64_t)));
        HIP_CHECK(hipMemsetAsync(state, 0, (nblocks + 2) * sizeof(uint64_t), s));
        TRY_K(alloc_rows(sc, total, &r));
        const size_t smem = 3 * (tile + 2) * sizeof(uint64_t);
        if (tile == 2048)
            k_mp_merge_onepass<W, 2048, 0><<<g, MP_THREADS, smem, s>>>(
                ak, av, aw, na, bk, bv, bw, nb, pa, pb, state, nblocks, r.k,
                r.v, (W *)r.w);
        else
            k_mp_merge_onepass<W, MP_TILE, 0><<<g, MP_THREADS, smem, s>>>(
                ak, av, aw, na, bk, bv, bw, nb, pa, pb, state, nblocks, r.k,
                r.v, (W *)r.w);
        unsigned long long h_state[2];
        HIP_CHECK(hipMemcpyAsync(&h_state[0], state + 1, sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&h_state[1], state + 2 + (nblocks - 1),
                                 sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        // early: state is back in the list before the fall-back path carves
        HIP_CHECK(sc.release(state));
        if (h_state[0] == 0 && (h_state[1] & 3ull) == 2ull) {
            r.n = (int64_t)(h_state[1] >> 2);
            return give_rows(sc, r, out);
        }
        // poisoned lookback: free the optimistic buffers and fall through to
        // the two-pass pipeline on the partitions already computed
        (void)sc.release(r.k);
        (void)sc.release(r.v);
        (void)sc.release(r.w);
    }
    uint64_t *counts;
    HIP_CHECK(sc.get(&counts, (nblocks + 1) * sizeof(uint64_t)));
    const size_t smem_count = 2 * (tile + 2) * sizeof(uint64_t);
    if (tile == 2048)
        k_mp_merge_onepass<W, 2048, 1><<<g, MP_THREADS, smem_count, s>>>(
            ak, av, aw, na, bk, bv, bw, nb, pa, pb,
            (unsigned long long *)counts, nblocks, nullptr, nullptr, nullptr);
    else
        k_mp_merge_onepass<W, MP_TILE, 1><<<g, MP_THREADS, smem_count, s>>>(
            ak, av, aw, na, bk, bv, bw, nb, pa, pb,
            (unsigned long long *)counts, nblocks, nullptr, nullptr, nullptr);
    uint64_t nout = 0;
    TRY_K(scan_exclusive(s, counts, counts, nblocks, &nout));
    TRY_K(alloc_rows(sc, (int64_t)nout, &r));
    const size_t smem_emit = 3 * (tile + 2) * sizeof(uint64_t);
    if (nout > 0) {
        if (tile == 2048)
            k_mp_merge_onepass<W, 2048, 2><<<g, MP_THREADS, smem_emit, s>>>(
                ak, av, aw, na, bk, bv, bw, nb, pa, pb,
                (unsigned long long *)counts, nblocks, r.k, r.v, (W *)r.w);
        else
            k_mp_merge_onepass<W, MP_TILE, 2><<<g, MP_THREADS, smem_emit, s>>>(
                ak, av, aw, na, bk, bv, bw, nb, pa, pb,
                (unsigned long long *)counts, nblocks, r.k, r.v, (W *)r.w);
    }
    return give_rows(sc, r, out);
}

dbsp_status merge_rows(hipStream_t s, const Rows &a, const Rows &b, bool wf64,
                       Rows *out) {
    return wf64 ? merge_rows_t<double>(s, a, b, out)
                : merge_rows_t<int64_t>(s, a, b, out);
}

dbsp_status minmax_rows(hipStream_t s, const Rows &rows, uint64_t mm[4]) {
    Scratch sc(s);
    unsigned long long *d;
    HIP_CHECK(sc.get(&d, 4 * sizeof(uint64_t)));
    const unsigned long long init[4] = {~0ull, ~0ull, 0ull, 0ull};
    HIP_CHECK(hipMemcpyAsync(d, init, sizeof(init), hipMemcpyHostToDevice, s));
    // cap the grid: each block ends with 8 global atomics on 4 hot words,
    // and a full grid_for() grid serializes ~15 us on them alone
    k_minmax_rows<<<dim3(std::min(grid_for(rows.n).x, 64u)), BLK, 0, s>>>(
        rows.k, rows.v, rows.n, d);
    HIP_CHECK(hipMemcpyAsync(mm, d, 4 * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return DBSP_OK;
}

// chained variant: n read from the device, results left in mm_dev[0..3]
// (caller reads them at its own sync); grid sized by the capacity bound
dbsp_status minmax_rows_chain(hipStream_t s, const Rows &rows,
                              const int64_t *n_dev,
                              unsigned long long *mm_dev) {
    const unsigned long long init[4] = {~0ull, ~0ull, 0ull, 0ull};
    HIP_CHECK(hipMemcpyAsync(mm_dev, init, sizeof(init), hipMemcpyHostToDevice,
                             s));
    k_minmax_rows<<<dim3(std::min(grid_for(rows.n).x, 64u)), BLK, 0, s>>>(
        rows.k, rows.v, 0, mm_dev, n_dev);
    return DBSP_OK;
}

// the dense consolidates' shared front: weights into the kspan*vspan
// histogram, cell flags scanned in place (total to *h_total if asked: a sync)
static dbsp_status dense_hist(Scratch &sc, const Rows &in, uint64_t kbase,
                              uint64_t vbase, int64_t vspan, int64_t r,
                              unsigned long long **wbuf, uint64_t **flags,
                              uint64_t *h_total) {
    hipStream_t s = sc.stream();
    HIP_CHECK(sc.get(wbuf, r * sizeof(uint64_t)));
    HIP_CHECK(sc.get(flags, (r + 1) * sizeof(uint64_t)));
    HIP_CHECK(hipMemsetAsync(*wbuf, 0, r * sizeof(uint64_t), s));
    k_hist_add<<<grid_for(in.n), BLK, 0, s>>>(in.k, in.v, in.w, in.n, kbase,
                                              vbase, (uint64_t)vspan, *wbuf);
    k_hist_flags<<<grid_for(r), BLK, 0, s>>>(*wbuf, r, *flags);
    return scan_exclusive(s, *flags, *flags, r, h_total);
}

// chained variant: no host sync — the consolidated length lands in
// *out_n_dev for the caller's one tick sync (the emit grid covers the whole
// histogram range, so nothing here needs the total on the host)
dbsp_status sort_cons_dense_chain(hipStream_t s, const Rows &in,
                                  uint64_t kbase, uint64_t vbase,
                                  int64_t kspan, int64_t vspan,
                                  const Rows &out, int64_t *out_n_dev) {
    const int64_t r = kspan * vspan;
    Scratch sc(s);
    unsigned long long *wbuf;
    uint64_t *flags;
    TRY_K(dense_hist(sc, in, kbase, vbase, vspan, r, &wbuf, &flags, nullptr));
    k_hist_total<<<1, 1, 0, s>>>(wbuf, flags, r, out_n_dev);
    k_hist_emit<<<grid_for(r), BLK, 0, s>>>(wbuf, flags, r, kbase, vbase,
                                            (uint64_t)vspan, out.k, out.v,
                                            out.w);
    return DBSP_OK;
}

dbsp_status sort_cons_dense(hipStream_t s, const Rows &in, uint64_t kbase,
                            uint64_t vbase, int64_t kspan, int64_t vspan,
                            Rows *out) {
    const int64_t r = kspan * vspan;
    Scratch sc(s);
    unsigned long long *wbuf;
    uint64_t *flags;
    uint64_t nout = 0;
    TRY_K(dense_hist(sc, in, kbase, vbase, vspan, r, &wbuf, &flags, &nout));
    if (nout > 0)
        k_hist_emit<<<grid_for(r), BLK, 0, s>>>(wbuf, flags, r, kbase, vbase,
                                                (uint64_t)vspan, out->k,
                                                out->v, out->w);
    out->n = (int64_t)nout;
    return DBSP_OK;
}

dbsp_status sort_cons_small_batch(hipStream_t s, const SortArgs &args,
                                  bool wf64) {
    for (int b = 0; b < args.nb; b++)
        if (args.n[b] > FUSE_MAX) return DBSP_ERR_INVALID;
    if (args.nb == 0) return DBSP_OK;
    const dim3 grid((uint32_t)args.nb);
    if (wf64)
        k_sort_cons_small<double><<<grid, FUSE_THREADS, 0, s>>>(args);
    else
        k_sort_cons_small<int64_t><<<grid, FUSE_THREADS, 0, s>>>(args);
    return DBSP_OK;
}

dbsp_status merge_small_batch(hipStream_t s, const MergeArgs &args,
                              bool wf64) {
    if (args.np == 0) return DBSP_OK;
    for (int i = 0; i < args.np; i++)
        if (args.na[i] + args.nb[i] > 4 * FUSE_MAX) return DBSP_ERR_INVALID;
    const dim3 grid((uint32_t)args.np);
    if (wf64)
        k_merge_small<double><<<grid, FUSE_THREADS, 0, s>>>(args);
    else
        k_merge_small<int64_t><<<grid, FUSE_THREADS, 0, s>>>(args);
    return DBSP_OK;
}

// launch generation for the fused barrier's tagged counts — shared across
// the int64/f64 instantiations so two launchers can never reuse a tag the
// other just published into the same scratch
static std::atomic<uint32_t> g_mid_gen{0};

dbsp_status merge_mid_batch(hipStream_t s, const MergeArgs &args,
                            int64_t *scratch, bool wf64) {
    if (args.np == 0) return DBSP_OK;
    const uint32_t gen = ++g_mid_gen;
    dim3 grid(MERGE_MID_WGS, (uint32_t)args.np);
    if (wf64)
        k_merge_mid_fused<double><<<grid, FUSE_THREADS, 0, s>>>(args, scratch,
                                                                gen);
    else
        k_merge_mid_fused<int64_t><<<grid, FUSE_THREADS, 0, s>>>(args, scratch,
                                                                 gen);
    return DBSP_OK;
}

dbsp_status acc_fold_batch(hipStream_t s, const MergeArgs &args, bool wf64) {
    if (args.np == 0) return DBSP_OK;
    if (args.np < 0 || args.np > MERGE_BATCH_MAX) return DBSP_ERR_INVALID;
    MergeArgs a = args;
    int wgs = 1;
    for (int i = 0; i < a.np; i++) {
        if (a.na[i] < 0 || a.na[i] > ACC_FOLD_NA_MAX) return DBSP_ERR_INVALID;
        if (!a.dnb[i]) {
            if (a.nb[i] < 0 || a.nb[i] > FUSE_MAX) return DBSP_ERR_INVALID;
            a.bcap[i] = a.nb[i];
        } else if (a.bcap[i] < 0) {
            return DBSP_ERR_INVALID;
        }
        wgs = std::max(wgs, acc_fold_wgs(a.na[i]));
    }
    const dim3 grid((uint32_t)wgs, (uint32_t)a.np);
    if (wf64)
        k_acc_fold<double><<<grid, FUSE_THREADS, 0, s>>>(a);
    else
        k_acc_fold<int64_t><<<grid, FUSE_THREADS, 0, s>>>(a);
    return DBSP_OK;
}

dbsp_status join_spine_rows(hipStream_t s, const Rows &delta,
                            const TraceArgs &t, int proj, uint64_t param,
                            Rows *out) {
    const int64_t nd = delta.n;
    if (nd == 0 || t.nb == 0) return no_rows(out);
    Scratch sc(s);
    uint32_t *cnts;
    uint64_t *counts;
    HIP_CHECK(sc.get(&cnts, (int64_t)nd * t.nb * sizeof(uint32_t) + 8));
    HIP_CHECK(sc.get(&counts, (nd + 1) * sizeof(uint64_t)));
    k_join_count_multi<<<grid_for(nd), BLK, 0, s>>>(delta.k, nd, t, cnts,
                                                    counts);
    uint64_t nout = 0;
    TRY_K(scan_exclusive(s, counts, counts, nd, &nout));
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)nout, &r));
    if (nout > 0)
        k_join_emit_multi<<<grid_for((int64_t)nout), BLK, 0, s>>>(
            delta.k, delta.v, delta.w, nd, t, cnts, counts, (int64_t)nout,
            proj, param, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

dbsp_status join_probe_batch(hipStream_t s, const JoinCountArgs &args) {
    if (args.np == 0) return DBSP_OK;
    for (int i = 0; i < args.np; i++)
        if (args.nd[i] > FUSE_MAX) return DBSP_ERR_INVALID;
    k_join_probe_multi<<<dim3((uint32_t)(args.np * JPROBE_BLOCKS)), BLK, 0,
                         s>>>(args);
    return DBSP_OK;
}

dbsp_status join_count_scan_batch(hipStream_t s, const JoinCountArgs &args) {
    if (args.np == 0) return DBSP_OK;
    TRY_K(join_probe_batch(s, args));
    k_join_scan_small<<<dim3((uint32_t)args.np), FUSE_THREADS, 0, s>>>(args);
    return DBSP_OK;
}

dbsp_status join_tail_small(hipStream_t s, const JoinTailArgs &a) {
    if (a.np < 0 || a.np > 3 || a.cap < FUSE_MAX) return DBSP_ERR_INVALID;
    k_join_tail_small<<<1, FUSE_THREADS, 0, s>>>(a);
    return DBSP_OK;
}

dbsp_status join_emit_prepared(hipStream_t s, const Rows &delta,
                               const TraceArgs &t, const uint32_t *cnts,
                               const uint64_t *offsets, int64_t n_out,
                               int proj, uint64_t param, const Rows &out) {
    if (n_out > 0)
        k_join_emit_multi<<<grid_for(n_out), BLK, 0, s>>>(
            delta.k, delta.v, delta.w, delta.n, t, cnts, offsets, n_out, proj,
            param, out.k, out.v, out.w);
    return DBSP_OK;
}

dbsp_status join_rows(hipStream_t s, const Rows &delta, const Rows &trace,
                      int proj, uint64_t param, Rows *out) {
    const int64_t nd = delta.n;
    if (nd == 0 || trace.n == 0) return no_rows(out);
    Scratch sc(s);
    uint64_t *counts, *starts;
    HIP_CHECK(sc.get(&counts, (nd + 1) * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&starts, nd * sizeof(uint64_t)));
    k_join_count<<<grid_for(nd), BLK, 0, s>>>(delta.k, nd, trace.k, trace.n,
                                              counts, starts);
    uint64_t nout = 0;
    TRY_K(scan_exclusive(s, counts, counts, nd, &nout));
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)nout, &r));
    if (nout > 0)
        k_join_emit<<<grid_for((int64_t)nout), BLK, 0, s>>>(
            delta.k, delta.v, delta.w, nd, trace.v, trace.w, counts, starts,
            (int64_t)nout, proj, param, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

template <int MODE>
static dbsp_status agg_upsert_impl(hipStream_t s, const uint64_t *keys,
                                   int64_t nd, const Rows &in,
                                   const Rows &out_trace, Rows *out) {
    if (nd == 0) return no_rows(out);
    Scratch sc(s);
    uint64_t *counts, *istart, *ostart, *newval, *hasnew, *offsets;
    HIP_CHECK(sc.get(&counts, nd * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&istart, nd * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&ostart, nd * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&newval, nd * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&hasnew, nd * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&offsets, nd * sizeof(uint64_t)));
    k_agg_count<MODE><<<grid_for(nd), BLK, 0, s>>>(
        keys, nd, in.k, in.w, in.n, out_trace.k, out_trace.n, counts, istart,
        ostart, newval, hasnew);
    uint64_t nout = 0;
    TRY_K(scan_exclusive(s, counts, offsets, nd, &nout));
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)nout, &r));
    if (nout > 0)
        k_agg_emit<MODE><<<grid_for(nd), BLK, 0, s>>>(
            keys, nd, in.v, out_trace.v, out_trace.w, offsets, counts, istart,
            ostart, newval, hasnew, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

dbsp_status agg_upsert_rows(hipStream_t s, AggMode mode, const uint64_t *keys,
                            int64_t nd, const Rows &in, const Rows &out_trace,
                            Rows *out) {
    switch (mode) {
    case AGG_LINEAR:
        return agg_upsert_impl<AGG_LINEAR>(s, keys, nd, in, out_trace, out);
    case AGG_MAX:
        return agg_upsert_impl<AGG_MAX>(s, keys, nd, in, out_trace, out);
    case AGG_LAST10:
        return agg_upsert_impl<AGG_LAST10>(s, keys, nd, in, out_trace, out);
    }
    return DBSP_ERR_INVALID;
}

dbsp_status distinct_inc_rows(hipStream_t s, const Rows &delta,
                              const TraceArgs &t, Rows *out) {
    const int64_t nd = delta.n;
    if (nd == 0) return no_rows(out);
    Scratch sc(s);
    uint64_t *flags, *fscan;
    int64_t *outw;
    HIP_CHECK(sc.get(&flags, nd * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, nd * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&outw, nd * sizeof(int64_t)));
    k_distinct_count<<<grid_for(nd), BLK, 0, s>>>(delta.k, delta.v, delta.w,
                                                  nd, t, flags, outw);
    uint64_t nout = 0;
    TRY_K(scan_exclusive(s, flags, fscan, nd, &nout));
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)nout, &r));
    k_compact<<<grid_for(nd), BLK, 0, s>>>(delta.k, delta.v, outw, flags,
                                           fscan, nd, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

dbsp_status window_ranges_multi(hipStream_t s, const TraceArgs &t,
                                const uint64_t *bk, int64_t bn, int have_prev,
                                uint64_t s0, uint64_t e0, uint64_t s1,
                                uint64_t e1, int64_t *table, int64_t *d_total) {
    k_window_ranges_multi<<<1, BLK, 0, s>>>(t, bk, bn, have_prev, s0, e0, s1,
                                            e1, table, d_total, nullptr,
                                            nullptr);
    return DBSP_OK;
}

dbsp_status wm_update(hipStream_t s, const WmSource &src, uint64_t width,
                      uint64_t tumble, uint64_t lag, unsigned long long *state,
                      unsigned long long *bounds) {
    k_wm_update<<<1, 1, 0, s>>>(src, width, tumble, lag, state, bounds);
    return DBSP_OK;
}

dbsp_status window_ranges_chain(hipStream_t s, const TraceArgs &t,
                                const uint64_t *bk, int64_t bn,
                                const int64_t *bn_dev,
                                const unsigned long long *bounds,
                                int64_t *table, int64_t *d_total) {
    k_window_ranges_multi<<<1, BLK, 0, s>>>(t, bk, bn, 0, 0, 0, 0, 0, table,
                                            d_total, bn_dev, bounds);
    return DBSP_OK;
}

dbsp_status window_emit_multi(hipStream_t s, const TraceArgs &t,
                              const Rows &batch, const int64_t *table,
                              int nreg, int64_t total, const Rows &out) {
    if (total > 0)
        k_window_emit_multi<<<grid_for(total), BLK, 0, s>>>(
            t, batch.k, batch.v, batch.w, table, nreg, total, out.k, out.v,
            out.w);
    return DBSP_OK;
}

dbsp_status shard_rows(hipStream_t s, const Rows &in, int nshards,
                       const Rows &out, int64_t *h_offsets) {
    const int64_t n = in.n;
    Scratch sc(s);
    uint64_t *hist;
    HIP_CHECK(sc.get(&hist, (nshards + 1) * sizeof(uint64_t)));
    HIP_CHECK(hipMemsetAsync(hist, 0, (nshards + 1) * sizeof(uint64_t), s));
    if (n > 0) k_shard_hist<<<grid_for(n), BLK, 0, s>>>(in.k, n, nshards, hist);
    uint64_t h_hist[64];
    HIP_CHECK(hipMemcpyAsync(h_hist, hist, nshards * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    int64_t acc = 0;
    for (int i = 0; i < nshards; i++) {
        h_offsets[i] = acc;
        acc += (int64_t)h_hist[i];
    }
    h_offsets[nshards] = acc;
    // cursor initialised to shard starts
    HIP_CHECK(hipMemcpyAsync(hist, h_offsets, nshards * sizeof(int64_t),
                             hipMemcpyHostToDevice, s));
    if (n > 0)
        k_shard_scatter<<<grid_for(n), BLK, 0, s>>>(in.k, in.v, in.w, n,
                                                    nshards, hist, out.k,
                                                    out.v, out.w);
    return DBSP_OK;
}

// pair variant: both deltas' histograms land in one readback, so the
// exchange pays ONE partition sync instead of two
dbsp_status shard_rows_pair(hipStream_t s, const Rows &in0, const Rows &in1,
                            int nshards, const Rows &out0, const Rows &out1,
                            int64_t *h_off0, int64_t *h_off1) {
    const int64_t n0 = in0.n, n1 = in1.n;
    Scratch sc(s);
    uint64_t *hist;
    HIP_CHECK(sc.get(&hist, 2 * (nshards + 1) * sizeof(uint64_t)));
    HIP_CHECK(hipMemsetAsync(hist, 0, 2 * (nshards + 1) * sizeof(uint64_t), s));
    uint64_t *hist1 = hist + nshards + 1;
    if (n0 > 0)
        k_shard_hist<<<grid_for(n0), BLK, 0, s>>>(in0.k, n0, nshards, hist);
    if (n1 > 0)
        k_shard_hist<<<grid_for(n1), BLK, 0, s>>>(in1.k, n1, nshards, hist1);
    uint64_t h_hist[130];
    HIP_CHECK(hipMemcpyAsync(h_hist, hist, sizeof(h_hist[0]) * (nshards + 1),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_hist + 65, hist1,
                             sizeof(h_hist[0]) * (nshards + 1),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    int64_t acc0 = 0, acc1 = 0;
    int64_t cur[130];
    for (int i = 0; i < nshards; i++) {
        h_off0[i] = acc0;
        h_off1[i] = acc1;
        cur[i] = acc0;
        cur[65 + i] = acc1;
        acc0 += (int64_t)h_hist[i];
        acc1 += (int64_t)h_hist[65 + i];
    }
    h_off0[nshards] = acc0;
    h_off1[nshards] = acc1;
    HIP_CHECK(hipMemcpyAsync(hist, cur, nshards * sizeof(int64_t),
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(hist1, cur + 65, nshards * sizeof(int64_t),
                             hipMemcpyHostToDevice, s));
    if (n0 > 0)
        k_shard_scatter<<<grid_for(n0), BLK, 0, s>>>(
            in0.k, in0.v, in0.w, n0, nshards, hist, out0.k, out0.v, out0.w);
    if (n1 > 0)
        k_shard_scatter<<<grid_for(n1), BLK, 0, s>>>(
            in1.k, in1.v, in1.w, n1, nshards, hist1, out1.k, out1.v, out1.w);
    return DBSP_OK;
}

// ---------------------------------------------------------------------------
// fixed-frame pair exchange (see kernels_iface.hpp FramePairArgs): ONE pack
// kernel + ONE equal-count ncclAllToAll + ONE unpack kernel replace the
// counts-allgather, its host sync, and the ~6*world-call grouped send/recv
// mesh of the dynamic path (r01_q3_shard_kernel_trace.txt attributed the 2x
// sharded-tick cost to exactly that host latency).
// ---------------------------------------------------------------------------

__global__ void k_frames_pack_pair(FramePairArgs a) {
    const int64_t S = 2 + 3 * a.P0 + 3 * a.P1;  // segment words
    const int64_t total = (int64_t)a.world * S;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         x < total; x += gridDim.x * (int64_t)blockDim.x) {
        const int r = (int)(x / S);
        const int64_t q = x % S;
        const int64_t n0 = a.off0[r + 1] - a.off0[r];
        const int64_t n1 = a.off1[r + 1] - a.off1[r];
        uint64_t val = 0;
        if (q == 0) {
            val = (uint64_t)n0;  // true count: > P0 flags sender overflow
        } else if (q == 1) {
            val = (uint64_t)n1;
        } else if (q - 2 < 3 * a.P0) {
            const int64_t p = q - 2;
            const int col = (int)(p / a.P0);
            const int64_t i = p % a.P0;
            if (i < n0 && i < a.P0) {
                const uint64_t *src = col == 0   ? a.p0k
                                      : col == 1 ? a.p0v
                                                 : (const uint64_t *)a.p0w;
                val = src[a.off0[r] + i];
            }
        } else {
            const int64_t p = q - 2 - 3 * a.P0;
            const int col = (int)(p / a.P1);
            const int64_t i = p % a.P1;
            if (i < n1 && i < a.P1) {
                const uint64_t *src = col == 0   ? a.p1k
                                      : col == 1 ? a.p1v
                                                 : (const uint64_t *)a.p1w;
                val = src[a.off1[r] + i];
            }
        }
        a.frame[x] = val;
    }
}

__global__ void k_frames_unpack_pair(const uint64_t *frame, int world,
                                     int64_t P0, int64_t P1, uint64_t *r0k,
                                     uint64_t *r0v, int64_t *r0w,
                                     uint64_t *r1k, uint64_t *r1v,
                                     int64_t *r1w, int64_t *d_tot0,
                                     int64_t *d_tot1) {
    const int64_t S = 2 + 3 * P0 + 3 * P1;
    // per-thread recompute of the <=8 headers (cached) + prefixes
    int64_t c0[8], c1[8], pre0[9], pre1[9];
    bool lost = false;
    pre0[0] = 0;
    pre1[0] = 0;
    for (int r = 0; r < world; r++) {
        c0[r] = (int64_t)frame[(int64_t)r * S];
        c1[r] = (int64_t)frame[(int64_t)r * S + 1];
        if (c0[r] > P0 || c1[r] > P1 || c0[r] < 0 || c1[r] < 0) lost = true;
        pre0[r + 1] = pre0[r] + (lost ? 0 : c0[r]);
        pre1[r + 1] = pre1[r] + (lost ? 0 : c1[r]);
    }
    if (lost) {
        // sender overflow somewhere: publish the sentinel; every rank sees
        // its own copy at the next sync and replays the dynamic exchange
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            *d_tot0 = -1;
            *d_tot1 = -1;
        }
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *d_tot0 = pre0[world];
        *d_tot1 = pre1[world];
    }
    const int64_t total = (int64_t)world * S;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         x < total; x += gridDim.x * (int64_t)blockDim.x) {
        const int r = (int)(x / S);
        const int64_t q = x % S;
        if (q < 2) continue;
        if (q - 2 < 3 * P0) {
            const int64_t p = q - 2;
            const int col = (int)(p / P0);
            const int64_t i = p % P0;
            if (i < c0[r]) {
                const uint64_t v = frame[x];
                if (col == 0) r0k[pre0[r] + i] = v;
                else if (col == 1) r0v[pre0[r] + i] = v;
                else r0w[pre0[r] + i] = (int64_t)v;
            }
        } else {
            const int64_t p = q - 2 - 3 * P0;
            const int col = (int)(p / P1);
            const int64_t i = p % P1;
            if (i < c1[r]) {
                const uint64_t v = frame[x];
                if (col == 0) r1k[pre1[r] + i] = v;
                else if (col == 1) r1v[pre1[r] + i] = v;
                else r1w[pre1[r] + i] = (int64_t)v;
            }
        }
    }
}

dbsp_status frames_pack_pair(hipStream_t s, const FramePairArgs &a) {
    const int64_t total = (int64_t)a.world * (2 + 3 * a.P0 + 3 * a.P1);
    k_frames_pack_pair<<<grid_for(total), BLK, 0, s>>>(a);
    return DBSP_OK;
}

// chained shard-to-frames: hash-partition BOTH raw streams straight into the
// frame segments with atomic header tickets — no host offsets, no separate
// partition/pack kernels, lengths read from the device (the chained tick's
// flatmap counters).  A ticket beyond capacity skips the write; the header
// keeps the true count, which the receiving unpack flags as the overflow
// sentinel.
__global__ void k_frames_init_headers(uint64_t *frame, int world, int64_t S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * world) frame[(int64_t)(i / 2) * S + (i & 1)] = 0;
}

__global__ void k_shard_frames_chain(const uint64_t *k0, const uint64_t *v0,
                                     const int64_t *w0, const int64_t *n0_dev,
                                     const uint64_t *k1, const uint64_t *v1,
                                     const int64_t *w1, const int64_t *n1_dev,
                                     int world, int64_t P0, int64_t P1,
                                     uint64_t *frame) {
    const int64_t S = 2 + 3 * P0 + 3 * P1;
    const int64_t n0 = *n0_dev, n1 = *n1_dev;
    const int64_t total = n0 + n1;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         x < total; x += gridDim.x * (int64_t)blockDim.x) {
        const bool s1 = x >= n0;
        const int64_t i = s1 ? x - n0 : x;
        const uint64_t key = s1 ? k1[i] : k0[i];
        const int peer = (int)(dev_xxh3_u64(key, DBSP_HASH_SEED) % world);
        uint64_t *seg = frame + (int64_t)peer * S;
        const int64_t P = s1 ? P1 : P0;
        const int64_t t = (int64_t)atomicAdd(
            (unsigned long long *)(seg + (s1 ? 1 : 0)), 1ull);
        if (t < P) {
            uint64_t *base = seg + 2 + (s1 ? 3 * P0 : 0);
            base[t] = key;
            base[P + t] = s1 ? v1[i] : v0[i];
            base[2 * P + t] = (uint64_t)(s1 ? w1[i] : w0[i]);
        }
    }
}

dbsp_status shard_frames_chain(hipStream_t s, const Rows &in0,
                               const int64_t *n0_dev, const Rows &in1,
                               const int64_t *n1_dev, int world, int64_t P0,
                               int64_t P1, int64_t n_cap, uint64_t *frame) {
    const int64_t S = 2 + 3 * P0 + 3 * P1;
    k_frames_init_headers<<<dim3(1), dim3(64), 0, s>>>(frame, world, S);
    k_shard_frames_chain<<<grid_for(n_cap > 0 ? n_cap : 1), BLK, 0, s>>>(
        in0.k, in0.v, in0.w, n0_dev, in1.k, in1.v, in1.w, n1_dev, world, P0,
        P1, frame);
    return DBSP_OK;
}

dbsp_status frames_unpack_pair(hipStream_t s, const uint64_t *frame,
                               int world, int64_t P0, int64_t P1,
                               const Rows &r0, const Rows &r1,
                               int64_t *d_tot0, int64_t *d_tot1) {
    const int64_t total = (int64_t)world * (2 + 3 * P0 + 3 * P1);
    k_frames_unpack_pair<<<grid_for(total), BLK, 0, s>>>(
        frame, world, P0, P1, r0.k, r0.v, r0.w, r1.k, r1.v, r1.w, d_tot0,
        d_tot1);
    return DBSP_OK;
}

dbsp_status columnize_events(hipStream_t s, const dbsp_event *ev, int64_t n,
                             uint64_t *kind, uint64_t *f0, uint64_t *f1,
                             uint64_t *f2, uint64_t *f3, uint64_t *f4,
                             int64_t *w) {
    if (n > 0)
        k_columnize<<<grid_for(n), BLK, 0, s>>>(ev, n, kind, f0, f1, f2, f3,
                                                f4, w);
    return DBSP_OK;
}

// query 19's front, defined with the top-K kernels below
__global__ __launch_bounds__(FLATMAP_BLK) void k_flatmap_bid_topk(
        const dbsp_event *ev, dbspk::EventCols cols, int64_t n, uint64_t *c0,
        uint64_t *k0, uint64_t *v0, int64_t *w0, int64_t cap0, uint64_t *c1,
        uint64_t *k1, uint64_t *v1, int64_t *w1, int64_t cap1);

// query 103's front, defined with the antijoin kernels below
__global__ __launch_bounds__(FLATMAP_BLK) void k_flatmap_auction_bidkey(
        const dbsp_event *ev, dbspk::EventCols cols, int64_t n, uint64_t *c0,
        uint64_t *k0, uint64_t *v0, int64_t *w0, int64_t cap0, uint64_t *c1,
        uint64_t *k1, uint64_t *v1, int64_t *w1, int64_t cap1);

// query 7's front, defined with the arg-max kernels below
__global__ __launch_bounds__(FLATMAP_BLK) void k_flatmap_bid_time(
        const dbsp_event *ev, dbspk::EventCols cols, int64_t n, uint64_t *c0,
        uint64_t *k0, uint64_t *v0, int64_t *w0, int64_t cap0, uint64_t *c1,
        uint64_t *k1, uint64_t *v1, int64_t *w1, int64_t cap1);

dbsp_status flatmap_events_chain(hipStream_t s, const dbsp_event *ev,
                                 const EventCols *cols, int64_t n, int query,
                                 const Rows &out0, const Rows &out1,
                                 uint64_t *ctr /* 2 device slots */,
                                 bool ctr_zero) {
    if (!ctr_zero) HIP_CHECK(hipMemsetAsync(ctr, 0, 2 * sizeof(uint64_t), s));
    EventCols c{};
    if (cols) c = *cols;
    if (n > 0 && query == 102)
        k_flatmap_bid_tv<<<grid_for(n, FLATMAP_BLK), FLATMAP_BLK, 0, s>>>(
            ev, c, n, ctr, out0.k, out0.v, out0.w, out0.n, ctr + 1);
    else if (n > 0 && query == 19)
        k_flatmap_bid_topk<<<grid_for(n, FLATMAP_BLK), FLATMAP_BLK, 0, s>>>(
            ev, c, n, ctr, out0.k, out0.v, out0.w, out0.n, ctr + 1, out1.k,
            out1.v, out1.w, out1.n);
    else if (n > 0 && query == 103)
        k_flatmap_auction_bidkey<<<grid_for(n, FLATMAP_BLK), FLATMAP_BLK, 0,
                                   s>>>(
            ev, c, n, ctr, out0.k, out0.v, out0.w, out0.n, ctr + 1, out1.k,
            out1.v, out1.w, out1.n);
    else if (n > 0 && query == 7)
        k_flatmap_bid_time<<<grid_for(n, FLATMAP_BLK), FLATMAP_BLK, 0, s>>>(
            ev, c, n, ctr, out0.k, out0.v, out0.w, out0.n, ctr + 1, out1.k,
            out1.v, out1.w, out1.n);
    else if (n > 0)
        k_flatmap<<<grid_for(n, FLATMAP_BLK), FLATMAP_BLK, 0, s>>>(
            ev, c, n, query, ctr, out0.k, out0.v, out0.w, out0.n, ctr + 1,
            out1.k, out1.v, out1.w, out1.n);
    return DBSP_OK;
}

dbsp_status flatmap_events(hipStream_t s, const dbsp_event *ev,
                           const EventCols *cols, int64_t n, int query,
                           Rows *out0, Rows *out1) {
    Scratch sc(s);
    uint64_t *ctr;
    HIP_CHECK(sc.get(&ctr, 2 * sizeof(uint64_t)));
    TRY_K(flatmap_events_chain(s, ev, cols, n, query, *out0, *out1, ctr));
    uint64_t h_ctr[2];
    HIP_CHECK(hipMemcpyAsync(h_ctr, ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    out0->n = (int64_t)h_ctr[0];
    out1->n = (int64_t)h_ctr[1];
    return DBSP_OK;
}

dbsp_status map_rows(hipStream_t s, const Rows &in, int mode, const Rows &out) {
    if (in.n > 0)
        k_map<<<grid_for(in.n), BLK, 0, s>>>(in.k, in.v, in.w, in.n, mode,
                                             out.k, out.v, out.w);
    return DBSP_OK;
}

dbsp_status agg_sum_batch(hipStream_t s, const uint64_t *keys, int64_t nd,
                          const Rows &in, int64_t *acc, bool wf64) {
    if (nd <= 0 || in.n <= 0) return DBSP_OK;
    if (wf64)
        k_agg_sum<double><<<grid_for(nd), BLK, 0, s>>>(
            keys, nd, in.k, (const double *)in.w, in.n, (double *)acc);
    else
        k_agg_sum<int64_t><<<grid_for(nd), BLK, 0, s>>>(keys, nd, in.k, in.w,
                                                        in.n, acc);
    return DBSP_OK;
}

dbsp_status emit_nonzero(hipStream_t s, const uint64_t *keys,
                         const int64_t *acc, int64_t nd, bool wf64, Rows *out) {
    Scratch sc(s);
    uint64_t *ctr;
    HIP_CHECK(sc.get(&ctr, sizeof(uint64_t)));
    HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof(uint64_t), s));
    if (nd > 0 && wf64)
        k_emit_nonzero<double><<<grid_for(nd), BLK, 0, s>>>(
            keys, (const double *)acc, nd, ctr, out->k, out->v, out->w);
    else if (nd > 0)
        k_emit_nonzero<int64_t><<<grid_for(nd), BLK, 0, s>>>(
            keys, acc, nd, ctr, out->k, out->v, out->w);
    uint64_t h = 0;
    HIP_CHECK(hipMemcpyAsync(&h, ctr, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    out->n = (int64_t)h;
    return DBSP_OK;
}

dbsp_status unique_keys(hipStream_t s, const uint64_t *kk, int64_t n,
                        uint64_t **okeys, int64_t *out_n) {
    if (n == 0) {
        *okeys = nullptr;
        *out_n = 0;
        return DBSP_OK;
    }
    Scratch sc(s);
    uint64_t *flags, *fscan;
    HIP_CHECK(sc.get(&flags, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, n * sizeof(uint64_t)));
    k_key_head_flags<<<grid_for(n), BLK, 0, s>>>(kk, n, flags);
    uint64_t nk = 0;
    TRY_K(scan_exclusive(s, flags, fscan, n, &nk));
    uint64_t *keys;
    HIP_CHECK(sc.get(&keys, nk * sizeof(uint64_t) + 8));
    k_compact_keys<<<grid_for(n), BLK, 0, s>>>(kk, flags, fscan, n, keys);
    sc.keep(keys);
    *okeys = keys;
    *out_n = (int64_t)nk;
    return DBSP_OK;
}


// ---------------------------------------------------------------------------
// Radix-tree rolling aggregate (operator/time_series/radix_tree/mod.rs:1-75,
// rolling_aggregate.rs:235-280, range.rs:76-110 — SURVEY.md §8f4).  The
// reference covers the timeline with an adaptive radix tree of per-prefix
// aggregates, stored as indexed Z-sets, so a range aggregate visits O(log n)
// nodes.  The MI355X-native restatement: the batch is already (partition,
// time)-sorted, so the same O(log) range queries come from a FLAT radix-16
// prefix-aggregate tree over the row array (levels of 16:1 weight-sum
// reductions — "prefix-sum trees map well to GPU scans") and
// a row's time range maps to a row range by binary search.  One query
// thread per input row computes the rolling aggregate
// range_of(ts) = [ts - width, ts] (RelRange::range_of, range.rs:93-110,
// saturating at 0) within its partition — the per-row output of
// partitioned_rolling_aggregate for the linear (weight-sum) aggregate.
// ---------------------------------------------------------------------------

#define RT_RADIX 16
#define RT_MAX_LEVELS 16

struct RtLevels {
    int nl;
    const int64_t *lv[RT_MAX_LEVELS];
    int64_t n[RT_MAX_LEVELS];
};

// The tree's semigroup (Agg::Semigroup, rolling_aggregate.rs:487-604): how
// two nodes combine, the identity an empty range yields, and the leaf read
// from the row array's 8-byte leaf column.  RtSum's leaves are the weights
// (the linear aggregate); RtMax / RtMin read the value half of a row's
// v = ts << 32 | val (the per-time Max / Min aggregate, aggregate/max.rs
// :36-55, min.rs:38-57, folded over a run of rows by the level-0 reduce).
// Both identities are also legal values: a query range is never empty.
struct RtSum {
    static __device__ __forceinline__ int64_t identity() { return 0; }
    static __device__ __forceinline__ int64_t leaf(int64_t x) { return x; }
    static __device__ __forceinline__ int64_t combine(int64_t a, int64_t b) {
        return a + b;
    }
};
struct RtMax {
    static __device__ __forceinline__ int64_t identity() { return 0; }
    static __device__ __forceinline__ int64_t leaf(int64_t x) {
        return x & 0xFFFFFFFFll;
    }
    static __device__ __forceinline__ int64_t combine(int64_t a, int64_t b) {
        return a > b ? a : b;
    }
};
struct RtMin {
    static __device__ __forceinline__ int64_t identity() {
        return 0xFFFFFFFFll;
    }
    static __device__ __forceinline__ int64_t leaf(int64_t x) {
        return x & 0xFFFFFFFFll;
    }
    static __device__ __forceinline__ int64_t combine(int64_t a, int64_t b) {
        return a < b ? a : b;
    }
};

// one 16:1 level.  LEAF: `in` is the row array's leaf column (level 0);
// otherwise it is the level below.  Every thread walks its 16 consecutive
// elements (the row-per-16-lanes form has not been written or measured).
template <class A, bool LEAF>
__global__ void k_rt_reduce(const int64_t *in, int64_t n, int64_t *out,
                            int64_t n_out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_out;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t s = A::identity();
        const int64_t lo = i * RT_RADIX;
        const int64_t hi = lo + RT_RADIX < n ? lo + RT_RADIX : n;
        for (int64_t j = lo; j < hi; j++)
            s = A::combine(s, LEAF ? A::leaf(in[j]) : in[j]);
        out[i] = s;
    }
}

// range aggregate over the rows [a, b) using the tree: peel unaligned edges
// at each level (<= 15 combines per level per side), then ascend —
// O(log16 n) work.  leaf: the column the tree was built over.
template <class A>
__device__ inline int64_t rt_range(const int64_t *leaf, const RtLevels &t,
                                   int64_t a, int64_t b) {
    int64_t acc = A::identity();
    // level 0: the leaf column through the accessor
    while ((a % RT_RADIX) != 0 && a < b) acc = A::combine(acc, A::leaf(leaf[a++]));
    while ((b % RT_RADIX) != 0 && a < b) acc = A::combine(acc, A::leaf(leaf[--b]));
    int lvl = 0;
    while (a < b) {
        a /= RT_RADIX;
        b /= RT_RADIX;
        const int64_t *cur = t.lv[lvl++];
        while ((a % RT_RADIX) != 0 && a < b) acc = A::combine(acc, cur[a++]);
        while ((b % RT_RADIX) != 0 && a < b) acc = A::combine(acc, cur[--b]);
    }
    return acc;
}
__device__ inline int64_t rt_range_sum(const int64_t *w, int64_t nw,
                                       const RtLevels &t, int64_t a,
                                       int64_t b) {
    return rt_range<RtSum>(w, t, a, b);
}

// first row of the (k, v)-sorted rows [lo, hi) with (k, v) >= (kk, vv) /
// > (kk, vv): a partition's time bound as a row index (shared by the batch
// primitive below and the incremental operator's gather / eval kernels)
__device__ inline int64_t lex_lower(const uint64_t *k, const uint64_t *v,
                                    int64_t lo, int64_t hi, uint64_t kk,
                                    uint64_t vv) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        const uint64_t km = k[mid];
        if (km < kk || (km == kk && v[mid] < vv)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ inline int64_t lex_upper(const uint64_t *k, const uint64_t *v,
                                    int64_t lo, int64_t hi, uint64_t kk,
                                    uint64_t vv) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        const uint64_t km = k[mid];
        if (km < kk || (km == kk && v[mid] <= vv)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_rolling_agg(const uint64_t *k, const uint64_t *v,
                              const int64_t *w, int64_t n, RtLevels t,
                              uint64_t width, uint64_t *ok, uint64_t *ov,
                              int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t p = k[i], ts = v[i];
        // partition row range
        const int64_t plo = lower_bound_k(k, n, p);
        int64_t phi = plo;
        {
            int64_t step = 1;
            while (phi + step < n && k[phi + step] == p) { phi += step; step <<= 1; }
            phi = upper_bound_k(k + phi, min(step, n - phi), p) + phi;
        }
        // time range [ts - width, ts] inclusive (range.rs:93-110, saturating)
        const uint64_t t0 = ts >= width ? ts - width : 0;
        const int64_t qlo = lex_lower(k, v, plo, phi, p, t0);
        const int64_t qhi = lex_upper(k, v, qlo, phi, p, ts);
        ok[i] = p;
        ov[i] = ts;
        ow[i] = rt_range_sum(w, n, t, qlo, qhi);
    }
}

// build the radix-16 levels over the leaf column leaf[0..n): the weights for
// RtSum, the v column for RtMax / RtMin (the levels live in sc)
template <class A>
static dbsp_status rt_build(Scratch &sc, const int64_t *leaf, int64_t n,
                            RtLevels &t) {
    int64_t cur_n = n;
    const int64_t *cur = leaf;
    while (cur_n > 1 && t.nl < RT_MAX_LEVELS) {
        const int64_t nn = (cur_n + RT_RADIX - 1) / RT_RADIX;
        int64_t *lv;
        HIP_CHECK(sc.get(&lv, nn * sizeof(int64_t) + 8));
        if (t.nl == 0)
            k_rt_reduce<A, true><<<grid_for(nn), BLK, 0, sc.stream()>>>(
                cur, cur_n, lv, nn);
        else
            k_rt_reduce<A, false><<<grid_for(nn), BLK, 0, sc.stream()>>>(
                cur, cur_n, lv, nn);
        t.lv[t.nl] = lv;
        t.n[t.nl] = nn;
        cur = lv;
        cur_n = nn;
        t.nl++;
    }
    return DBSP_OK;
}

dbsp_status rolling_agg_rows(hipStream_t s, const Rows &in, uint64_t width,
                             const Rows &out) {
    if (in.n <= 0) return DBSP_OK;
    Scratch sc(s);
    RtLevels t{};
    TRY_K(rt_build<RtSum>(sc, in.w, in.n, t));
    k_rolling_agg<<<grid_for(in.n), BLK, 0, s>>>(in.k, in.v, in.w, in.n, t,
                                                 width, out.k, out.v, out.w);
    return DBSP_OK;
}

// ---------------------------------------------------------------------------
// Incremental partitioned rolling aggregate (PartitionedRollingAggregate::eval,
// operator/time_series/rolling_aggregate.rs:487-604, linear weight-sum
// aggregator).  Per tick the operator (engine.cpp RollingOp) touches only
// the times the delta can affect:
//   k_roll_heads / k_roll_ranges   delta -> merged gather + affected ranges
//                                  (affected_ranges, rolling_aggregate.rs
//                                  :436-456 / RelRange::affected_range_of,
//                                  range.rs:109-120)
//   k_range_count / k_range_emit   ranges x spine batches -> signed row copy
//   k_roll_flags / k_roll_emit     gathered slice -> (p<<32|ts, sum, +1) for
//                                  the affected rows of positive weight
// Times and partitions are < 2^32 (they pack into one output key); ranges
// saturate at 0 and at 2^32-1.
// ---------------------------------------------------------------------------

#define ROLL_TMAX 0xFFFFFFFFull

__device__ inline uint64_t roll_lo(uint64_t ts, uint64_t below) {
    return ts >= below ? ts - below : 0;
}
__device__ inline uint64_t roll_hi(uint64_t ts, uint64_t above) {
    if (ts >= ROLL_TMAX) return ROLL_TMAX;
    return above >= ROLL_TMAX - ts ? ROLL_TMAX : ts + above;
}

// head flags of both run lists, packed (gather | affected << 32) so ONE scan
// numbers both.  The delta is (p, ts)-sorted and each list's widths are
// uniform, so a run breaks exactly where the partition changes or this row's
// range starts past the previous row's end.  Raises the precondition word.
// TSH: where a row's time sits in v: 0 for rows (p, ts, w), 32 for rows
// (p, ts << 32 | val, w), whose equal-time rows merge into one run like any
// other overlap and whose v can raise nothing.
template <int TSH>
__global__ void k_roll_heads(const uint64_t *dk, const uint64_t *dv, int64_t n,
                             uint64_t before, uint64_t after, uint64_t both,
                             uint64_t *flags, unsigned long long *err) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t p = dk[i], ts = dv[i] >> TSH;
        if (p > ROLL_TMAX || ts > ROLL_TMAX) atomicOr(err, 1ull);
        uint64_t hg = 1, ha = 1;
        if (i > 0 && dk[i - 1] == p) {
            const uint64_t tp = dv[i - 1] >> TSH;
            hg = roll_lo(ts, both) > roll_hi(tp, both);
            ha = roll_lo(ts, after) > roll_hi(tp, before);
        }
        flags[i] = hg | (ha << 32);
    }
}

// run r of a list takes lo from its first row and hi from its last
template <int TSH>
__global__ void k_roll_ranges(const uint64_t *dk, const uint64_t *dv, int64_t n,
                              uint64_t before, uint64_t after, uint64_t both,
                              const uint64_t *flags, const uint64_t *fscan,
                              uint64_t *gp, uint64_t *glo, uint64_t *ghi,
                              uint64_t *ap, uint64_t *alo, uint64_t *ahi) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t p = dk[i], ts = dv[i] >> TSH;
        const uint64_t f = flags[i], sc = fscan[i];
        const uint64_t fn = i + 1 < n ? flags[i + 1] : ~0ull;
        const uint64_t hg = f & 1, ha = (f >> 32) & 1;
        // row 0 heads both lists, so the run index is never negative
        const int64_t ig = (int64_t)(sc & ROLL_TMAX) + (int64_t)hg - 1;
        const int64_t ia = (int64_t)(sc >> 32) + (int64_t)ha - 1;
        if (hg) { gp[ig] = p; glo[ig] = roll_lo(ts, both); }
        if (fn & 1) ghi[ig] = roll_hi(ts, both);
        if (ha) { ap[ia] = p; alo[ia] = roll_lo(ts, after); }
        if ((fn >> 32) & 1) ahi[ia] = roll_hi(ts, before);
    }
}

// range-gather count: one thread per (range, spine batch) pair, two binary
// searches.  mode 0: rows (k, v) in [(p, lo), (p, hi)] (the input trace);
// mode 1: rows with k in [p<<32|lo, p<<32|hi] (the output trace, whose key
// packs partition and time); mode 2: rows (k, v) in [(p, lo<<32),
// (p, hi<<32|0xffffffff)] (an input trace whose v packs time and value).
// Empty batches and ranges count 0.
__global__ void k_range_count(const uint64_t *rp, const uint64_t *rlo,
                              const uint64_t *rhi, int64_t nr, TraceArgs t,
                              int mode, uint64_t *cnt, uint64_t *start) {
    const int64_t np = nr * t.nb;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < np;
         j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = j / t.nb;
        const int b = (int)(j % t.nb);
        const uint64_t p = rp[r], lo_t = rlo[r], hi_t = rhi[r];
        const int64_t n = t.n[b];
        int64_t lo = 0, hi = 0;
        if (n > 0 && lo_t <= hi_t) {
            if (mode == 0) {
                lo = lex_lower(t.k[b], t.v[b], 0, n, p, lo_t);
                hi = lex_upper(t.k[b], t.v[b], lo, n, p, hi_t);
            } else if (mode == 2) {
                lo = lex_lower(t.k[b], t.v[b], 0, n, p, lo_t << 32);
                hi = lex_upper(t.k[b], t.v[b], lo, n, p,
                               (hi_t << 32) | ROLL_TMAX);
            } else {
                lo = lower_bound_k(t.k[b], n, (p << 32) | lo_t);
                hi = lo + upper_bound_k(t.k[b] + lo, n - lo, (p << 32) | hi_t);
            }
        }
        cnt[j] = (uint64_t)(hi - lo);
        start[j] = (uint64_t)lo;
    }
}

// emit over the OUTPUT index space (as k_join_emit): the pair is found by
// binary search in the exclusive offsets, so one huge range costs no more
// per thread than many small ones
__global__ void k_range_emit(TraceArgs t, int64_t np, const uint64_t *offsets,
                             const uint64_t *start, int64_t n_out,
                             int64_t sign, uint64_t *ok, uint64_t *ov,
                             int64_t *ow) {
    for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < n_out;
         o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = upper_bound_k(offsets, np, (uint64_t)o) - 1;
        const int b = (int)(j % t.nb);
        const int64_t src = (int64_t)start[j] + (o - (int64_t)offsets[j]);
        ok[o] = t.k[b][src];
        ov[o] = t.v[b][src];
        ow[o] = sign * t.w[b][src];
    }
}

// a slice row (p, ts) is re-emitted iff its total weight is positive
// (!weight.le0(), rolling_aggregate.rs:574) and the delta has a row of
// partition p with time in range_of(ts) = [ts - before, ts + after]
__global__ void k_roll_flags(const uint64_t *sk, const uint64_t *sv,
                             const int64_t *sw, int64_t n, const uint64_t *dk,
                             const uint64_t *dv, int64_t nd, uint64_t before,
                             uint64_t after, uint64_t *flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t f = 0;
        if (sw[i] > 0) {
            const uint64_t p = sk[i], ts = sv[i];
            const int64_t j = lex_lower(dk, dv, 0, nd, p, roll_lo(ts, before));
            f = j < nd && dk[j] == p && dv[j] <= roll_hi(ts, after);
        }
        flags[i] = f;
    }
}

__global__ void k_roll_emit(const uint64_t *sk, const uint64_t *sv,
                            const int64_t *sw, int64_t n, RtLevels t,
                            uint64_t before, uint64_t after,
                            const uint64_t *flags, const uint64_t *fscan,
                            uint64_t *ok, uint64_t *ov, int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!flags[i]) continue;
        const uint64_t p = sk[i], ts = sv[i];
        const int64_t qlo = lex_lower(sk, sv, 0, n, p, roll_lo(ts, before));
        const int64_t qhi = lex_upper(sk, sv, qlo, n, p, roll_hi(ts, after));
        const int64_t o = (int64_t)fscan[i];
        ok[o] = (p << 32) | ts;
        ov[o] = (uint64_t)rt_range_sum(sw, n, t, qlo, qhi);
        ow[o] = 1;
    }
}

static inline uint64_t sat_add_u64(uint64_t a, uint64_t b) {
    return a + b < a ? UINT64_MAX : a + b;
}

dbsp_status roll_ranges(hipStream_t s, const Rows &delta, bool time_hi,
                        uint64_t before, uint64_t after, uint64_t **ranges,
                        int64_t *n_gather, int64_t *n_affected, int *err) {
    const uint64_t *dk = delta.k, *dv = delta.v;
    const int64_t n = delta.n;
    *ranges = nullptr;
    *n_gather = *n_affected = 0;
    *err = 0;
    if (n <= 0) return DBSP_OK;
    const uint64_t both = sat_add_u64(before, after);
    Scratch sc(s);
    uint64_t *flags, *fscan, *rb;
    // flags[n] is the precondition error word
    HIP_CHECK(sc.get(&flags, (n + 1) * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&rb, 6 * n * sizeof(uint64_t)));
    HIP_CHECK(hipMemsetAsync(flags + n, 0, sizeof(uint64_t), s));
    unsigned long long *d_err = (unsigned long long *)(flags + n);
    if (time_hi)
        k_roll_heads<32><<<grid_for(n), BLK, 0, s>>>(dk, dv, n, before, after,
                                                     both, flags, d_err);
    else
        k_roll_heads<0><<<grid_for(n), BLK, 0, s>>>(dk, dv, n, before, after,
                                                    both, flags, d_err);
    uint64_t h_err = 0, total = 0;
    HIP_CHECK(hipMemcpyAsync(&h_err, flags + n, sizeof(uint64_t),
                             hipMemcpyDeviceToHost, s));
    TRY_K(scan_exclusive(s, flags, fscan, n, &total));  // syncs: err + lengths
    if (h_err == 0) {
        if (time_hi)
            k_roll_ranges<32><<<grid_for(n), BLK, 0, s>>>(
                dk, dv, n, before, after, both, flags, fscan, rb, rb + n,
                rb + 2 * n, rb + 3 * n, rb + 4 * n, rb + 5 * n);
        else
            k_roll_ranges<0><<<grid_for(n), BLK, 0, s>>>(
                dk, dv, n, before, after, both, flags, fscan, rb, rb + n,
                rb + 2 * n, rb + 3 * n, rb + 4 * n, rb + 5 * n);
        *n_gather = (int64_t)(total & ROLL_TMAX);
        *n_affected = (int64_t)(total >> 32);
        sc.keep(rb);
        *ranges = rb;
    } else {
        HIP_CHECK(sc.release(rb));  // early: ahead of flags and fscan
        *err = 1;
    }
    return DBSP_OK;
}

dbsp_status range_gather(hipStream_t s, const uint64_t *rp,
                         const uint64_t *rlo, const uint64_t *rhi, int64_t nr,
                         const TraceArgs &t, int mode, int64_t sign,
                         Rows *out) {
    if (nr <= 0 || t.nb <= 0) return no_rows(out);
    const int64_t np = nr * t.nb;
    Scratch sc(s);
    uint64_t *cnt, *start;
    HIP_CHECK(sc.get(&cnt, np * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&start, np * sizeof(uint64_t)));
    k_range_count<<<grid_for(np), BLK, 0, s>>>(rp, rlo, rhi, nr, t, mode, cnt,
                                               start);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, cnt, cnt, np, &total));
    if (total == 0) return no_rows(out);
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)total, &r));
    k_range_emit<<<grid_for((int64_t)total), BLK, 0, s>>>(
        t, np, cnt, start, (int64_t)total, sign, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

// ---------------------------------------------------------------------------
// Order-preserving truncation of a spine (TraceBounds lower bound,
// operator/trace.rs:463-607): every batch compacted to its rows whose time
// is >= bound.  The dead rows are a prefix of each partition's run, so they
// are interleaved through a batch: a stable stream compaction, not a slice.
//   k_trunc_count   one block per TRUNC_TILE rows of one batch, tiles laid
//                   out batch-major; reads the 8-byte time column only
//   scan_exclusive  over the tile counts of the whole spine
//   k_trunc_totals  per-batch totals out of the scanned counts (one readback)
//   k_trunc_emit    same tiling; ranks by wave64 ballot inside the block and
//                   by the scanned count across blocks
// A tile is BLK lanes x TRUNC_ITEMS passes with lane-consecutive rows per
// pass, so every load is a coalesced 8 B/lane stream and the kept rows of a
// wave land contiguously.  No tile looks at another tile's state.
// ---------------------------------------------------------------------------

#define TRUNC_ITEMS 8
#define TRUNC_TILE (BLK * TRUNC_ITEMS)  // 2048 rows per block
#define TRUNC_WAVES (BLK / WAVE)

struct TruncArgs {
    TraceArgs t;
    int64_t blk0[MAX_TRACE_BATCHES + 1];  // first tile of batch b; [nb] = all
    int mode;        // 0: time = v; 1: time = low 32 bits of k; 2: v >> 32
    uint64_t bound;
};
struct TruncOut {
    uint64_t *k[MAX_TRACE_BATCHES];
    uint64_t *v[MAX_TRACE_BATCHES];
    int64_t *w[MAX_TRACE_BATCHES];
};

__device__ inline int trunc_batch_of(const TruncArgs &a, int64_t blk) {
    int b = 0;
    while (b + 1 < a.t.nb && blk >= a.blk0[b + 1]) b++;
    return b;
}

__global__ void __launch_bounds__(BLK)
k_trunc_count(TruncArgs a, uint64_t *counts) {
    __shared__ uint32_t wave_cnt[TRUNC_WAVES];
    const int64_t blk = blockIdx.x;
    const int b = trunc_batch_of(a, blk);
    const uint64_t *tc = a.mode == 1 ? a.t.k[b] : a.t.v[b];
    const uint64_t mask = a.mode == 1 ? ROLL_TMAX : ~0ull;
    const int tsh = a.mode == 2 ? 32 : 0;
    const int64_t n = a.t.n[b];
    const int64_t base = (blk - a.blk0[b]) * TRUNC_TILE + threadIdx.x;
    uint32_t c = 0;  // wave-uniform
#pragma unroll
    for (int it = 0; it < TRUNC_ITEMS; it++) {
        const int64_t i = base + it * BLK;
        const bool keep = i < n && ((tc[i] & mask) >> tsh) >= a.bound;
        c += (uint32_t)__popcll(__ballot(keep));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_cnt[threadIdx.x / WAVE] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < TRUNC_WAVES; w++) sum += wave_cnt[w];
        counts[blk] = sum;
    }
}

__global__ void k_trunc_totals(TruncArgs a, const uint64_t *offsets,
                               int64_t *totals) {
    const int b = threadIdx.x;
    if (b < a.t.nb)
        totals[b] = (int64_t)(offsets[a.blk0[b + 1]] - offsets[a.blk0[b]]);
}

// offsets: exclusive scan of the tile counts, one entry past the last tile
__global__ void __launch_bounds__(BLK)
k_trunc_emit(TruncArgs a, const uint64_t *offsets, TruncOut o) {
    __shared__ uint64_t pre[TRUNC_ITEMS * TRUNC_WAVES];
    const int64_t blk = blockIdx.x;
    const uint64_t off0 = offsets[blk];
    if (offsets[blk + 1] == off0) return;  // nothing of this tile survives
    const int b = trunc_batch_of(a, blk);
    const uint64_t *tc = a.mode == 1 ? a.t.k[b] : a.t.v[b];
    const uint64_t *oc = a.mode == 1 ? a.t.v[b] : a.t.k[b];
    uint64_t *otc = a.mode == 1 ? o.k[b] : o.v[b];
    uint64_t *ooc = a.mode == 1 ? o.v[b] : o.k[b];
    const int64_t *wc = a.t.w[b];
    int64_t *owc = o.w[b];
    const uint64_t mask = a.mode == 1 ? ROLL_TMAX : ~0ull;
    const int tsh = a.mode == 2 ? 32 : 0;
    const int64_t n = a.t.n[b];
    const int64_t base = (blk - a.blk0[b]) * TRUNC_TILE + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    uint64_t tv[TRUNC_ITEMS], bal[TRUNC_ITEMS];
#pragma unroll
    for (int it = 0; it < TRUNC_ITEMS; it++) {
        const int64_t i = base + it * BLK;
        tv[it] = i < n ? tc[i] : 0;
        bal[it] = __ballot(i < n && ((tv[it] & mask) >> tsh) >= a.bound);
        if (lane == 0)
            pre[it * TRUNC_WAVES + wid] = (uint64_t)__popcll(bal[it]);
    }
    __syncthreads();
    // rows ascend with (pass, wave, lane), and so does the pre[] index
    if (threadIdx.x < WAVE) {
        const bool in = threadIdx.x < TRUNC_ITEMS * TRUNC_WAVES;
        uint64_t tot;
        const uint64_t ex = wave_scan_excl(in ? pre[threadIdx.x] : 0, tot);
        if (in) pre[threadIdx.x] = ex;
    }
    __syncthreads();
    // position inside the batch's own output
    const int64_t dst0 = (int64_t)(off0 - offsets[a.blk0[b]]);
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (int it = 0; it < TRUNC_ITEMS; it++) {
        if (!((bal[it] >> lane) & 1)) continue;
        const int64_t i = base + it * BLK;
        const int64_t d = dst0 + (int64_t)pre[it * TRUNC_WAVES + wid] +
                          __popcll(bal[it] & below);
        otc[d] = tv[it];
        ooc[d] = oc[i];
        owc[d] = wc[i];
    }
}

dbsp_status truncate_spine(hipStream_t s, const TraceArgs &t, int mode,
                           uint64_t bound, Rows *out) {
    if (t.nb < 0 || t.nb > MAX_TRACE_BATCHES || mode < 0 || mode > 2)
        return DBSP_ERR_INVALID;
    TruncArgs a{};
    a.t = t;
    a.mode = mode;
    a.bound = bound;
    int64_t nblk = 0;
    for (int b = 0; b < t.nb; b++) {
        out[b] = Rows{};
        if (t.n[b] < 0) return DBSP_ERR_INVALID;
        a.blk0[b] = nblk;
        nblk += ceil_div(t.n[b], TRUNC_TILE);
    }
    a.blk0[t.nb] = nblk;
    if (nblk == 0) return DBSP_OK;
    if (nblk >= (int64_t)1 << 31) return DBSP_ERR_INVALID;  // grid.x limit
    // counts[nblk] = 0 so the scan leaves the grand total there; the
    // per-batch totals follow in the same buffer
    Scratch sc(s);
    uint64_t *counts;
    HIP_CHECK(sc.get(&counts,
                     (nblk + 1 + MAX_TRACE_BATCHES) * sizeof(uint64_t)));
    int64_t *d_tot = (int64_t *)(counts + nblk + 1);
    HIP_CHECK(hipMemsetAsync(counts + nblk, 0, sizeof(uint64_t), s));
    k_trunc_count<<<dim3((uint32_t)nblk), BLK, 0, s>>>(a, counts);
    TRY_K(scan_exclusive(s, counts, counts, nblk + 1, nullptr));
    k_trunc_totals<<<1, WAVE, 0, s>>>(a, counts, d_tot);
    int64_t h_tot[MAX_TRACE_BATCHES];
    HIP_CHECK(hipMemcpyAsync(h_tot, d_tot, t.nb * sizeof(int64_t),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // the one length sync
    TruncOut o{};
    Rows r[MAX_TRACE_BATCHES];
    int64_t kept = 0;
    for (int b = 0; b < t.nb; b++) {
        const int64_t m = h_tot[b];
        if (m < 0 || m > t.n[b]) return DBSP_ERR_INTERNAL;
        kept += m;
        if (m == 0) continue;
        TRY_K(alloc_rows(sc, m, &r[b]));
        o.k[b] = r[b].k;
        o.v[b] = r[b].v;
        o.w[b] = r[b].w;
    }
    if (kept > 0)
        k_trunc_emit<<<dim3((uint32_t)nblk), BLK, 0, s>>>(a, counts, o);
    for (int b = 0; b < t.nb; b++) (void)give_rows(sc, r[b], &out[b]);
    return DBSP_OK;
}

dbsp_status roll_eval_rows(hipStream_t s, const Rows &slice,
                           const Rows &delta, uint64_t before, uint64_t after,
                           Rows *out) {
    const int64_t n = slice.n;
    if (n <= 0 || delta.n <= 0) return no_rows(out);
    Scratch sc(s);
    uint64_t *flags, *fscan;
    HIP_CHECK(sc.get(&flags, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, n * sizeof(uint64_t)));
    k_roll_flags<<<grid_for(n), BLK, 0, s>>>(slice.k, slice.v, slice.w, n,
                                             delta.k, delta.v, delta.n, before,
                                             after, flags);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, flags, fscan, n, &total));
    if (total == 0) return no_rows(out);
    // an inner scope: the tree levels go back ahead of flags and fscan
    Scratch lv(s);
    RtLevels t{};
    TRY_K(rt_build<RtSum>(lv, slice.w, n, t));
    Rows r;
    TRY_K(alloc_rows(lv, (int64_t)total, &r));
    k_roll_emit<<<grid_for(n), BLK, 0, s>>>(slice.k, slice.v, slice.w, n, t,
                                            before, after, flags, fscan, r.k,
                                            r.v, r.w);
    return give_rows(lv, r, out);
}

// ---------------------------------------------------------------------------
// Rolling Max / Min (partitioned_rolling_aggregate<TS, V, Agg> with Agg = Max
// or Min, rolling_aggregate.rs:235-321; eval at :487-604 combining nodes with
// Agg::Semigroup).  Rows are (p, ts << 32 | val, w), so (k, v) order is
// (p, ts, val) order and a time's rows are one run.  The aggregate of a time
// is the extreme val over its rows of ANY non-zero weight (max.rs:36-55,
// min.rs:38-57: the first / last value "with non-zero weight" — a
// consolidated batch holds no other), which the RtMax / RtMin tree folds
// over row ranges.  Every row range is two lexicographic searches over the
// packed v: [(p, lo << 32), (p, hi << 32 | 0xffffffff)].
// ---------------------------------------------------------------------------

// batch primitive: per row i, the extreme over its partition's rows with time
// in range_of(ts_i)
template <class A>
__global__ void k_rolling_minmax(const uint64_t *k, const uint64_t *v,
                                 int64_t n, RtLevels t, uint64_t before,
                                 uint64_t after, uint64_t *ok, uint64_t *ov,
                                 int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t p = k[i], ts = v[i] >> 32;
        const int64_t qlo = lex_lower(k, v, 0, n, p, roll_lo(ts, before) << 32);
        const int64_t qhi = lex_upper(k, v, qlo, n, p,
                                      (roll_hi(ts, after) << 32) | ROLL_TMAX);
        ok[i] = p;
        ov[i] = v[i];
        ow[i] = rt_range<A>((const int64_t *)v, t, qlo, qhi);
    }
}

dbsp_status rolling_minmax_rows(hipStream_t s, const Rows &in, bool is_min,
                                uint64_t before, uint64_t after,
                                const Rows &out) {
    if (in.n <= 0) return DBSP_OK;
    Scratch sc(s);
    RtLevels t{};
    const int64_t *leaf = (const int64_t *)in.v;
    if (is_min) {
        TRY_K(rt_build<RtMin>(sc, leaf, in.n, t));
        k_rolling_minmax<RtMin><<<grid_for(in.n), BLK, 0, s>>>(
            in.k, in.v, in.n, t, before, after, out.k, out.v, out.w);
    } else {
        TRY_K(rt_build<RtMax>(sc, leaf, in.n, t));
        k_rolling_minmax<RtMax><<<grid_for(in.n), BLK, 0, s>>>(
            in.k, in.v, in.n, t, before, after, out.k, out.v, out.w);
    }
    return DBSP_OK;
}

// pos[i] = 1 iff slice row i has positive weight; pos[n] = 0, so the
// exclusive scan over n + 1 entries counts the positive rows of any row range
__global__ void k_roll_pos(const int64_t *sw, int64_t n, uint64_t *pos) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= n;
         i += (int64_t)gridDim.x * blockDim.x)
        pos[i] = i < n && sw[i] > 0;
}

// One flag per TIME: the head row of a (p, ts) run is flagged iff some row of
// the run has w > 0 (the value loop breaks at the first !weight.le0(),
// rolling_aggregate.rs:572-592, so a time emits once however many values it
// holds) and the delta has a row of partition p with time in range_of(ts).
// The run's end is one binary search and its positive rows one difference of
// the prefix count, so a hot time costs its head thread O(log n) like any
// other.
__global__ void k_roll_mm_flags(const uint64_t *sk, const uint64_t *sv,
                                int64_t n, const uint64_t *ppos,
                                const uint64_t *dk, const uint64_t *dv,
                                int64_t nd, uint64_t before, uint64_t after,
                                uint64_t *flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t p = sk[i], ts = sv[i] >> 32;
        uint64_t f = 0;
        if (i == 0 || sk[i - 1] != p || (sv[i - 1] >> 32) != ts) {
            const int64_t end =
                lex_upper(sk, sv, i, n, p, (ts << 32) | ROLL_TMAX);
            if (ppos[end] > ppos[i]) {
                const int64_t j =
                    lex_lower(dk, dv, 0, nd, p, roll_lo(ts, before) << 32);
                f = j < nd && dk[j] == p &&
                    (dv[j] >> 32) <= roll_hi(ts, after);
            }
        }
        flags[i] = f;
    }
}

template <class A>
__global__ void k_roll_mm_emit(const uint64_t *sk, const uint64_t *sv,
                               int64_t n, RtLevels t, uint64_t before,
                               uint64_t after, const uint64_t *flags,
                               const uint64_t *fscan, uint64_t *ok,
                               uint64_t *ov, int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!flags[i]) continue;
        const uint64_t p = sk[i], ts = sv[i] >> 32;
        const int64_t qlo =
            lex_lower(sk, sv, 0, n, p, roll_lo(ts, before) << 32);
        const int64_t qhi = lex_upper(sk, sv, qlo, n, p,
                                      (roll_hi(ts, after) << 32) | ROLL_TMAX);
        const int64_t o = (int64_t)fscan[i];
        ok[o] = (p << 32) | ts;
        ov[o] = (uint64_t)rt_range<A>((const int64_t *)sv, t, qlo, qhi);
        ow[o] = 1;
    }
}

dbsp_status roll_eval_minmax_rows(hipStream_t s, const Rows &slice,
                                  const Rows &delta, bool is_min,
                                  uint64_t before, uint64_t after, Rows *out) {
    const int64_t n = slice.n;
    if (n <= 0 || delta.n <= 0) return no_rows(out);
    Scratch sc(s);
    uint64_t *ppos, *flags, *fscan;
    HIP_CHECK(sc.get(&ppos, (n + 1) * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&flags, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, n * sizeof(uint64_t)));
    k_roll_pos<<<grid_for(n + 1), BLK, 0, s>>>(slice.w, n, ppos);
    TRY_K(scan_exclusive(s, ppos, ppos, n + 1, nullptr));
    k_roll_mm_flags<<<grid_for(n), BLK, 0, s>>>(slice.k, slice.v, n, ppos,
                                                delta.k, delta.v, delta.n,
                                                before, after, flags);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, flags, fscan, n, &total));
    if (total == 0) return no_rows(out);
    // an inner scope: the tree levels go back ahead of the flag columns
    Scratch lv(s);
    RtLevels t{};
    Rows r;
    const int64_t *leaf = (const int64_t *)slice.v;
    if (is_min) {
        TRY_K(rt_build<RtMin>(lv, leaf, n, t));
        TRY_K(alloc_rows(lv, (int64_t)total, &r));
        k_roll_mm_emit<RtMin><<<grid_for(n), BLK, 0, s>>>(
            slice.k, slice.v, n, t, before, after, flags, fscan, r.k, r.v,
            r.w);
    } else {
        TRY_K(rt_build<RtMax>(lv, leaf, n, t));
        TRY_K(alloc_rows(lv, (int64_t)total, &r));
        k_roll_mm_emit<RtMax><<<grid_for(n), BLK, 0, s>>>(
            slice.k, slice.v, n, t, before, after, flags, fscan, r.k, r.v,
            r.w);
    }
    return give_rows(lv, r, out);
}

// ---------------------------------------------------------------------------
// Incremental top-K per group (the aggregate(Fold) + flat_map of
// crates/nexmark/src/queries/q19.rs: a VecDeque that keeps the last K values
// of the group's cursor-ordered run, every value of non-zero weight stepping
// once, aggregate/fold.rs:83-92).  A row's group is k >> shift; plain (k, v)
// order is (group, rank) order.  A group's keys are the INCLUSIVE range
// [k & ~mask, k | mask] with mask = 2^shift - 1: the first key of the next
// group is never formed, it does not exist for the all-ones group.
//   k_topk_classify        per delta row: total weight in the input integral
//                          before the tick (one lexicographic search per
//                          spine batch) -> appear / vanish / neither, and
//                          the group head flag
//   k_topk_groups          head flags + scan -> row's group index, the
//                          affected groups' key ranges
//   k_keyrange_count       key-range-only gather count (k_range_emit emits)
//   k_topk_verdict         per vanish row: its group must refill iff the
//                          current top-K is full and the row is not below
//                          its first member
//   k_topk_refill_ranges   the refilled groups' key ranges, compacted
//   k_topk_cand_flags/emit the candidate rows of the groups NOT refilled
//   k_topk_select_flags/emit  a slice row is kept iff at most K - 1 rows
//                          follow it in its group: one binary search per row
// Every data-dependent size is flags -> scan -> emit; nothing passes between
// workgroups.
// ---------------------------------------------------------------------------

__device__ inline uint64_t topk_mask(int shift) {
    return shift ? ~0ull >> (64 - shift) : 0ull;
}

// cls: +1 appear (absent before, present after), -1 vanish, 0 neither.
// Presence is a non-zero total, negative totals included (fold.rs:83-92).
__global__ void k_topk_classify(const uint64_t *dk, const uint64_t *dv,
                                const int64_t *dw, int64_t n, TraceArgs t,
                                int shift, int64_t *cls, uint64_t *heads) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = dk[i], v = dv[i];
        int64_t before = 0;
        for (int b = 0; b < t.nb; b++) {
            const int64_t nb = t.n[b];
            const int64_t j = lex_lower(t.k[b], t.v[b], 0, nb, k, v);
            if (j < nb && t.k[b][j] == k && t.v[b][j] == v) before += t.w[b][j];
        }
        const int64_t after = before + dw[i];
        cls[i] = (int64_t)(before == 0 && after != 0) -
                 (int64_t)(before != 0 && after == 0);
        heads[i] = i == 0 || (dk[i - 1] >> shift) != (k >> shift);
    }
}

// gidx[i]: the affected-group index of delta row i; a head row writes its
// group's inclusive key range
__global__ void k_topk_groups(const uint64_t *dk, int64_t n, int shift,
                              const uint64_t *heads, const uint64_t *hscan,
                              uint64_t *gidx, uint64_t *glo, uint64_t *ghi) {
    const uint64_t mask = topk_mask(shift);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t h = heads[i];
        // row 0 is a head, so the index is never negative
        const uint64_t g = hscan[i] + h - 1;
        gidx[i] = g;
        if (h) {
            glo[g] = dk[i] & ~mask;
            ghi[g] = dk[i] | mask;
        }
    }
}

// key-range gather count: one thread per (range, spine batch) pair, rows with
// k in [klo, khi] whatever their v.  A sibling of k_range_count, whose modes
// split a 64-bit word into partition and time halves.
__global__ void k_keyrange_count(const uint64_t *klo, const uint64_t *khi,
                                 int64_t nr, TraceArgs t, uint64_t *cnt,
                                 uint64_t *start) {
    const int64_t np = nr * t.nb;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < np;
         j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = j / t.nb;
        const int b = (int)(j % t.nb);
        const int64_t n = t.n[b];
        int64_t lo = 0, hi = 0;
        if (n > 0 && klo[r] <= khi[r]) {
            lo = lower_bound_k(t.k[b], n, klo[r]);
            hi = lo + upper_bound_k(t.k[b] + lo, n - lo, khi[r]);
        }
        cnt[j] = (uint64_t)(hi - lo);
        start[j] = (uint64_t)lo;
    }
}

// ok/ov: the affected groups' current top-K rows (consolidated, at most K per
// group).  Several rows of a group may raise its flag: all store the same 1.
__global__ void k_topk_verdict(const uint64_t *dk, const uint64_t *dv,
                               const int64_t *cls, const uint64_t *gidx,
                               int64_t n, const uint64_t *glo,
                               const uint64_t *ghi, const uint64_t *ok,
                               const uint64_t *ov, int64_t no, int64_t K,
                               uint64_t *refill) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (cls[i] >= 0) continue;
        const uint64_t g = gidx[i];
        const int64_t a = lower_bound_k(ok, no, glo[g]);
        const int64_t b = a + upper_bound_k(ok + a, no - a, ghi[g]);
        if (b - a == K && !row_lt(dk[i], dv[i], ok[a], ov[a])) refill[g] = 1;
    }
}

__global__ void k_topk_refill_ranges(const uint64_t *refill,
                                     const uint64_t *rscan, int64_t ng,
                                     const uint64_t *glo, const uint64_t *ghi,
                                     uint64_t *rlo, uint64_t *rhi) {
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < ng;
         g += (int64_t)gridDim.x * blockDim.x) {
        if (!refill[g]) continue;
        rlo[rscan[g]] = glo[g];
        rhi[rscan[g]] = ghi[g];
    }
}

// Candidates of the groups that are not refilled, over the index space
// [0, no) = the current top-K rows, [no, no + n) = the delta rows: a top-K
// row stays, an appear row enters, a vanish row enters (negated) iff it is a
// top-K row.  Rows of refilled groups stay out: those groups come from the
// input integral with their real weights.
__global__ void k_topk_cand_flags(const uint64_t *dk, const uint64_t *dv,
                                  const int64_t *cls, const uint64_t *gidx,
                                  int64_t n, const uint64_t *glo, int64_t ng,
                                  const uint64_t *refill, const uint64_t *ok,
                                  const uint64_t *ov, int64_t no,
                                  uint64_t *flags) {
    const int64_t tot = no + n;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < tot;
         j += (int64_t)gridDim.x * blockDim.x) {
        uint64_t f;
        if (j < no) {
            // every top-K row lies in an affected group: it was gathered by
            // that group's range, and glo[0] <= its key
            const int64_t g = upper_bound_k(glo, ng, ok[j]) - 1;
            f = g >= 0 && !refill[g];
        } else {
            const int64_t i = j - no;
            const int64_t c = cls[i];
            f = 0;
            if (c != 0 && !refill[gidx[i]]) {
                f = 1;
                if (c < 0) {
                    const int64_t p = lex_lower(ok, ov, 0, no, dk[i], dv[i]);
                    f = p < no && ok[p] == dk[i] && ov[p] == dv[i];
                }
            }
        }
        flags[j] = f;
    }
}

__global__ void k_topk_cand_emit(const uint64_t *dk, const uint64_t *dv,
                                 const int64_t *cls, int64_t n,
                                 const uint64_t *ok, const uint64_t *ov,
                                 int64_t no, const uint64_t *flags,
                                 const uint64_t *fscan, uint64_t *ck,
                                 uint64_t *cv, int64_t *cw) {
    const int64_t tot = no + n;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < tot;
         j += (int64_t)gridDim.x * blockDim.x) {
        if (!flags[j]) continue;
        const uint64_t o = fscan[j];
        if (j < no) {
            ck[o] = ok[j]; cv[o] = ov[j]; cw[o] = 1;
        } else {
            const int64_t i = j - no;
            ck[o] = dk[i]; cv[o] = dv[i]; cw[o] = cls[i];
        }
    }
}

// a row of the consolidated slice is selected iff at most K - 1 rows follow
// it inside its group: the group's end is one binary search over the keys
__global__ void k_topk_select_flags(const uint64_t *sk, int64_t n, int shift,
                                    int64_t K, uint64_t *flags) {
    const uint64_t mask = topk_mask(shift);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t from = i + 1;
        const int64_t end =
            from + upper_bound_k(sk + from, n - from, sk[i] | mask);
        flags[i] = end - i <= K;
    }
}

__global__ void k_topk_select_emit(const uint64_t *sk, const uint64_t *sv,
                                   int64_t n, const uint64_t *flags,
                                   const uint64_t *fscan, uint64_t *ok,
                                   uint64_t *ov, int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!flags[i]) continue;
        const uint64_t o = fscan[i];
        ok[o] = sk[i]; ov[o] = sv[i]; ow[o] = 1;
    }
}

dbsp_status topk_classify(hipStream_t s, const Rows &delta, const TraceArgs &t,
                          int shift, uint64_t **plan, int64_t *n_groups) {
    const int64_t n = delta.n;
    *plan = nullptr;
    *n_groups = 0;
    if (n <= 0) return DBSP_OK;
    Scratch sc(s);
    uint64_t *heads, *hscan, *pb;
    HIP_CHECK(sc.get(&heads, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&hscan, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&pb, 4 * n * sizeof(uint64_t)));
    k_topk_classify<<<grid_for(n), BLK, 0, s>>>(delta.k, delta.v, delta.w, n, t,
                                                shift, (int64_t *)pb, heads);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, heads, hscan, n, &total));
    k_topk_groups<<<grid_for(n), BLK, 0, s>>>(delta.k, n, shift, heads, hscan,
                                              pb + n, pb + 2 * n, pb + 3 * n);
    *n_groups = (int64_t)total;
    sc.keep(pb);
    *plan = pb;
    return DBSP_OK;
}

dbsp_status keyrange_gather(hipStream_t s, const uint64_t *klo,
                            const uint64_t *khi, int64_t nr,
                            const TraceArgs &t, int64_t sign, Rows *out) {
    if (nr <= 0 || t.nb <= 0) return no_rows(out);
    const int64_t np = nr * t.nb;
    Scratch sc(s);
    uint64_t *cnt, *start;
    HIP_CHECK(sc.get(&cnt, np * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&start, np * sizeof(uint64_t)));
    k_keyrange_count<<<grid_for(np), BLK, 0, s>>>(klo, khi, nr, t, cnt, start);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, cnt, cnt, np, &total));
    if (total == 0) return no_rows(out);
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)total, &r));
    k_range_emit<<<grid_for((int64_t)total), BLK, 0, s>>>(
        t, np, cnt, start, (int64_t)total, sign, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

dbsp_status topk_verdict(hipStream_t s, const Rows &delta,
                         const uint64_t *plan, int64_t ng, const Rows &cur,
                         int64_t K, bool refill_all, uint64_t **verdict,
                         int64_t *n_refill) {
    const int64_t n = delta.n;
    *verdict = nullptr;
    *n_refill = 0;
    if (n <= 0 || ng <= 0) return DBSP_OK;
    const int64_t *cls = (const int64_t *)plan;
    const uint64_t *gidx = plan + n, *glo = plan + 2 * n, *ghi = plan + 3 * n;
    Scratch sc(s);
    uint64_t *vb, *rscan;
    HIP_CHECK(sc.get(&vb, 3 * ng * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&rscan, ng * sizeof(uint64_t)));
    if (refill_all) {
        k_fill_u64<<<grid_for(ng), BLK, 0, s>>>(vb, 1, ng);
    } else {
        HIP_CHECK(hipMemsetAsync(vb, 0, ng * sizeof(uint64_t), s));
        k_topk_verdict<<<grid_for(n), BLK, 0, s>>>(delta.k, delta.v, cls, gidx,
                                                   n, glo, ghi, cur.k, cur.v,
                                                   cur.n, K, vb);
    }
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, vb, rscan, ng, &total));
    if (total > 0)
        k_topk_refill_ranges<<<grid_for(ng), BLK, 0, s>>>(
            vb, rscan, ng, glo, ghi, vb + ng, vb + 2 * ng);
    *n_refill = (int64_t)total;
    sc.keep(vb);
    *verdict = vb;
    return DBSP_OK;
}

dbsp_status topk_candidates(hipStream_t s, const Rows &delta,
                            const uint64_t *plan, int64_t ng,
                            const uint64_t *refill, const Rows &cur,
                            Rows *out) {
    const int64_t n = delta.n, no = cur.n, tot = n + no;
    if (n <= 0 || ng <= 0) return no_rows(out);
    const int64_t *cls = (const int64_t *)plan;
    const uint64_t *gidx = plan + n, *glo = plan + 2 * n;
    Scratch sc(s);
    uint64_t *flags, *fscan;
    HIP_CHECK(sc.get(&flags, tot * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, tot * sizeof(uint64_t)));
    k_topk_cand_flags<<<grid_for(tot), BLK, 0, s>>>(delta.k, delta.v, cls,
                                                    gidx, n, glo, ng, refill,
                                                    cur.k, cur.v, no, flags);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, flags, fscan, tot, &total));
    if (total == 0) return no_rows(out);
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)total, &r));
    k_topk_cand_emit<<<grid_for(tot), BLK, 0, s>>>(delta.k, delta.v, cls, n,
                                                   cur.k, cur.v, no, flags,
                                                   fscan, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

dbsp_status topk_select(hipStream_t s, const Rows &slice, int64_t K, int shift,
                        Rows *out) {
    const int64_t n = slice.n;
    if (n <= 0) return no_rows(out);
    Scratch sc(s);
    uint64_t *flags, *fscan;
    HIP_CHECK(sc.get(&flags, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, n * sizeof(uint64_t)));
    k_topk_select_flags<<<grid_for(n), BLK, 0, s>>>(slice.k, n, shift, K,
                                                    flags);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, flags, fscan, n, &total));
    if (total == 0) return no_rows(out);
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)total, &r));
    k_topk_select_emit<<<grid_for(n), BLK, 0, s>>>(slice.k, slice.v, n, flags,
                                                   fscan, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

// Query 19's front (queries/q19.rs: bids.flat_map_index(|b| (b.auction,
// (b.price, b)))), a kernel of its own as k_flatmap_bid_tv is, so that
// k_flatmap (on q3's measured path) stays as it is.  Stream
// 0: k = auction << 27 | price, v = bidder << 32 | date_time, so (k, v) order
// is (auction, price, bidder, date_time) order.  Stream 1 collects the bids
// with a field too wide for its place, as (auction, price, w): its counter is
// the step's error word, read back with the lengths the step syncs on anyway.
__global__ __launch_bounds__(FLATMAP_BLK) void k_flatmap_bid_topk(
        const dbsp_event *ev, dbspk::EventCols cols, int64_t n, uint64_t *c0,
        uint64_t *k0, uint64_t *v0, int64_t *w0, int64_t cap0, uint64_t *c1,
        uint64_t *k1, uint64_t *v1, int64_t *w1, int64_t cap1) {
    __shared__ uint32_t s_cnt[2][FLATMAP_WAVES];
    __shared__ unsigned long long s_base[2][FLATMAP_WAVES];
    const int64_t stride = (int64_t)gridDim.x * FLATMAP_BLK;
    for (int64_t base = blockIdx.x * (int64_t)FLATMAP_BLK; base < n;
         base += stride) {
        const int64_t i = base + threadIdx.x;
        uint64_t kind = 0, auction = 0, bidder = 0, price = 0, dt = 0;
        int64_t w = 0;
        if (i < n) {
            if (cols.kind) {
                kind = cols.kind[i]; auction = cols.f0[i]; bidder = cols.f1[i];
                price = cols.f2[i]; dt = cols.f3[i]; w = cols.w[i];
            } else {
                const dbsp_event e = ev[i];
                kind = e.kind; auction = e.f0; bidder = e.f1; price = e.f2;
                dt = e.f3; w = e.w;
            }
        }
        const bool bid = i < n && kind == 2;
        const bool wide = (auction >> 37) || (price >> 27) || (bidder >> 32) ||
                          (dt >> 32);
        const bool p0 = bid && !wide, p1 = bid && wide;
        uint64_t pos0, pos1;
        block_append2((unsigned long long *)c0, (unsigned long long *)c1, p0,
                      p1, s_cnt, s_base, pos0, pos1);
        if (p0 && pos0 < (uint64_t)cap0) {
            k0[pos0] = (auction << 27) | price;
            v0[pos0] = (bidder << 32) | dt;
            w0[pos0] = w;
        }
        if (p1 && pos1 < (uint64_t)cap1) {
            k1[pos1] = auction; v1[pos1] = price; w1[pos1] = w;
        }
    }
}

// ---------------------------------------------------------------------------
// Incremental antijoin / semijoin (Stream::antijoin, operator/join.rs:294-320:
// A - A |><| distinct(B), as ONE operator over two spines).  The right side is
// a key set stored as rows (k, 0, w); a key is PRESENT iff its total weight
// over every batch of its spine is > 0 (operator/distinct.rs), so a key at
// net -1 is absent.
//   k_anti_flip            per key of the consolidated dB: its weight in the
//                          right spine before the tick (one lower_bound_k per
//                          batch, a batch holds a key at most once) ->
//                          flip = [before + dw > 0] - [before > 0]
//   k_anti_flip_emit       flags + scan -> the flipped keys and their signed
//                          multiplier (-flip antijoin, +flip semijoin)
//   k_keyrange_count       the flipped keys' runs of the left spine
//   k_range_emit_mul       k_range_emit with a multiplier per range instead
//                          of one sign per launch, over the OUTPUT index space
//   k_anti_heads           key-head flags of the consolidated dA
//   k_anti_present         one search per key HEAD: present after the tick
//   k_anti_keep            a row is kept iff anti != present[its head]
//   k_anti_emit            flags + scan -> the kept rows
// Every data-dependent size is flags -> scan -> emit; nothing passes between
// workgroups.
// ---------------------------------------------------------------------------

// total weight of key over every batch of a key-set spine
__device__ inline int64_t anti_weight(const TraceArgs &t, uint64_t key) {
    int64_t sum = 0;
    for (int b = 0; b < t.nb; b++) {
        const int64_t nb = t.n[b];
        const int64_t j = lower_bound_k(t.k[b], nb, key);
        if (j < nb && t.k[b][j] == key) sum += t.w[b][j];
    }
    return sum;
}

__global__ void k_anti_flip(const uint64_t *bk, const int64_t *bw, int64_t n,
                            TraceArgs t, int64_t *flip, uint64_t *flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t before = anti_weight(t, bk[i]);
        const int64_t f =
            (int64_t)(before + bw[i] > 0) - (int64_t)(before > 0);
        flip[i] = f;
        flags[i] = f != 0;
    }
}

__global__ void k_anti_flip_emit(const uint64_t *bk, const int64_t *flip,
                                 const uint64_t *flags, const uint64_t *fscan,
                                 int64_t n, int64_t sign, uint64_t *fkey,
                                 int64_t *fmul) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!flags[i]) continue;
        const uint64_t o = fscan[i];
        fkey[o] = bk[i];
        fmul[o] = sign * flip[i];
    }
}

// k_range_emit with the weight multiplier read per range (pair j belongs to
// range j / t.nb): one thread per OUTPUT row, so a key with 100,000 values
// costs 100,000 threads, not one thread's loop
__global__ void k_range_emit_mul(TraceArgs t, int64_t np,
                                 const uint64_t *offsets, const uint64_t *start,
                                 int64_t n_out, const int64_t *mul,
                                 uint64_t *ok, uint64_t *ov, int64_t *ow) {
    for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < n_out;
         o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = upper_bound_k(offsets, np, (uint64_t)o) - 1;
        const int b = (int)(j % t.nb);
        const int64_t src = (int64_t)start[j] + (o - (int64_t)offsets[j]);
        ok[o] = t.k[b][src];
        ov[o] = t.v[b][src];
        ow[o] = mul[j / t.nb] * t.w[b][src];
    }
}

__global__ void k_anti_heads(const uint64_t *ak, int64_t n, uint64_t *heads) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        heads[i] = i == 0 || ak[i - 1] != ak[i];
}

// present[h]: the key of head number h is present in the key-set spine
__global__ void k_anti_present(const uint64_t *ak, int64_t n,
                               const uint64_t *heads, const uint64_t *hscan,
                               TraceArgs t, uint64_t *present) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!heads[i]) continue;
        present[hscan[i]] = anti_weight(t, ak[i]) > 0;
    }
}

// row 0 is a head, so hscan[i] + heads[i] - 1 is the row's head number
__global__ void k_anti_keep(int64_t n, const uint64_t *heads,
                            const uint64_t *hscan, const uint64_t *present,
                            int anti, uint64_t *flags) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        flags[i] = (anti != 0) != (present[hscan[i] + heads[i] - 1] != 0);
}

__global__ void k_anti_emit(const uint64_t *ak, const uint64_t *av,
                            const int64_t *aw, int64_t n, const uint64_t *flags,
                            const uint64_t *fscan, uint64_t *ok, uint64_t *ov,
                            int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!flags[i]) continue;
        const uint64_t o = fscan[i];
        ok[o] = ak[i]; ov[o] = av[i]; ow[o] = aw[i];
    }
}

dbsp_status anti_flip(hipStream_t s, const Rows &db, const TraceArgs &t,
                      bool anti, uint64_t **plan, int64_t *n_flip) {
    const int64_t n = db.n;
    *plan = nullptr;
    *n_flip = 0;
    if (n <= 0) return DBSP_OK;
    Scratch sc(s);
    uint64_t *flags, *fscan, *pb;
    int64_t *flip;
    HIP_CHECK(sc.get(&flip, n * sizeof(int64_t)));
    HIP_CHECK(sc.get(&flags, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, n * sizeof(uint64_t)));
    k_anti_flip<<<grid_for(n), BLK, 0, s>>>(db.k, db.w, n, t, flip, flags);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, flags, fscan, n, &total));
    if (total == 0) return DBSP_OK;
    HIP_CHECK(sc.get(&pb, 2 * total * sizeof(uint64_t)));
    k_anti_flip_emit<<<grid_for(n), BLK, 0, s>>>(
        db.k, flip, flags, fscan, n, anti ? -1 : 1, pb,
        (int64_t *)(pb + total));
    *n_flip = (int64_t)total;
    sc.keep(pb);
    *plan = pb;
    return DBSP_OK;
}

dbsp_status keyrange_gather_mul(hipStream_t s, const uint64_t *keys,
                                const int64_t *mul, int64_t nr,
                                const TraceArgs &t, Rows *out) {
    if (nr <= 0 || t.nb <= 0) return no_rows(out);
    const int64_t np = nr * t.nb;
    Scratch sc(s);
    uint64_t *cnt, *start;
    HIP_CHECK(sc.get(&cnt, np * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&start, np * sizeof(uint64_t)));
    k_keyrange_count<<<grid_for(np), BLK, 0, s>>>(keys, keys, nr, t, cnt,
                                                  start);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, cnt, cnt, np, &total));
    if (total == 0) return no_rows(out);
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)total, &r));
    k_range_emit_mul<<<grid_for((int64_t)total), BLK, 0, s>>>(
        t, np, cnt, start, (int64_t)total, mul, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

dbsp_status anti_filter(hipStream_t s, const Rows &a, const TraceArgs &t,
                        bool anti, Rows *out) {
    const int64_t n = a.n;
    if (n <= 0) return no_rows(out);
    Scratch sc(s);
    uint64_t *heads, *hscan, *present, *flags;
    HIP_CHECK(sc.get(&heads, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&hscan, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&present, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&flags, n * sizeof(uint64_t)));
    k_anti_heads<<<grid_for(n), BLK, 0, s>>>(a.k, n, heads);
    TRY_K(scan_exclusive(s, heads, hscan, n, nullptr));
    k_anti_present<<<grid_for(n), BLK, 0, s>>>(a.k, n, heads, hscan, t,
                                               present);
    k_anti_keep<<<grid_for(n), BLK, 0, s>>>(n, heads, hscan, present, anti,
                                            flags);
    // the head flags are spent: their column takes the second scan
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, flags, heads, n, &total));
    if (total == 0) return no_rows(out);
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)total, &r));
    k_anti_emit<<<grid_for(n), BLK, 0, s>>>(a.k, a.v, a.w, n, flags, heads,
                                            r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

// Query 103's front (auctions.map_index(|a| (a.id, a.seller)) and
// bids.map_index(|b| (b.auction, ()))), a kernel of its own as
// k_flatmap_bid_tv is, so that k_flatmap (on q3's measured path) stays as it
// is.  Stream 0: auctions as (id, seller, w); stream 1: bids as the key rows
// (auction, 0, w) of the antijoin's right side.
__global__ __launch_bounds__(FLATMAP_BLK) void k_flatmap_auction_bidkey(
        const dbsp_event *ev, dbspk::EventCols cols, int64_t n, uint64_t *c0,
        uint64_t *k0, uint64_t *v0, int64_t *w0, int64_t cap0, uint64_t *c1,
        uint64_t *k1, uint64_t *v1, int64_t *w1, int64_t cap1) {
    __shared__ uint32_t s_cnt[2][FLATMAP_WAVES];
    __shared__ unsigned long long s_base[2][FLATMAP_WAVES];
    const int64_t stride = (int64_t)gridDim.x * FLATMAP_BLK;
    for (int64_t base = blockIdx.x * (int64_t)FLATMAP_BLK; base < n;
         base += stride) {
        const int64_t i = base + threadIdx.x;
        uint64_t kind = 0, f0 = 0, f1 = 0;
        int64_t w = 0;
        if (i < n) {
            if (cols.kind) {
                kind = cols.kind[i]; f0 = cols.f0[i]; f1 = cols.f1[i];
                w = cols.w[i];
            } else {
                const dbsp_event e = ev[i];
                kind = e.kind; f0 = e.f0; f1 = e.f1; w = e.w;
            }
        }
        const bool p0 = i < n && kind == 1, p1 = i < n && kind == 2;
        uint64_t pos0, pos1;
        block_append2((unsigned long long *)c0, (unsigned long long *)c1, p0,
                      p1, s_cnt, s_base, pos0, pos1);
        if (p0 && pos0 < (uint64_t)cap0) {
            k0[pos0] = f0; v0[pos0] = f1; w0[pos0] = w;
        }
        if (p1 && pos1 < (uint64_t)cap1) {
            k1[pos1] = f0; v1[pos1] = 0; w1[pos1] = w;
        }
    }
}

// ---------------------------------------------------------------------------
// Incremental arg-max per group, ties kept (the tail of
// crates/nexmark/src/queries/q7.rs:82-93: aggregate(Min) over the negated
// price joined back on the price; SQL's RANK() OVER (PARTITION BY g ORDER BY
// x DESC) = 1).  A row's group is k >> group_shift, its rank k >> rank_shift
// with rank_shift <= group_shift, so equal ranks imply one group and (k, v)
// order is (group, rank, tie) order.  The relation holds, per group, every
// present row of the group's largest present rank AT ITS OWN WEIGHT.
// Divergence from the reference: Min::aggregate
// (operator/aggregate/min.rs:38-57) sums the weights of all rows sharing a
// price and skips the price when that sum is zero; here a rank stays present
// as long as any single row at it is present.  The two agree whenever the
// weights are positive; they differ only when different rows at one rank
// carry weights of mixed sign that cancel.
// Classify, the group list and both gathers are the top-K ones
// (k_topk_classify, k_topk_groups, k_keyrange_count, k_range_emit,
// k_topk_refill_ranges).  New here:
//   k_argmax_verdict       over Oc ++ D: a group's refill flag starts at 1
//                          and every keep event stores the same 0
//   k_argmax_cand_flags/emit  the candidate rows of the groups NOT refilled
//   k_argmax_select_flags/emit  a slice row is kept iff its rank is the rank
//                          of its group's last row: one binary search per row
//   k_negate_weights       -Oc for the output merge
// Every data-dependent size is flags -> scan -> emit; nothing passes between
// workgroups.
// ---------------------------------------------------------------------------

// ok/ov: the affected groups' current tie sets, consolidated.  The group
// keeps its maximum (no refill) iff an Oc row is not taken away by a vanish
// row of D, or a delta row that is present after the tick has a rank >= the
// rank of Oc_g.  A group whose Oc_g is empty had no present row: any of its
// delta rows clears the flag.
__global__ void k_argmax_verdict(const uint64_t *dk, const uint64_t *dv,
                                 const int64_t *cls, const uint64_t *gidx,
                                 int64_t n, const uint64_t *glo,
                                 const uint64_t *ghi, int64_t ng,
                                 const uint64_t *ok, const uint64_t *ov,
                                 int64_t no, int rank_shift,
                                 uint64_t *refill) {
    const int64_t tot = no + n;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < tot;
         j += (int64_t)gridDim.x * blockDim.x) {
        if (j < no) {
            const uint64_t k = ok[j], v = ov[j];
            const int64_t p = lex_lower(dk, dv, 0, n, k, v);
            const bool gone = p < n && dk[p] == k && dv[p] == v && cls[p] < 0;
            if (!gone) {
                // every Oc row lies in an affected group: it was gathered by
                // that group's range, and glo[0] <= its key
                const int64_t g = upper_bound_k(glo, ng, k) - 1;
                if (g >= 0) refill[g] = 0;
            }
        } else {
            const int64_t i = j - no;
            const uint64_t g = gidx[i];
            const int64_t a = lower_bound_k(ok, no, glo[g]);
            const bool empty = a >= no || ok[a] > ghi[g];
            if (empty || (cls[i] >= 0 &&
                          (dk[i] >> rank_shift) >= (ok[a] >> rank_shift)))
                refill[g] = 0;
        }
    }
}

// Candidates of the groups that are not refilled, over the index space
// [0, no) = Oc, [no, no + n) = D: an Oc row enters at its weight, a delta row
// at dw iff its rank is >= the rank of Oc_g (every delta row when Oc_g is
// empty).  A delta row above Oc_g's rank was absent before, one at that rank
// is in Oc_g or was absent: the sums are the rows' new integral weights.
__global__ void k_argmax_cand_flags(const uint64_t *dk, const uint64_t *gidx,
                                    int64_t n, const uint64_t *glo,
                                    const uint64_t *ghi, int64_t ng,
                                    const uint64_t *refill, const uint64_t *ok,
                                    int64_t no, int rank_shift,
                                    uint64_t *flags) {
    const int64_t tot = no + n;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < tot;
         j += (int64_t)gridDim.x * blockDim.x) {
        uint64_t f = 0;
        if (j < no) {
            const int64_t g = upper_bound_k(glo, ng, ok[j]) - 1;
            f = g >= 0 && !refill[g];
        } else {
            const int64_t i = j - no;
            const uint64_t g = gidx[i];
            if (!refill[g]) {
                const int64_t a = lower_bound_k(ok, no, glo[g]);
                f = a >= no || ok[a] > ghi[g] ||
                    (dk[i] >> rank_shift) >= (ok[a] >> rank_shift);
            }
        }
        flags[j] = f;
    }
}

__global__ void k_argmax_cand_emit(const uint64_t *dk, const uint64_t *dv,
                                   const int64_t *dw, int64_t n,
                                   const uint64_t *ok, const uint64_t *ov,
                                   const int64_t *ow, int64_t no,
                                   const uint64_t *flags,
                                   const uint64_t *fscan, uint64_t *ck,
                                   uint64_t *cv, int64_t *cw) {
    const int64_t tot = no + n;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < tot;
         j += (int64_t)gridDim.x * blockDim.x) {
        if (!flags[j]) continue;
        const uint64_t o = fscan[j];
        if (j < no) {
            ck[o] = ok[j]; cv[o] = ov[j]; cw[o] = ow[j];
        } else {
            const int64_t i = j - no;
            ck[o] = dk[i]; cv[o] = dv[i]; cw[o] = dw[i];
        }
    }
}

// a row of the consolidated slice is selected iff its rank is the rank of the
// last row of its group: the group's end is one binary search over the keys
__global__ void k_argmax_select_flags(const uint64_t *sk, int64_t n,
                                      int group_shift, int rank_shift,
                                      uint64_t *flags) {
    const uint64_t mask = topk_mask(group_shift);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t from = i + 1;
        const int64_t end =
            from + upper_bound_k(sk + from, n - from, sk[i] | mask);
        flags[i] = (sk[end - 1] >> rank_shift) == (sk[i] >> rank_shift);
    }
}

__global__ void k_argmax_select_emit(const uint64_t *sk, const uint64_t *sv,
                                     const int64_t *sw, int64_t n,
                                     const uint64_t *flags,
                                     const uint64_t *fscan, uint64_t *ok,
                                     uint64_t *ov, int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!flags[i]) continue;
        const uint64_t o = fscan[i];
        ok[o] = sk[i]; ov[o] = sv[i]; ow[o] = sw[i];
    }
}

__global__ void k_negate_weights(int64_t *w, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        w[i] = -w[i];
}

dbsp_status argmax_verdict(hipStream_t s, const Rows &delta,
                           const uint64_t *plan, int64_t ng, const Rows &cur,
                           int rank_shift, bool refill_all, uint64_t **verdict,
                           int64_t *n_refill) {
    const int64_t n = delta.n;
    *verdict = nullptr;
    *n_refill = 0;
    if (n <= 0 || ng <= 0) return DBSP_OK;
    const int64_t *cls = (const int64_t *)plan;
    const uint64_t *gidx = plan + n, *glo = plan + 2 * n, *ghi = plan + 3 * n;
    Scratch sc(s);
    uint64_t *vb, *rscan;
    HIP_CHECK(sc.get(&vb, 3 * ng * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&rscan, ng * sizeof(uint64_t)));
    k_fill_u64<<<grid_for(ng), BLK, 0, s>>>(vb, 1, ng);
    if (!refill_all)
        k_argmax_verdict<<<grid_for(cur.n + n), BLK, 0, s>>>(
            delta.k, delta.v, cls, gidx, n, glo, ghi, ng, cur.k, cur.v, cur.n,
            rank_shift, vb);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, vb, rscan, ng, &total));
    if (total > 0)
        k_topk_refill_ranges<<<grid_for(ng), BLK, 0, s>>>(
            vb, rscan, ng, glo, ghi, vb + ng, vb + 2 * ng);
    *n_refill = (int64_t)total;
    sc.keep(vb);
    *verdict = vb;
    return DBSP_OK;
}

dbsp_status argmax_candidates(hipStream_t s, const Rows &delta,
                              const uint64_t *plan, int64_t ng,
                              const uint64_t *refill, const Rows &cur,
                              int rank_shift, Rows *out) {
    const int64_t n = delta.n, no = cur.n, tot = n + no;
    if (n <= 0 || ng <= 0) return no_rows(out);
    const uint64_t *gidx = plan + n, *glo = plan + 2 * n, *ghi = plan + 3 * n;
    Scratch sc(s);
    uint64_t *flags, *fscan;
    HIP_CHECK(sc.get(&flags, tot * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, tot * sizeof(uint64_t)));
    k_argmax_cand_flags<<<grid_for(tot), BLK, 0, s>>>(
        delta.k, gidx, n, glo, ghi, ng, refill, cur.k, no, rank_shift, flags);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, flags, fscan, tot, &total));
    if (total == 0) return no_rows(out);
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)total, &r));
    k_argmax_cand_emit<<<grid_for(tot), BLK, 0, s>>>(
        delta.k, delta.v, delta.w, n, cur.k, cur.v, cur.w, no, flags, fscan,
        r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

dbsp_status argmax_select(hipStream_t s, const Rows &slice, int group_shift,
                          int rank_shift, Rows *out) {
    const int64_t n = slice.n;
    if (n <= 0) return no_rows(out);
    Scratch sc(s);
    uint64_t *flags, *fscan;
    HIP_CHECK(sc.get(&flags, n * sizeof(uint64_t)));
    HIP_CHECK(sc.get(&fscan, n * sizeof(uint64_t)));
    k_argmax_select_flags<<<grid_for(n), BLK, 0, s>>>(slice.k, n, group_shift,
                                                      rank_shift, flags);
    uint64_t total = 0;
    TRY_K(scan_exclusive(s, flags, fscan, n, &total));
    if (total == 0) return no_rows(out);
    Rows r;
    TRY_K(alloc_rows(sc, (int64_t)total, &r));
    k_argmax_select_emit<<<grid_for(n), BLK, 0, s>>>(
        slice.k, slice.v, slice.w, n, flags, fscan, r.k, r.v, r.w);
    return give_rows(sc, r, out);
}

void negate_weights(hipStream_t s, int64_t *w, int64_t n) {
    if (n > 0) k_negate_weights<<<grid_for(n), BLK, 0, s>>>(w, n);
}

// Query 7's front (queries/q7.rs:47-54: bids indexed by date_time), a kernel
// of its own as k_flatmap_bid_tv is, so that k_flatmap (on q3's measured
// path) stays as it is.  Stream 0: k = date_time << 27 | price, v = auction
// << 32 | bidder, so key order is time order and the window stage's bounds
// are date_time << 27.  Stream 1 collects the bids with a field too wide for
// its place, as (date_time, price, w): its counter is the step's error word,
// read back with the lengths the step syncs on anyway.
__global__ __launch_bounds__(FLATMAP_BLK) void k_flatmap_bid_time(
        const dbsp_event *ev, dbspk::EventCols cols, int64_t n, uint64_t *c0,
        uint64_t *k0, uint64_t *v0, int64_t *w0, int64_t cap0, uint64_t *c1,
        uint64_t *k1, uint64_t *v1, int64_t *w1, int64_t cap1) {
    __shared__ uint32_t s_cnt[2][FLATMAP_WAVES];
    __shared__ unsigned long long s_base[2][FLATMAP_WAVES];
    const int64_t stride = (int64_t)gridDim.x * FLATMAP_BLK;
    for (int64_t base = blockIdx.x * (int64_t)FLATMAP_BLK; base < n;
         base += stride) {
        const int64_t i = base + threadIdx.x;
        uint64_t kind = 0, auction = 0, bidder = 0, price = 0, dt = 0;
        int64_t w = 0;
        if (i < n) {
            if (cols.kind) {
                kind = cols.kind[i]; auction = cols.f0[i]; bidder = cols.f1[i];
                price = cols.f2[i]; dt = cols.f3[i]; w = cols.w[i];
            } else {
                const dbsp_event e = ev[i];
                kind = e.kind; auction = e.f0; bidder = e.f1; price = e.f2;
                dt = e.f3; w = e.w;
            }
        }
        const bool bid = i < n && kind == 2;
        const bool wide = (auction >> 32) || (price >> 27) || (bidder >> 32) ||
                          (dt >> 32);
        const bool p0 = bid && !wide, p1 = bid && wide;
        uint64_t pos0, pos1;
        block_append2((unsigned long long *)c0, (unsigned long long *)c1, p0,
                      p1, s_cnt, s_base, pos0, pos1);
        if (p0 && pos0 < (uint64_t)cap0) {
            k0[pos0] = (dt << 27) | price;
            v0[pos0] = (auction << 32) | bidder;
            w0[pos0] = w;
        }
        if (p1 && pos1 < (uint64_t)cap1) {
            k1[pos1] = dt; v1[pos1] = price; w1[pos1] = w;
        }
    }
}

// q7.rs:74-79, bids_by_price: a windowed row (date_time << 27 | price, v, w)
// becomes (price << 32 | date_time, v, w).  Not order-preserving.
__global__ void k_map_price_time(const uint64_t *ik, const uint64_t *iv,
                                 const int64_t *iw, int64_t n, uint64_t *ok,
                                 uint64_t *ov, int64_t *ow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = ik[i];
        ok[i] = ((k & ((1ull << 27) - 1)) << 32) | (k >> 27);
        ov[i] = iv[i];
        ow[i] = iw[i];
    }
}

dbsp_status map_price_time(hipStream_t s, const Rows &in, const Rows &out) {
    if (in.n > 0)
        k_map_price_time<<<grid_for(in.n), BLK, 0, s>>>(in.k, in.v, in.w, in.n,
                                                        out.k, out.v, out.w);
    return DBSP_OK;
}

uint64_t host_xxh3_u64(uint64_t key, uint64_t seed) {
    // host copy of dev_xxh3_u64 (kept in sync; parity-tested against the oracle)
    const uint64_t SEC8_16 = 0x1cad21f72c81017cull ^ 0xdb979083e96dd4deull;
    uint64_t s = seed ^ ((uint64_t)__builtin_bswap32((uint32_t)seed) << 32);
    uint64_t input64 = (uint64_t)(uint32_t)(key >> 32) + ((uint64_t)(uint32_t)key << 32);
    uint64_t h = input64 ^ (SEC8_16 - s);
    uint64_t r49 = (h << 49) | (h >> 15);
    uint64_t r24 = (h << 24) | (h >> 40);
    h ^= r49 ^ r24;
    h *= 0x9FB21C651E98DF25ull;
    h ^= (h >> 35) + 8;
    h *= 0x9FB21C651E98DF25ull;
    h ^= h >> 28;
    return h;
}

}  // namespace dbspk
