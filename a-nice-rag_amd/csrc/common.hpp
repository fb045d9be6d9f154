// Shared host/device definitions of libanrag.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "anrag.h"
#include "host_slots.hpp"
#include "scan_lanes.hpp"

namespace anrag {

constexpr int kWave = 64;            // CDNA wavefront
constexpr int kListLen = 64;         // one top-k slot per lane (ANRAG_FUSED_K_MAX)
constexpr int kScanThreads = 256;    // 4 waves: one scan workgroup per CU (sweep: profiles/r01_scan_config_sweep.txt)
constexpr int kScanWaves = kScanThreads / kWave;
constexpr int kScanGroupMax = 16;  // queries one scan / K3 / tail launch can carry (dense_scan.hip, bm25.hip, tail.hip)
// kPipeSlots (queries in flight, list sets) and kScanLanesMax: scan_lanes.hpp
constexpr int kMaxScanBlocks = 256;  // one per CU
constexpr int kMaxScanLists = kMaxScanBlocks * kScanWaves;  // K1 leaves one sorted list per WAVE (the tail merges them)
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
constexpr int kAllowWords = 2048;    // an allow bitmap: one bit per source id (65536), as the kernels stage it in LDS

void set_error(const char *fmt, ...);

#define ANRAG_HIP(expr)                                                                    \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess) {                                                           \
            ::anrag::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),     \
                               __FILE__, __LINE__);                                        \
            return ANRAG_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)

#define ANRAG_REQUIRE(cond, ...)                                                           \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            ::anrag::set_error(__VA_ARGS__);                                               \
            return ANRAG_ERR_INVALID;                                                      \
        }                                                                                  \
    } while (0)

struct ProfSpan {
    int kernel;
    hipEvent_t start, stop;
    int units;  // queries the bracketed launch carried
};

// Every device / pinned-host allocation and release of the library goes through these four: they count (process-wide)
// so that a test can assert that a steady-state query loop performs none (anrag_debug_alloc_calls) -- hipMalloc and
// hipFree synchronise the whole device.
int64_t alloc_calls();
hipError_t counted_malloc(void **p, size_t bytes);
hipError_t counted_free(void *p);
hipError_t counted_host_malloc(void **p, size_t bytes, unsigned flags);
hipError_t counted_host_free(void *p);
template <typename T>
inline hipError_t counted_malloc(T **p, size_t bytes) { return counted_malloc(reinterpret_cast<void **>(p), bytes); }

// A kernel that asks for more than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize set -- per
// DEVICE: remembered per (device, function) under a mutex, so that indexes on several GPUs of one process are
// independent (include/anrag.h) and concurrent first calls do not race.
int ensure_dynamic_lds(int device, const void *func, int bytes);

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// grow-only device block, freed at anrag_index_destroy
struct DevicePool {
    char *p = nullptr;
    int64_t bytes = 0;
};

// a single query's list merge that rides in the NEXT scan launch of its stream (dense_scan.hip: DeferredTail)
struct PendingTail {
    int set;              // list set the query's scan wrote
    int32_t k;
    anrag_candidate *out;
};

// carve pieces of 256-byte granularity out of one block (base == nullptr: only measure)
struct Carver {
    char *base;
    int64_t at = 0;
    explicit Carver(char *b) : base(b) {}
    template <typename T>
    T *take(int64_t count) {
        T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += (count * (int64_t)sizeof(T) + 255) / 256 * 256;
        return p;
    }
};

// Lay a call's buffers out in a grow-only block: `layout(Carver &)` runs once to measure, `reserve(bytes, &base)` makes
// the block hold that much, `layout` runs again on the block itself.
template <class Reserve, class Layout>
inline int carve_block(Reserve &&reserve, Layout &&layout) {
    Carver measure(nullptr);
    layout(measure);
    char *base = nullptr;
    if (int rc = reserve(measure.at, &base)) return rc;
    Carver real(base);
    layout(real);
    return ANRAG_OK;
}

// allow list (one byte per source, NOT NULL) -> bitmap of kAllowWords words in host memory
int pack_allow_bits(const uint8_t *allow, int32_t n_sources, uint32_t *h_bits);

// k candidate records -> the caller's arrays; *out_count = the records that name a document (padding has doc -1)
template <typename S>
inline void unpack_records(const anrag_candidate *rec, int32_t k, int64_t *out_doc, S *out_score, int32_t *out_count) {
    int32_t cnt = 0;
    for (int32_t i = 0; i < k; ++i) {
        out_doc[i] = rec[i].doc;
        out_score[i] = (S)rec[i].score;
        if (rec[i].doc >= 0) ++cnt;
    }
    *out_count = cnt;
}

}  // namespace anrag

// One GPU's shard.  Everything the kernels touch lives in HBM for the index's lifetime.
struct anrag_index {
    int device = 0;
    int n_cus = 256;
    std::mutex mu;
    // primary: dense scans.  secondary: BM25 + its list merge.  fusion: dense list merge + WRRF (and, in the
    // sharded path, the caller's collectives).  A hybrid query touches all three and never syncs the host.
    hipStream_t own_primary = nullptr, own_secondary = nullptr, own_fusion = nullptr;
    hipStream_t primary = nullptr, secondary = nullptr, fusion = nullptr;
    // hybrid pipeline: slot = query sequence number % kPipeSlots owns one set of dense block lists, one set
    // of BM25 partition lists and three events
    hipEvent_t ev_scan[anrag::kPipeSlots] = {};    // scan of the slot finished (primary)
    hipEvent_t ev_bm25[anrag::kPipeSlots] = {};    // BM25 lists of the slot ready (secondary)
    hipEvent_t ev_fused[anrag::kPipeSlots] = {};   // tail of the slot finished: its lists may be overwritten
    uint64_t hyb_seq = 0;
    bool hyb_outstanding = false;
    // Dense-only queries submitted ONE per call (anrag_dense_search_device, n_queries == 1, the index's own streams):
    // lanes of scans, each lane its own stream, consecutive queries on consecutive lanes.  A query's list merge rides in
    // the next scan launch of its lane (no marker between the scans, no second stream to wake), the lanes' kernels
    // overlap, so one query's launch boundary, ramp and drain are covered by the other lane's streaming.  api.hip.
    struct ScanLane {
        hipStream_t st = nullptr;
        bool pending = false;         // a scan whose lists have not been merged yet
        anrag::PendingTail tail{};
        hipEvent_t ev[4] = {};        // backpressure: recorded every (slots per lane / 4) queries
    };
    ScanLane lane[anrag::kScanLanesMax];
    int n_lanes = 1;                  // configured (ANRAG_SCAN_LANES)
    anrag::ScanLanes lanes;           // which lane and list set the next query takes, which event covers the set's reuse
    hipEvent_t ev_order = nullptr;  // anrag_index_wait_stream / anrag_index_signal_stream
    // host-pointer hybrid queries (anrag_hybrid_search): per-slot staging, so that callers on several threads
    // overlap -- a caller holds the index lock while it enqueues, not while it waits for its result
    struct HostSlot {
        char *h = nullptr;            // pinned: query | terms | allow bitmaps | result records | count
        float *d_query = nullptr;
        int32_t *d_terms = nullptr;
        uint32_t *d_allow_a = nullptr, *d_allow_b = nullptr;
        anrag_candidate *d_out = nullptr;
        int32_t *d_count = nullptr;
        hipEvent_t done = nullptr;
    };
    HostSlot host_slot[anrag::kPipeSlots];
    char *host_slots_h = nullptr, *host_slots_d = nullptr;  // the one pinned / one device block the slots carve
    anrag::HostSlotRing<anrag::kPipeSlots> host_ring;       // busy flags, waiters, the dimension the slots are sized for

    // ---- dense shard: row-major fp32, rows 16-byte aligned when dim % 4 == 0
    float *d_emb = nullptr;
    int64_t n_rows = 0;
    int32_t dim = 0;
    uint16_t *d_dense_src = nullptr;
    int64_t *d_dense_doc = nullptr;
    int64_t dense_doc_base = 0;

    // ---- BM25 shard (see bm25.hip for the layout)
    int64_t n_docs = 0, n_terms = 0, n_postings = 0;
    int64_t *d_indptr = nullptr;       // n_terms + 1
    int32_t *d_post_doc = nullptr;     // n_postings
    double *d_post_impact = nullptr;   // n_postings: tf*(k1+1)/(tf + k1*(1-b+b*dl/avgdl)), fp64
    double *d_idf = nullptr;           // n_terms
    int32_t n_parts = 0, part_docs = 0;  // doc-range partitions (one workgroup each)
    int32_t *d_part_ptr = nullptr;     // per "frequent" term: n_parts+1 offsets (relative to indptr[t])
    int32_t *d_part_slot = nullptr;    // n_terms: row into d_part_ptr, or -1 (rare term: scan whole list)
    uint16_t *d_bm25_src = nullptr;
    int64_t *d_bm25_doc = nullptr;
    int64_t bm25_doc_base = 0;
    double bm25_k1 = 0, bm25_b = 0, bm25_avgdl = 0;

    // ---- workspaces (sized at load; reused by every query on the stream that owns them)
    float *d_blk_score_f32 = nullptr;  // [kPipeSlots][kMaxScanLists][kListLen]
    uint32_t *d_blk_row_a = nullptr;
    double *d_blk_score_f64 = nullptr;  // BM25 per-partition lists [kPipeSlots][n_parts][kListLen]
    uint32_t *d_blk_row_b = nullptr;
    float *d_query = nullptr;           // staged queries
    int64_t query_cap = 0;
    uint32_t *d_allow_a = nullptr, *d_allow_b = nullptr;  // staged allow bitmaps (kAllowWords each)
    int32_t *d_terms = nullptr;         // staged term ids
    anrag_candidate *d_cand_a = nullptr, *d_cand_out = nullptr;
    int64_t cand_cap = 0;
    void *h_pinned = nullptr;           // result staging
    int64_t pinned_bytes = 0;
    float *d_scores_f32 = nullptr;      // full score arrays for k > ANRAG_FUSED_K_MAX
    double *d_scores_f64 = nullptr;
    double *d_dense_scores_f64 = nullptr;  // fp64-query dense path: n_rows scores
    double *d_query_f64 = nullptr;
    double *d_blk_score_f64q = nullptr;    // fp64-query list scan (K1D, dense_scan_f64.hip): ONE set [kMaxScanLists][kListLen]
    bool f64_scan_on = true;               // anrag_set_dense_f64_scan
    int64_t f64_scanned = 0, f64_sorted = 0;  // fp64 queries answered by K1D / by the score array + sort
    int64_t rank_f64_tiled = 0, rank_f64_passed = 0;  // fp64 list queries scored by K1TD / by per-query score passes
    // the shadow prefilter for fp64 queries (K1FD, dense_prefilter_f64.hip): on while a prefilter form is built
    bool f64_pf_on = true;                 // anrag_set_dense_f64_prefilter
    bool f64_pf_ready = false;             // Emax computed for the loaded corpus (the first such query after a load)
    double f64_pf_emax = 0.0;              // largest finite row norm <= 2^60, rounded up
    int64_t f64_pf_queries = 0;            // fp64 queries answered through the prefilter since then
    void *d_sort_tmp = nullptr;
    int64_t sort_tmp_bytes = 0;
    void *d_sort_buf = nullptr;
    int64_t sort_buf_bytes = 0;
    // K2 (batched queries) workspace
    float *d_bq = nullptr, *d_btau = nullptr, *d_bsample = nullptr;
    int32_t *d_bcnt = nullptr, *d_bflag = nullptr;
    void *d_bcand = nullptr;
    int64_t bsample_cap = 0;
    bool batched_split = false;         // K2 arithmetic: false = exact f32 MFMA, true = bf16 x 3 split products
    void *d_bq_hi = nullptr, *d_bq_lo = nullptr;  // bf16 halves of the padded query block
    void *d_split_img = nullptr;        // split-precision K2: the corpus as ready-to-copy LDS images (built on first use)
    int64_t split_img_bytes = 0;
    void *d_bq_img = nullptr;           // ... and the query block in the same form
    // WRRF scratch
    int64_t *d_w_ids = nullptr, *d_w_in = nullptr;
    double *d_w_contrib = nullptr, *d_w_score = nullptr;
    void *d_w_blob = nullptr;           // sort-based long form (sort_select.hip)
    int64_t w_blob_bytes = 0;
    int32_t *d_w_first = nullptr, *d_w_count = nullptr;
    anrag_candidate *d_w_out = nullptr;
    int64_t wrrf_cap = 0;

    // full-ranking batches (rank_batch.hip): score tiles, ranked row lists, fusion arrays -- one grow-only block
    anrag::DevicePool rank_pool;
    // pooled per-call buffers of the host-pointer list entry points (anrag_dense_search with many queries,
    // anrag_hybrid_search_batch): grow-only, so a steady-state loop allocates nothing
    anrag::DevicePool call_pool;
    void *call_pin = nullptr;           // pinned staging of the same calls
    int64_t call_pin_bytes = 0;

    // dense prefilter (dense_prefilter.hip): an fp16 or int8 shadow of the corpus, its per-row data, and per list set
    // the rows' score upper bounds and the threshold T -- one block of one form, dropped by the next dense load / the
    // destroy, or replaced when the mode asks for the other form
    int32_t pf_mode = -1;               // -1 auto (int8, past kScanLanesMaxBytes of fp32 corpus), 0 off, 1 fp16, 2 int8
    bool pf_on = false;
    int32_t pf_form = 0;                // form of pf_block: 0 none, kPrefilterFp16, kPrefilterInt8
    void *pf_block = nullptr;
    int64_t pf_bytes = 0;
    void *d_pf_img = nullptr;           // n_rows x dim fp16 / int8
    float *d_pf_m = nullptr;            // fp16: n_rows radii; int8: n_rows x {s_e, m1, m2, 0}
    float *d_pf_hi = nullptr;           // [kPipeSlots][pf_hi_stride]
    int64_t pf_hi_stride = 0;
    float *d_pf_thr = nullptr;          // [kPipeSlots]
    unsigned long long *d_pf_survivors = nullptr;  // cumulative survivors
    int64_t pf_queries = 0;             // cumulative queries through the prefilter
    // the int8 scan's pair pass (two queries per walk of the image) and the pairing of single fused hybrid calls (api.hip)
    int32_t scan_pair_mode = 1;         // ANRAG_SCAN_PAIR / anrag_set_scan_pairing: 0 off, 1 auto, 2 always hold the odd query
    int64_t pf_pair_passes = 0, pf_single_passes = 0;  // int8 scan passes by form (anrag_scan_pair_stats)
    struct PendingQuery {               // one fused hybrid query held back for a partner
        bool held = false;
        const float *d_query = nullptr;
        const int32_t *d_terms = nullptr;
        int32_t n_terms = 0;
        anrag_candidate *d_out = nullptr;
        int32_t *d_count = nullptr;
        int32_t k = 0, top_n = 0;
        double w_dense = 0, w_bm25 = 0, wrrf_k = 0;
        const uint32_t *allow_dense = nullptr, *allow_bm25 = nullptr;
    } pair_pending;
    int last_scan_slot = -1;            // slot whose ev_scan the pipeline's latest scan launch recorded

    int64_t hbm_bytes = 0;
    int64_t bm25_hbm_bytes = 0;

    // ---- measurement
    bool profiling = false;
    uint32_t profile_mask = 0xFFFFFFFFu;  // bit i: time kernel id i
    uint32_t profile_every = 1;           // bracket every n-th launch of a kernel id
    uint32_t profile_seen[ANRAG_KERNEL_COUNT] = {0};
    std::vector<anrag::ProfSpan> spans;
    std::vector<hipEvent_t> event_pool;
    double prof_ms[ANRAG_KERNEL_COUNT] = {0};
    int64_t prof_launches[ANRAG_KERNEL_COUNT] = {0};
    int64_t prof_units[ANRAG_KERNEL_COUNT] = {0};
};

namespace anrag {

// Upload helper for operands that may already live in HBM (torch tensors): a device-to-device hipMemcpy is NOT
// ordered against the index's non-blocking streams and may return before it has finished, so copy on the
// primary stream and wait for it.  (The caller must have synchronised whatever produced a device operand.)
inline hipError_t copy_in(anrag_index *idx, void *dst, const void *src, size_t bytes) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, idx->primary);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(idx->primary);
}

// Bracket a launch with events when profiling is on.
struct LaunchTimer {
    anrag_index *idx;
    hipStream_t stream;
    int kernel;
    hipEvent_t start = nullptr, stop = nullptr;
    int units;
    LaunchTimer(anrag_index *i, int k, hipStream_t s, int units = 1);
    ~LaunchTimer();
};

int drain_profile(anrag_index *idx);
int pair_flush(anrag_index *idx);       // launch the fused hybrid query held back for a partner, if any (api.hip)
int sync_all(anrag_index *idx);         // wait for the index's three streams
int settle_pipeline(anrag_index *idx);  // ... only when pipeline queries may be outstanding
int ensure_pool(anrag_index *idx, DevicePool &pool, int64_t bytes);  // grow-only (contents are NOT kept)
// carve_block in one of the index's pools, grown to the layout's size plus `slack`
template <class Layout>
inline int carve_pool(anrag_index *idx, DevicePool &pool, int64_t slack, Layout &&layout) {
    return carve_block(
        [&](int64_t bytes, char **base) {
            const int rc = ensure_pool(idx, pool, bytes + slack);
            *base = pool.p;
            return rc;
        },
        layout);
}

// ---- kernel launchers (each enqueues on `stream`, never syncs)
int dense_scan_grid(const anrag_index *idx);
inline int dense_scan_lists(const anrag_index *idx) { return dense_scan_grid(idx) * kScanWaves; }
int dense_scan_vgprs(const anrag_index *idx);  // registers of the scan kernel this index's dimension runs
// K1 alone: one sorted list per workgroup into block-list set `set` (or every score into d_scores_out, k = 0)
int launch_dense_scan(anrag_index *idx, hipStream_t stream, const float *d_query, int32_t k,
                      const uint32_t *d_allow_bits, float *d_scores_out, int set);
constexpr int kTileLaunchMax = 128;  // queries one K1T launch carries (dense_tile.hip)
int dense_tile_group_max(const anrag_index *idx);  // queries K1T holds in LDS at a time at this dimension (0: no tile kernel)
int launch_dense_tile(anrag_index *idx, hipStream_t stream, const float *d_queries, int64_t q_stride, int32_t n_queries,
                      const uint32_t *d_allow_bits, float *d_scores_out, int64_t scores_stride);
// K1TD, fp64 score tiles for lists of float64 queries (dense_tile_f64.hip): up to kTileLaunchMax queries per launch
int dense_tile_f64_group_max(const anrag_index *idx);  // queries K1TD holds in LDS at a time (0: no tile kernel at this dimension)
int launch_dense_tile_f64(anrag_index *idx, hipStream_t stream, const double *d_queries, int64_t q_stride, int32_t n_queries,
                          const uint32_t *d_allow_bits, double *d_scores_out, int64_t scores_stride);
bool dense_tile_mfma_has_shape(const anrag_index *idx);  // ... on the matrix cores (dense_tile_mfma.hip)
int dense_tile_mfma_block_rows(const anrag_index *idx);   // rows per block of that kernel (score rows must hold whole blocks)
int launch_dense_tile_mfma(anrag_index *idx, hipStream_t stream, const float *d_queries, int64_t q_stride, int32_t n_queries,
                           const uint32_t *d_allow_bits, float *d_scores_out, int64_t scores_stride);
bool dense_scan_has_shape(const anrag_index *idx);  // a shaped (not the generic) scan kernel serves this dimension
// K1F / K1F8, the prefiltered dense top-k (dense_prefilter.hip): fp16 or int8 shadow scan -> threshold -> exact
// rescoring of survivors
bool dense_prefilter_has_shape(const anrag_index *idx);
bool dense_prefilter_pairs(const anrag_index *idx, bool filtered);  // the int8 form has a pair kernel for this shape
int dense_prefilter_vgprs(const anrag_index *idx);  // the largest K1F kernel that runs beside K3 (0: no shape)
constexpr int32_t kPrefilterFp16 = 1, kPrefilterInt8 = 2;  // the forms (K1F, K1F8): anrag_set_dense_prefilter's modes
int64_t dense_prefilter_bytes(int64_t n_rows, int32_t dim, int32_t form);
// allocate + convert (syncs the primary stream); no-op when that form is built, drops the other form's block first
int build_dense_prefilter(anrag_index *idx, int32_t form);
void free_dense_prefilter(anrag_index *idx);
struct DeferredTail;
// the scan half (hi, lo lists) and the finish half (threshold + rescore -> the set's exact lists; a lane's DeferredTail
// rides in the rescore launch).  One stream for both, or the finish half on another stream behind an event recorded
// after the scan half: the hybrid pipeline keeps `primary` for the scans alone that way.
int launch_dense_prefilter_scan(anrag_index *idx, hipStream_t stream, const float *const *d_queries, int32_t n_queries,
                                int32_t k, const uint32_t *d_allow_bits, const int *sets);
int launch_dense_prefilter_finish(anrag_index *idx, hipStream_t stream, const float *const *d_queries, int32_t n_queries,
                                  int32_t k, const int *sets, const DeferredTail &dt);
// diagnostics (anrag_debug_prefilter_*): the finish half's threshold launch alone; the scan's rows per wave and batch
int launch_dense_prefilter_threshold(anrag_index *idx, hipStream_t stream, const float *const *d_queries,
                                     int32_t n_queries, int32_t k, const int *sets);
void dense_prefilter_geometry(const anrag_index *idx, int64_t *rows_per_wave, int32_t *batch_rows);
// `finish_later`: when the top-k goes through the prefilter, launch its scan half only; the caller then orders
// launch_dense_scan_finish (same queries, k and sets; a no-op on every other route) behind it on a stream of its choice.
int launch_dense_scan_group(anrag_index *idx, hipStream_t stream, const float *const *d_queries, int32_t n_queries,
                            int32_t k, const uint32_t *d_allow_bits, float *d_scores_out, const int *sets,
                            int64_t scores_stride = 0, const PendingTail *pending = nullptr, bool finish_later = false);
int launch_dense_scan_finish(anrag_index *idx, hipStream_t stream, const float *const *d_queries, int32_t n_queries,
                             int32_t k, const int *sets);
int launch_bm25_lists(anrag_index *idx, hipStream_t st, const int32_t *d_terms, int32_t n_terms, int32_t k,
                      const uint32_t *d_allow_bits, double *d_scores_out, int set);
// the K3 kernel form a launch of n_queries queries takes on this index (bm25.hip; anrag_debug_bm25_geometry reports it)
enum { kBm25FormSmall = 0, kBm25FormWide = 1, kBm25FormTall = 2 };  // <256,4>, <1024,4>, <256,16>
int bm25_form(const anrag_index *idx, int32_t n_queries);
int launch_bm25_lists_group(anrag_index *idx, hipStream_t st, const int32_t *const *d_terms, const int32_t *n_terms,
                            int32_t n_queries, int32_t k, const uint32_t *d_allow_bits, double *const *d_scores_out,
                            const int *sets);
// ... every score of any number of queries in one launch, the queries described in HBM (bm25.hip)
int launch_bm25_scores_table(anrag_index *idx, hipStream_t stream, const int32_t *d_terms_base, const int64_t *d_term_off,
                             int32_t n_queries, const uint32_t *d_allow_bits, double *d_scores_base, int64_t scores_stride);
// Tail of a query, ONE launch (tail.hip): merge the dense block lists of set `set` and/or the BM25 partition
// lists into per-modality top-k, then either write both lists (kTailCandidates: d_out[0..k) dense,
// [k..2k) BM25; with one modality only its k records at d_out[0..k)) or fuse them (kTailFuse: WRRF + top_n).
// kTailCandidates2k: always the two-list layout ([0,k) dense, [k,2k) BM25), an absent leg all padding (doc -1,
// score -inf) -- the shape of one rank's all-gather payload, whatever the query skipped.
enum TailMode { kTailFuse = 0, kTailCandidates = 1, kTailCandidates2k = 2 };
int launch_tail(anrag_index *idx, hipStream_t st, int set, bool use_dense, bool use_bm25, int32_t k, TailMode mode,
                double w_dense, double w_bm25, double wrrf_k, int32_t top_n, anrag_candidate *d_out,
                int32_t *d_count);
// ... for the n <= kScanGroupMax queries of a group in ONE launch (a workgroup per query)
int launch_tail_group(anrag_index *idx, hipStream_t st, const int *sets, bool use_dense, const bool *use_bm25, int32_t n,
                      int32_t k, TailMode mode, double w_dense, double w_bm25, double wrrf_k, int32_t top_n,
                      anrag_candidate *const *d_out, int32_t *const *d_count);
// ... with the dense group merging the fp64 lists of K1D (set 0 for both legs)
int launch_tail_f64(anrag_index *idx, hipStream_t st, bool use_dense, bool use_bm25, int32_t k, TailMode mode, double w_dense,
                    double w_bm25, double wrrf_k, int32_t top_n, anrag_candidate *d_out, int32_t *d_count);
// K1 + tail on one stream (set 0)
int launch_dense_topk(anrag_index *idx, hipStream_t stream, const float *d_query, int32_t k,
                      const uint32_t *d_allow_bits, anrag_candidate *d_out, float *d_scores_out);
// fp64 query: every row's fp64 dot product (dense_scan.hip); selection by dense_search_f64 (sort_select.hip)
int launch_dense_scores_f64(anrag_index *idx, hipStream_t st, const double *d_query, const uint32_t *d_allow_bits,
                            double *d_scores_out);
int dense_search_f64(anrag_index *idx, hipStream_t st, const double *h_query, int32_t k, const uint32_t *d_allow_bits,
                     int64_t *out_doc, double *out_score, int32_t *out_count);
// K1D, the list-keeping scan of one fp64 query (dense_scan_f64.hip): dim % 4 == 0 up to 3,072, k <= 64.  One sorted fp64
// list per wave into the fp64 list set, rows into set 0 of d_blk_row_a; launch_tail_f64 merges them (with the BM25
// lists of set 0).
bool dense_scan_f64_serves(const anrag_index *idx);
int ensure_dense_f64_lists(anrag_index *idx);  // allocated by the first such query (counted), freed with the dense buffers
void free_dense_f64_lists(anrag_index *idx);
int32_t *dense_f64_count(const anrag_index *idx);  // a device int32 behind the lists: the fused call's count
int ensure_query_f64(anrag_index *idx);
int launch_dense_scan_f64(anrag_index *idx, hipStream_t st, const double *d_query, int32_t k, const uint32_t *d_allow_bits);
// K1FD, the shadow prefilter for one fp64 query (dense_prefilter_f64.hip): behind launch_dense_prefilter_scan and
// launch_dense_prefilter_threshold on list set 0 with fl32(query), the survivors (hi >= T - 2w) rescored with K1D's
// arithmetic into K1D's lists.  ensure_...: Emax of the corpus (idx->f64_pf_emax), once per dense load, syncs `st`.
int ensure_dense_prefilter_f64(anrag_index *idx, hipStream_t st);
int launch_dense_prefilter_rescore_f64(anrag_index *idx, hipStream_t st, const double *d_query, double w, int32_t k);
int dense_prefilter_f64_survivors(anrag_index *idx, int64_t *out);  // cumulative rows rescored since Emax was computed
// K2: up to 256 queries per pass on the fp32 matrix cores (dense_batched.hip)
bool batched_path_applies(const anrag_index *idx, int32_t n_queries, int32_t k);
int launch_dense_batched(anrag_index *idx, hipStream_t st, const float *d_queries, int32_t nq, int32_t k,
                         const uint32_t *d_allow_bits, anrag_candidate *d_out, int32_t *d_flag);
int reserve_dense_batched(anrag_index *idx, hipStream_t st, int32_t nq, int32_t k);  // its workspace, ahead of the pass
void free_batched(anrag_index *idx);
// k > ANRAG_FUSED_K_MAX: score array + radix sort (select.hip); host operands, syncs.
int dense_search_large_k(anrag_index *idx, hipStream_t stream, const float *h_queries, int32_t n_queries, int32_t k,
                         const uint32_t *d_allow_bits, int64_t *out_doc, float *out_score, int32_t *out_count);
void free_bm25(anrag_index *idx);
int bm25_load(anrag_index *idx, const int64_t *indptr, int64_t n_terms, const int32_t *post_doc,
              const int32_t *post_tf, const double *idf, const int32_t *doc_len, int64_t n_docs, double avgdl,
              double k1, double b, const uint16_t *source_id, const int64_t *doc_id, int64_t doc_id_base);
// d_out: k candidates (fused path, k <= 64) -- or d_scores_out: all n_docs scores; exactly one non-null
int launch_bm25(anrag_index *idx, hipStream_t stream, const int32_t *d_terms, int32_t n_terms, int32_t k,
                const uint32_t *d_allow_bits, anrag_candidate *d_out, double *d_scores_out);
int bm25_search_large_k(anrag_index *idx, hipStream_t stream, const int32_t *d_terms, int32_t n_terms, int32_t k,
                        const uint32_t *d_allow_bits, int64_t *out_doc, double *out_score, int32_t *out_count);
// WRRF over `n_lists` id lists laid out back to back in d_ids or d_cands (list l = [h_off[l], h_off[l+1])); entries
// with id < 0 are padding.  Writes min(top_n, distinct) records to d_out and the count to *d_count.
int ensure_wrrf_scratch(anrag_index *idx, int64_t n_entries);
void free_wrrf_scratch(anrag_index *idx);
int wrrf_sorted(anrag_index *idx, hipStream_t st, const int64_t *d_ids, const double *d_contrib, int32_t m,
                int32_t top_n, anrag_candidate *d_out, int32_t *d_count);
int launch_wrrf(anrag_index *idx, hipStream_t st, const int64_t *d_ids, const anrag_candidate *d_cands,
                const int32_t *h_off, const double *h_weight, int32_t n_lists, double k, int32_t top_n,
                anrag_candidate *d_out, int32_t *d_count);
int launch_merge_fuse(anrag_index *idx, hipStream_t st, const anrag_candidate *d_lists, int32_t n_lists, int32_t k,
                      int64_t list_stride, double w_dense, double w_bm25, double wrrf_k, int32_t top_n,
                      int32_t n_queries, anrag_candidate *d_out, int32_t *d_count);
int launch_merge_candidates(anrag_index *idx, hipStream_t stream, const anrag_candidate *d_lists,
                            int32_t n_lists, int32_t k, int64_t list_stride, anrag_candidate *d_out);
// One shard's share of a shard group's exchange group (api.hip; shard_group.hip calls them): 2k candidate records per
// query into d_out, complete in the shard's fusion-stream order; and the shard's call pool for staged operands.
struct CandQuery {
    const float *d_query;   // NULL: no dense leg
    const int32_t *d_terms;
    int32_t n_terms;        // 0 beside a dense leg: no BM25 leg
    anrag_candidate *d_out;
};
int enqueue_candidates_2k(anrag_index *idx, const CandQuery *q, int32_t n, int32_t k, const uint32_t *d_allow_dense,
                          const uint32_t *d_allow_bm25);
int reserve_call_pool(anrag_index *idx, int64_t bytes, char **out);

// ---- full ranking (rank_batch.hip): the pieces anrag_rank_batch and anrag_shard_group_rank_batch share: the call plan
// (RankPlan: checks, fusion plan, chunk), a leg's share on one index and its producer (RankLegRun, rank_leg_chunk), the
// per-call uploads (rank_stage_*), and everything behind the legs' lists (RankTail)
int rank_list_cap(bool fp64);  // anrag_rank_caps
// The wide form of the select (rank_batch.hip, "K4 wide") needs scratch of the caller's rank_pool: rank_wide_bytes for
// the launch's segments, asked for where rank_wide_wanted says the current mode would take it.
struct RankWide {
    char *scratch = nullptr;
    int64_t bytes = 0;
    int32_t form = -1;   // -1: by anrag_set_rank_wide; 0 narrow; 1 wide wherever n > the list cap (anrag_debug_rank_select)
    int32_t parts = 0;   // 0: the launcher chooses the slices
};
bool rank_wide_wanted(bool fp64, int32_t n_seg, int32_t n);
bool rank_wide_gate(bool fp64, int32_t n_seg, int32_t n);  // the auto gate alone
int64_t rank_wide_bytes(bool fp64, int32_t n_seg);
// the k best of n scores per segment by (score desc, position asc) -> rows, keys (fp64, nullable), counts: one workgroup
// per segment, or (wide) a segment across the device
int launch_rank_sort(int device, hipStream_t st, int32_t n_seg, const void *keys, bool fp64, int64_t key_stride, int32_t n,
                     int32_t k, const int32_t *seg_k, uint32_t *out_rows, double *out_keys, int64_t out_stride,
                     int32_t *out_count, const RankWide &wide = RankWide());
// a leg's host operands, whichever entry point's leg struct they came in
struct RankLegOps {
    int32_t kind = 0;
    const void *queries = nullptr;  // float, or double for ANRAG_LEG_DENSE_F64: [n_queries][dim]
    const int32_t *term_ids = nullptr;
    const int64_t *term_offsets = nullptr;
    const uint8_t *allow_source = nullptr;
    int32_t n_sources = 0;
    const int64_t *doc_of_row = nullptr;
    double weight = 0;
};
template <class Leg>
inline RankLegOps rank_leg_ops(const Leg &g) {
    return RankLegOps{g.kind, g.queries, g.term_ids, g.term_offsets, g.allow_source, g.n_sources, g.doc_of_row, g.weight};
}
// The plan of a call, in the order the steps run: rank_plan_call, rank_plan_kind per leg (before any lock),
// rank_plan_leg per leg on its GLOBAL rows, rank_plan_fusion; the caller adds what its legs take per query of a chunk
// (`per_query`) and per call (`fixed`); rank_plan_chunk.
struct RankPlan {
    int32_t n_legs = 0, n_queries = 0, similarity_k = 0, top_n = 0;
    double wrrf_k = 0;
    int64_t id_space = 0;
    int64_t leg_rows[ANRAG_WRRF_MAX_LISTS] = {};
    int32_t leg_k[ANRAG_WRRF_MAX_LISTS] = {};  // min(similarity_k, rows)
    bool fuse = false, fuse_in_lds = false;    // in LDS: rank_fuse_sort_kernel does the whole fusion
    int32_t fuse_n = 0, out_n = 0;             // entries the fused order is cut to; entries a query returns
    int64_t per_query = 0, fixed = 0;          // bytes of scratch
    int64_t chunk = 0, max_terms_chunk = 0;    // queries per chunk; the most term ids a chunk of a BM25 leg carries
    int32_t c_full = 0;                        // segments of a full chunk's sort launches
};
int rank_plan_call(RankPlan &p, bool have_legs, int32_t n_legs, int32_t n_queries, int32_t similarity_k, double wrrf_k,
                   int32_t top_n, int64_t id_space, const int64_t *out_id, const double *out_score, const int32_t *out_count,
                   const int64_t *expect_id, const int32_t *out_rank);
int rank_plan_kind(int l, const RankLegOps &g, unsigned kinds);  // `kinds`: bit (1 << kind) per kind the route admits
int rank_plan_index(int l, const RankLegOps &g, const anrag_index *ix);  // a leg on ONE index: loaded, source ids there
int rank_plan_leg(RankPlan &p, int l, const RankLegOps &g, int64_t rows);
// fuse_n, fuse_in_lds, out_n; every map inside [0, id_space) and injective (a NULL map: the leg's rows fit the id space)
int rank_plan_fusion(RankPlan &p, const RankLegOps *legs);
void rank_plan_chunk(RankPlan &p, const RankLegOps *legs);  // 6 GiB of scratch a chunk, or ANRAG_RANK_CHUNK_BUDGET
// One leg's share on one index: all of it (anrag_rank_batch) or a shard's block of rows.  The buffers are device memory
// of ix's device, the staging vectors stay as they are until the chunk's host sync.
struct RankLegRun {
    anrag_index *ix = nullptr;
    hipStream_t st = nullptr;  // every copy and launch of the run
    int32_t kind = 0;
    int64_t rows = 0, stride = 0;
    int32_t k = 0;  // min(similarity_k, rows)
    uint32_t *allow = nullptr;
    void *q = nullptr;  // float, or double for ANRAG_LEG_DENSE_F64
    int32_t *terms = nullptr, *seg_k = nullptr;
    int64_t *term_off = nullptr;
    void *scores = nullptr;
    uint32_t *list_rows = nullptr;
    double *list_keys = nullptr;  // nullable
    int32_t *list_cnt = nullptr;
    RankWide wide;  // the wide select's scratch, where the mode takes it for these rows
    std::vector<int32_t> h_segk;
    std::vector<int64_t> h_off;
    void carve(Carver &cv, const RankPlan &p, bool want_allow, bool want_keys);
};
struct RankTail;
// One chunk (queries q0 .. q0 + c) of a leg on run.ix, whose device is current: operands up, score tiles (K1T / K1TD, a
// pass per query where the dimension has no tile kernel; K3's score table), then the sort into the run's lists -- or,
// with `count`, the rank of count->d_expect in leg 0's order alone (rank_count_kernel; no lists).  Never syncs.
int rank_leg_chunk(RankLegRun &run, const RankLegOps &g, int64_t q0, int32_t c, const RankTail *count);
// per-call uploads on the run's / the given stream, each followed by its host sync
int rank_stage_allow(const RankLegRun &run, const RankLegOps &g);  // no-op without an allow list
int rank_stage_map(hipStream_t st, const int64_t *doc_of_row, int64_t rows, int32_t *d_map);  // int64 -> int32
struct RankTailLeg {
    const uint32_t *rows;       // [chunk][leg_k]
    const double *row_keys;     // one leg only
    const int32_t *cnt;         // [chunk]
    const int32_t *doc_of_row;  // nullable
    int32_t leg_k;
    double weight;
};
// what runs behind the legs' lists on one device and stream; every pointer is device memory of that device
struct RankTail {
    int device = 0;
    hipStream_t st = nullptr;
    int n_legs = 0;
    RankTailLeg leg[ANRAG_WRRF_MAX_LISTS] = {};
    bool fuse_in_lds = false;
    double wrrf_k = 0;
    int64_t id_space = 0;
    int32_t fuse_n = 0, out_n = 0;
    double *d_f = nullptr, *d_skey = nullptr;  // fusion in HBM
    uint32_t *d_t = nullptr, *d_stie = nullptr;
    int32_t *d_scnt = nullptr;
    uint64_t *d_fuse_legs = nullptr;           // fusion in LDS: rank_stage_fuse_table's words
    int64_t *d_out_id = nullptr;
    double *d_out_score = nullptr;
    int32_t *d_out_cnt = nullptr;
    int64_t *d_expect = nullptr;
    int32_t *d_rank = nullptr;
    RankWide wide;                             // for the fused-sums select (fusion in HBM)
    void carve(Carver &cv, const RankPlan &p, bool want_expect);  // the plan's figures and every buffer above; not leg[]
};
int rank_stage_fuse_table(const RankTail &t);  // fusion in LDS: the table of the filled leg[] up, and its host sync
int rank_stage_expect(const RankTail &t, const int64_t *expect_id, int64_t q0, int32_t c);  // a chunk's; no sync
int launch_rank_tail(const RankTail &t, int32_t c, bool want_ids);
int rank_copy_out(const RankTail &t, int32_t c, int64_t q0, int32_t top_n, int64_t *out_id, double *out_score,
                  int32_t *out_count, int32_t *out_rank);

// ---- a shard group as the ranked route sees it (shard_group.hip owns the struct)
struct GroupView {
    std::mutex *mu;
    int32_t n;
    anrag_index *const *shard;
    const int *device;
    const int64_t *dense_lo, *bm25_lo;  // n + 1 block bounds
    bool has_dense, has_bm25, has_dense_src, has_bm25_src;
};
GroupView shard_group_view(anrag_shard_group *g);

}  // namespace anrag
