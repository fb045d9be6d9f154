// Shard group: one corpus over several anrag_index objects in ONE process (include/anrag.h, "shard group").
//
// Per exchange group of up to 8 queries every shard enqueues its 2k candidate records per query into a slab of its own
// HBM (the three-stream pipeline, complete in the shard's fusion-stream order) and records an event there; the home
// shard (shard 0) makes its fusion stream wait for those events and launches ONE group_tail_kernel, which reads the
// slabs in place.  Nothing syncs the host between the shards' work and the tail, and no collective runs.
//
// Why the merge is in SHARD ORDER and not by doc id (select.hip's merge_fuse_kernel): shards are contiguous row blocks
// in ascending order and a shard's list is already (score desc, row asc), so "on equal scores the earlier shard, inside
// a shard the earlier position, stays ahead" IS (score desc, global row asc), the single index's rule, whatever the doc
// id map.  The drop-in layer maps BM25 sections to the dense row of their chunk id -- an arbitrary permutation -- and
// equal BM25 scores (zeros) are common, so a doc-id tie-break would return other ids than the single index.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "common.hpp"
#include "wave_topk.hpp"
#include "wrrf_block.hpp"

namespace anrag {

constexpr int kGroupDepth = 4;      // exchange groups in flight: kPipeSlots / kGroupQueries
constexpr int kGroupQueries = 8;    // queries per exchange group (one scan launch per shard)
constexpr int kGroupChunk = 1024;   // queries per host sync of a batch call
constexpr int kGroupTermsMax = 4096;
constexpr int64_t kSlabRecords = (int64_t)kGroupDepth * kGroupQueries * 2 * kListLen;
static_assert(kGroupDepth * kGroupQueries <= kPipeSlots, "a shard's pipeline holds every group in flight");

enum GroupTailMode { kGroupFuse = 0, kGroupDense = 1, kGroupBm25 = 2 };

// Register top-k over (fp64 score, int64 doc) that is STABLE in insertion order: a newcomer displaces a held entry only
// when its score is strictly greater.  An empty slot is doc -1 and loses to everything real.
struct ShardOrderTopK {
    double s;
    long long d;
    double thr_s;
    long long thr_d;
    int k;
    __device__ __forceinline__ void init(int k_) {
        s = -__builtin_huge_val();
        d = -1;
        thr_s = s;
        thr_d = -1;
        k = k_;
    }
    __device__ __forceinline__ bool admits(double cs, long long cd) const {
        if (cd < 0) return false;
        return thr_d < 0 || cs > thr_s;
    }
    __device__ __forceinline__ void insert(double cs, long long cd) {
        const int lane = threadIdx.x & 63;
        const bool ahead = d >= 0 && s >= cs;  // a held entry stays ahead of an equal score: earlier shard / position
        const double up_s = lane_up1(s);
        const long long up_d = __double_as_longlong(lane_up1(__longlong_as_double(d)));  // bits only
        const uint32_t up_ahead = lane_up1((uint32_t)ahead);
        if (!ahead) {
            const bool first = (lane == 0) || up_ahead;
            s = first ? cs : up_s;
            d = first ? cd : up_d;
        }
        thr_s = read_lane(s, k - 1);
        thr_d = __double_as_longlong(read_lane(__longlong_as_double(d), k - 1));
    }
};

struct GroupTailArgs {
    const anrag_candidate *slab[ANRAG_GROUP_MAX_SHARDS];  // shard l: [n_queries][2k] records, [0,k) dense, [k,2k) BM25
    int32_t n_shards, k, mode, top_n;
    double w_dense, w_bm25, wrrf_k;
    anrag_candidate *out;  // [n_queries][out_stride]
    int32_t *count;        // [n_queries]
    int64_t out_stride;
};

__device__ __forceinline__ anrag_candidate load_record(const anrag_candidate *p, bool on) {
    anrag_candidate c;
    c.score = -__builtin_huge_val();
    c.doc = -1;
    if (on) c = *p;
    if (c.score != c.score) c.score = __builtin_huge_val();  // NaN ranks first, reported as +inf
    return c;
}

// The group's tail, ONE launch: a workgroup per query; wave 0 merges the shards' dense lists, wave 1 their BM25 lists,
// stably in shard order; then weighted RRF + top-n on the global ranks (kGroupFuse) or the merged k records of the one
// active leg with their leg scores.  The slab pointers arrive by value: no table upload.
__global__ __launch_bounds__(128) void group_tail_kernel(GroupTailArgs a) {
    __shared__ int64_t s_id[2 * kListLen];
    __shared__ double s_c[2 * kListLen];
    __shared__ double s_score[2 * kListLen];
    __shared__ int32_t s_owner[2 * kListLen];
    __shared__ int32_t s_distinct;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = a.k;
    const int64_t at = (int64_t)blockIdx.x * 2 * k + wave * k + lane;
    anrag_candidate *out = a.out + (int64_t)blockIdx.x * a.out_stride;
    int32_t *count = a.count + blockIdx.x;
    const bool mine = a.mode == kGroupFuse || a.mode == (wave ? kGroupBm25 : kGroupDense);
    ShardOrderTopK top;
    top.init(k);
    if (mine) {
        anrag_candidate next = load_record(a.slab[0] + at, lane < k);
        for (int li = 0; li < a.n_shards; ++li) {
            const anrag_candidate c = next;
            // the following shard's record is on its way (over the fabric) while this one's list is walked
            if (li + 1 < a.n_shards) next = load_record(a.slab[li + 1] + at, lane < k);
            for (int i = 0; i < k; ++i) {
                const double cs = read_lane(c.score, i);
                const long long cd = __double_as_longlong(read_lane(__longlong_as_double((long long)c.doc), i));
                if (!top.admits(cs, cd)) break;  // the list is sorted: nothing behind its first loser gets in
                top.insert(cs, cd);
            }
        }
    }
    if (a.mode != kGroupFuse) {
        if (mine) {
            if (lane < k) {
                anrag_candidate c;
                c.score = top.d < 0 ? -__builtin_huge_val() : top.s;
                c.doc = top.d;
                out[lane] = c;
            }
            const unsigned long long real = __ballot(lane < k && top.d >= 0);
            if (lane == 0) *count = __builtin_popcountll(real);
        }
        return;
    }
    if (lane < k) {
        const int slot = wave * k + lane;
        const double w = wave ? a.w_bm25 : a.w_dense;
        s_id[slot] = top.d;
        s_c[slot] = top.d < 0 ? 0.0 : w * (1.0 / (a.wrrf_k + (double)(lane + 1)));
    }
    __syncthreads();
    wrrf_in_block(s_id, s_c, s_score, s_owner, &s_distinct, 2 * k, a.top_n, out, count);
}

// ---- dense query LISTS: every shard runs the single index's K2 pass (dense_batched.hip) over its rows, the home device
// merges the shards' k records per query.  A K2 score is the accumulator of one (corpus row, query) element: its k-steps
// and the order inside them do not depend on the row's tile, on its place in the tile or on the 128 / 256-query geometry,
// so a row scores the same bits in its shard as in the whole corpus, and the merged answer is the single index's.
constexpr int kBatchedQueries = 256;  // queries per chunk: one K2 pass per shard
constexpr int kBatchedBlocks = 2;     // result blocks per shard: the next chunk's pass runs under this chunk's merge

struct BatchedMergeArgs {
    const anrag_candidate *list[ANRAG_GROUP_MAX_SHARDS];  // shard s: [n_queries][k], (score desc, row asc), empty (doc -1) last
    const int32_t *flag[ANRAG_GROUP_MAX_SHARDS];          // shard s: [n_queries], nonzero = its survivor list overflowed
    int32_t n_shards, k;
    anrag_candidate *out;  // [n_queries][k]
    int32_t *count;        // [n_queries]
    int32_t *out_flag;     // [n_queries]: the OR of the shards' flags
};

// order-preserving bits of a score, as the list kernels compare them (shard_group_rank.hip): -0.0 == +0.0
__device__ __forceinline__ uint64_t score_order_bits(double v) {
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if ((b << 1) == 0) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// A wave per query: lane p owns entry p of every shard's list.  The keys of all S lists go to LDS; entry p of shard s
// then lands at  p + sum over t < s of #{keys of t >= mine} + sum over t > s of #{keys of t > mine}  -- a later shard's
// candidate gets ahead of an earlier shard's only on a strictly greater score: (score desc, global row asc).  Each term is
// a binary search over a sorted list; the ranks of the real entries are a permutation, so every output slot has one
// writer (the slots past the last real entry: the lanes of that number) and nothing is atomic.
__global__ __launch_bounds__(kWave) void group_batched_merge_kernel(BatchedMergeArgs a) {
    __shared__ uint64_t s_key[ANRAG_GROUP_MAX_SHARDS * kListLen];
    __shared__ int32_t s_n[ANRAG_GROUP_MAX_SHARDS];
    const int lane = threadIdx.x, k = a.k;
    const int64_t q = blockIdx.x, at = q * k + lane;
    int32_t total = 0, flagged = 0;
    for (int s = 0; s < a.n_shards; ++s) {
        const anrag_candidate c = load_record(a.list[s] + at, lane < k);
        s_key[s * kListLen + lane] = score_order_bits(c.score);
        const int32_t n = __builtin_popcountll(__ballot(c.doc >= 0));  // empty entries are the list's tail
        if (lane == 0) s_n[s] = n;
        total += n;
        flagged |= a.flag[s][q];
    }
    __syncthreads();
    anrag_candidate *out = a.out + q * k;
    for (int s = 0; s < a.n_shards; ++s) {
        if (lane >= s_n[s]) continue;
        const uint64_t x = s_key[s * kListLen + lane];
        int32_t r = lane;
        for (int t = 0; t < a.n_shards && r < k; ++t) {
            if (t == s) continue;
            // entries of t ahead of mine; more than k - r of them put mine outside the answer, so the search stops there
            const int32_t n_t = s_n[t], room = k - r;
            int32_t lo = 0, hi = n_t < room ? n_t : room;
            const uint64_t *kt = s_key + t * kListLen;
            const bool strict = t > s;  // a later shard stays behind an equal score
            while (lo < hi) {
                const int32_t mid = (lo + hi) >> 1;
                const uint64_t u = kt[mid];
                if (strict ? u > x : u >= x) lo = mid + 1;
                else hi = mid;
            }
            r += lo;
        }
        if (r < k) out[r] = load_record(a.list[s] + at, true);
    }
    if (lane < k && lane >= total) {
        anrag_candidate c;
        c.score = -__builtin_huge_val();
        c.doc = -1;
        out[lane] = c;
    }
    if (lane == 0) {
        a.count[q] = total < k ? total : k;
        a.out_flag[q] = flagged ? -1 : 0;
    }
}

}  // namespace anrag

using namespace anrag;

struct anrag_shard_group {
    std::mutex mu;
    int32_t n = 0;
    anrag_index *shard[ANRAG_GROUP_MAX_SHARDS] = {};
    int device[ANRAG_GROUP_MAX_SHARDS] = {};
    bool in_place[ANRAG_GROUP_MAX_SHARDS] = {};  // the home device reads shard i's slab where it is
    int64_t dense_lo[ANRAG_GROUP_MAX_SHARDS + 1] = {};
    int64_t bm25_lo[ANRAG_GROUP_MAX_SHARDS + 1] = {};
    int32_t dim = 0;
    bool has_dense = false, has_bm25 = false, has_dense_src = false, has_bm25_src = false;
    // per shard, in its own HBM: the slab and the allow bitmaps; for a shard the home device cannot map, a copy of its slab
    // on the home device
    char *d_block[ANRAG_GROUP_MAX_SHARDS] = {};
    anrag_candidate *d_slab[ANRAG_GROUP_MAX_SHARDS] = {};
    anrag_candidate *d_stage[ANRAG_GROUP_MAX_SHARDS] = {};
    uint32_t *d_allow_a[ANRAG_GROUP_MAX_SHARDS] = {}, *d_allow_b[ANRAG_GROUP_MAX_SHARDS] = {};
    hipEvent_t ev_cand[ANRAG_GROUP_MAX_SHARDS][kGroupDepth] = {};  // shard i's records of the slot are in its slab
    hipEvent_t ev_tail[kGroupDepth] = {};                          // the home tail has read the slot
    uint64_t seq = 0;                                              // exchange groups so far
    int64_t enqueue_ns = 0;  // host time spent enqueuing them (every shard's launches, the waits, the tail launch)
    // pinned: allow bitmaps | one query's terms | a chunk's result records and counts; the single query's vector
    char *h_pin = nullptr;
    float *h_query = nullptr;
    int64_t own_bytes = 0;
    // the batched dense route (run_batched): the result blocks live in the shards' call pools; here the events, the copy
    // of an unmappable shard's blocks on the home device, the pinned query chunks, the counters
    bool batched_on = true;                                                  // ANRAG_GROUP_BATCHED, read at create
    hipEvent_t ev_pass[ANRAG_GROUP_MAX_SHARDS][kBatchedBlocks] = {};         // shard i's pass has filled the block
    hipEvent_t ev_merged[kBatchedBlocks] = {};                               // the home stream has read the block
    char *d_bstage[ANRAG_GROUP_MAX_SHARDS] = {};
    float *h_bq = nullptr;                                                   // [kBatchedBlocks][kBatchedQueries][dim]
    int64_t b_passes = 0, b_queries = 0, b_redone = 0;
};

anrag::GroupView anrag::shard_group_view(anrag_shard_group *g) {
    return GroupView{&g->mu, g->n, g->shard, g->device, g->dense_lo, g->bm25_lo,
                     g->has_dense, g->has_bm25, g->has_dense_src, g->has_bm25_src};
}

namespace {

constexpr size_t kPinTerms = 2 * kAllowWords * sizeof(uint32_t);  // behind the two allow bitmaps
constexpr size_t kPinOut = kPinTerms + kGroupTermsMax * sizeof(int32_t);
constexpr size_t kPinCount = kPinOut + (size_t)kGroupChunk * 2 * kListLen * sizeof(anrag_candidate);
constexpr size_t kPinBytes = kPinCount + (size_t)kGroupChunk * sizeof(int32_t);
// the batched dense route's chunks come back through the hot route's result region: per block k records, a count and a
// flag per query (the two routes never run at the same time)
constexpr size_t kPinBlock = (size_t)kBatchedQueries * (kListLen * sizeof(anrag_candidate) + 2 * sizeof(int32_t));
static_assert(kPinOut + kBatchedBlocks * kPinBlock <= kPinBytes, "the batched route's blocks fit the pinned result region");
// an unmappable shard's block on the home device: records at 0, flags behind them (sized for k = kListLen)
constexpr size_t kStageFlags = (size_t)kBatchedQueries * kListLen * sizeof(anrag_candidate);
constexpr size_t kStageBlock = kStageFlags + kBatchedQueries * sizeof(int32_t);

void shard_bounds(int64_t n, int32_t S, int64_t *lo) {
    const int64_t base = n / S, extra = n % S;
    for (int32_t i = 0; i <= S; ++i) lo[i] = (int64_t)i * base + std::min<int64_t>(i, extra);
}

int drain(anrag_shard_group *g) {
    int rc = ANRAG_OK;
    for (int32_t i = 0; i < g->n; ++i)
        if (g->shard[i])
            if (int r = anrag_index_sync(g->shard[i])) rc = r;
    return rc;
}

void destroy(anrag_shard_group *g) {
    (void)drain(g);
    for (int32_t i = 0; i < g->n; ++i) {
        DeviceGuard guard(g->device[i]);
        for (hipEvent_t e : g->ev_cand[i])
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : g->ev_pass[i])
            if (e) (void)hipEventDestroy(e);
        if (g->d_block[i]) (void)counted_free(g->d_block[i]);
    }
    {
        DeviceGuard guard(g->device[0]);
        for (hipEvent_t e : g->ev_tail)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : g->ev_merged)
            if (e) (void)hipEventDestroy(e);
        for (int32_t i = 0; i < g->n; ++i) {
            if (g->d_stage[i]) (void)counted_free(g->d_stage[i]);
            if (g->d_bstage[i]) (void)counted_free(g->d_bstage[i]);
        }
        if (g->h_pin) (void)counted_host_free(g->h_pin);
        if (g->h_query) (void)counted_host_free(g->h_query);
        if (g->h_bq) (void)counted_host_free(g->h_bq);
    }
    for (int32_t i = 0; i < g->n; ++i)
        if (g->shard[i]) (void)anrag_index_destroy(g->shard[i]);
    delete g;
}

// One call's worth of the hot route.  mode kGroupFuse: the answer of anrag_hybrid_search per query; kGroupDense /
// kGroupBm25: the k records of the one leg.  `queries` NULL = no dense leg; `term_offsets` NULL = no query has terms.
// h_out [n_queries][width] / h_cnt [n_queries]: width = top_n (fuse) or k.
struct HotCall {
    int32_t mode;
    const float *queries;
    const int32_t *term_ids;
    const int64_t *term_offsets;
    int32_t n_queries, k;
    double w_dense, w_bm25, wrrf_k;
    int32_t top_n;
    const uint8_t *allow_dense;
    int32_t n_dense_sources;
    const uint8_t *allow_bm25;
    int32_t n_bm25_sources;
};

int run_chunk(anrag_shard_group *g, const HotCall &c, int32_t q0, int32_t nq, bool dense_leg, anrag_candidate *h_out,
              int32_t *h_cnt) {
    const int32_t width = c.mode == kGroupFuse ? c.top_n : c.k;
    const int64_t t0 = c.term_offsets ? c.term_offsets[q0] : 0;
    const int64_t n_terms = c.term_offsets ? c.term_offsets[q0 + nq] - t0 : 0;
    const float *src_q = dense_leg ? c.queries + (int64_t)q0 * g->dim : nullptr;
    const int32_t *src_t = n_terms > 0 ? c.term_ids + t0 : nullptr;
    if (nq == 1) {  // the single query goes up from pinned staging: the copies below return at once
        if (dense_leg) {
            memcpy(g->h_query, src_q, (size_t)g->dim * sizeof(float));
            src_q = g->h_query;
        }
        if (n_terms > 0) {
            memcpy(g->h_pin + kPinTerms, src_t, (size_t)n_terms * sizeof(int32_t));
            src_t = reinterpret_cast<const int32_t *>(g->h_pin + kPinTerms);
        }
    }
    const uint32_t *h_aa = reinterpret_cast<const uint32_t *>(g->h_pin);
    const uint32_t *h_ab = h_aa + kAllowWords;
    float *d_q[ANRAG_GROUP_MAX_SHARDS] = {};
    int32_t *d_t[ANRAG_GROUP_MAX_SHARDS] = {};
    anrag_candidate *d_out = nullptr;
    int32_t *d_cnt = nullptr;
    int rc;
    for (int32_t i = 0; i < g->n; ++i) {  // operands up: the query vectors on the scan's stream, the rest on K3's
        rc = carve_block([&](int64_t bytes, char **pool) { return reserve_call_pool(g->shard[i], bytes + 256, pool); },
                         [&](Carver &cv) {
                             d_q[i] = dense_leg ? cv.take<float>((int64_t)nq * g->dim) : nullptr;
                             d_t[i] = n_terms > 0 ? cv.take<int32_t>(n_terms) : nullptr;
                             if (i == 0) {
                                 d_out = cv.take<anrag_candidate>((int64_t)nq * width);
                                 d_cnt = cv.take<int32_t>(nq);
                             }
                         });
        if (rc) return rc;
        DeviceGuard guard(g->device[i]);
        anrag_index *sh = g->shard[i];
        if (dense_leg)
            ANRAG_HIP(hipMemcpyAsync(d_q[i], src_q, (size_t)nq * g->dim * sizeof(float), hipMemcpyHostToDevice, sh->primary));
        if (c.allow_dense)
            ANRAG_HIP(hipMemcpyAsync(g->d_allow_a[i], h_aa, kAllowWords * sizeof(uint32_t), hipMemcpyHostToDevice, sh->primary));
        if (n_terms > 0)
            ANRAG_HIP(hipMemcpyAsync(d_t[i], src_t, (size_t)n_terms * sizeof(int32_t), hipMemcpyHostToDevice, sh->secondary));
        if (c.allow_bm25)
            ANRAG_HIP(hipMemcpyAsync(g->d_allow_b[i], h_ab, kAllowWords * sizeof(uint32_t), hipMemcpyHostToDevice, sh->secondary));
    }
    hipStream_t home = g->shard[0]->fusion;
    for (int32_t e0 = 0; e0 < nq; e0 += kGroupQueries) {
        const int n = std::min<int32_t>(kGroupQueries, nq - e0);
        const int slot = (int)(g->seq % kGroupDepth);
        const auto t_enqueue = std::chrono::steady_clock::now();
        const int64_t slot_at = (int64_t)slot * kGroupQueries * 2 * kListLen;  // a slot is sized for k = kListLen
        for (int32_t i = 0; i < g->n; ++i) {
            DeviceGuard guard(g->device[i]);
            anrag_index *sh = g->shard[i];
            // the slot's previous records must have been read: a device-side wait (the home shard's own stream orders it)
            if (i > 0 && g->seq >= (uint64_t)kGroupDepth) ANRAG_HIP(hipStreamWaitEvent(sh->fusion, g->ev_tail[slot], 0));
            CandQuery cq[kGroupQueries];
            for (int j = 0; j < n; ++j) {
                const int32_t q = q0 + e0 + j;
                const int64_t off = c.term_offsets ? c.term_offsets[q] - t0 : 0;
                int32_t nt = c.term_offsets ? (int32_t)(c.term_offsets[q + 1] - c.term_offsets[q]) : 0;
                if (c.mode == kGroupFuse && !(c.w_bm25 > 0.0)) nt = 0;
                cq[j].d_query = dense_leg ? d_q[i] + (int64_t)(e0 + j) * g->dim : nullptr;
                cq[j].d_terms = nt > 0 ? d_t[i] + off : nullptr;
                cq[j].n_terms = g->has_bm25 ? nt : 0;
                cq[j].d_out = g->d_slab[i] + slot_at + (int64_t)j * 2 * c.k;
            }
            if ((rc = enqueue_candidates_2k(sh, cq, n, c.k, c.allow_dense ? g->d_allow_a[i] : nullptr,
                                            c.allow_bm25 ? g->d_allow_b[i] : nullptr)))
                return rc;
            if (i > 0) ANRAG_HIP(hipEventRecord(g->ev_cand[i][slot], sh->fusion));
        }
        DeviceGuard guard(g->device[0]);
        GroupTailArgs a;
        for (int32_t i = 0; i < ANRAG_GROUP_MAX_SHARDS; ++i) a.slab[i] = g->d_slab[0] + slot_at;
        for (int32_t i = 1; i < g->n; ++i) {
            ANRAG_HIP(hipStreamWaitEvent(home, g->ev_cand[i][slot], 0));
            if (g->in_place[i]) {
                a.slab[i] = g->d_slab[i] + slot_at;
            } else {
                ANRAG_HIP(hipMemcpyPeerAsync(g->d_stage[i] + slot_at, g->device[0], g->d_slab[i] + slot_at, g->device[i],
                                             (size_t)n * 2 * c.k * sizeof(anrag_candidate), home));
                a.slab[i] = g->d_stage[i] + slot_at;
            }
        }
        a.n_shards = g->n;
        a.k = c.k;
        a.mode = c.mode;
        a.top_n = c.top_n;
        a.w_dense = c.w_dense;
        a.w_bm25 = c.w_bm25;
        a.wrrf_k = c.wrrf_k;
        a.out = d_out + (int64_t)e0 * width;
        a.count = d_cnt + e0;
        a.out_stride = width;
        {   // under the home shard's own lock: its profiling state is also reached through the borrowed handle
            std::lock_guard<std::mutex> home_lock(g->shard[0]->mu);
            LaunchTimer t(g->shard[0], c.mode == kGroupFuse ? ANRAG_KERNEL_WRRF : ANRAG_KERNEL_SELECT, home, n);
            group_tail_kernel<<<n, 128, 0, home>>>(a);
            ANRAG_HIP(hipGetLastError());
        }
        ANRAG_HIP(hipEventRecord(g->ev_tail[slot], home));
        g->seq += 1;
        g->enqueue_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_enqueue).count();
    }
    DeviceGuard guard(g->device[0]);
    anrag_candidate *p_out = reinterpret_cast<anrag_candidate *>(g->h_pin + kPinOut);
    int32_t *p_cnt = reinterpret_cast<int32_t *>(g->h_pin + kPinCount);
    ANRAG_HIP(hipMemcpyAsync(p_out, d_out, (size_t)nq * width * sizeof(anrag_candidate), hipMemcpyDeviceToHost, home));
    ANRAG_HIP(hipMemcpyAsync(p_cnt, d_cnt, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, home));
    ANRAG_HIP(hipStreamSynchronize(home));  // everything of the chunk, on every shard, precedes this point of the home stream
    memcpy(h_out, p_out, (size_t)nq * width * sizeof(anrag_candidate));
    memcpy(h_cnt, p_cnt, (size_t)nq * sizeof(int32_t));
    return ANRAG_OK;
}

int run_hot(anrag_shard_group *g, const HotCall &c, std::vector<anrag_candidate> &h_out, std::vector<int32_t> &h_cnt) {
    ANRAG_REQUIRE(c.n_queries >= 1 && c.n_queries <= (1 << 20), "n_queries %d out of range", c.n_queries);
    ANRAG_REQUIRE(c.k > 0 && c.k <= ANRAG_FUSED_K_MAX, "the fused route serves 1 <= k <= %d", ANRAG_FUSED_K_MAX);
    ANRAG_REQUIRE(!(c.allow_dense && !g->has_dense_src) && !(c.allow_bm25 && !g->has_bm25_src),
                  "a source filter needs source ids");
    // which legs a query has: the single index's rule, decided here once for all shards
    const bool dense_leg = c.mode == kGroupDense || (c.mode == kGroupFuse && g->has_dense && c.w_dense > 0.0);
    ANRAG_REQUIRE(!dense_leg || c.queries != nullptr, "queries is NULL");
    if (c.term_offsets) {
        ANRAG_REQUIRE(c.term_offsets[0] == 0 && (c.term_offsets[c.n_queries] == 0 || c.term_ids), "bad term offsets");
        for (int32_t q = 0; q < c.n_queries; ++q) {
            const int64_t nt = c.term_offsets[q + 1] - c.term_offsets[q];
            ANRAG_REQUIRE(nt >= 0 && nt <= kGroupTermsMax, "query %d: term count out of range [0, %d]", q, kGroupTermsMax);
            ANRAG_REQUIRE(c.mode != kGroupFuse || dense_leg || (g->has_bm25 && c.w_bm25 > 0.0 && nt > 0),
                          "hybrid search with neither a dense nor a BM25 leg");
        }
    } else {
        ANRAG_REQUIRE(c.mode != kGroupFuse || dense_leg, "hybrid search with neither a dense nor a BM25 leg");
    }
    int rc;
    uint32_t *h_bits = reinterpret_cast<uint32_t *>(g->h_pin);
    if (c.allow_dense && (rc = pack_allow_bits(c.allow_dense, c.n_dense_sources, h_bits))) return rc;
    if (c.allow_bm25 && (rc = pack_allow_bits(c.allow_bm25, c.n_bm25_sources, h_bits + kAllowWords))) return rc;
    const int32_t width = c.mode == kGroupFuse ? c.top_n : c.k;
    h_out.resize((size_t)c.n_queries * width);
    h_cnt.resize(c.n_queries);
    for (int32_t q0 = 0; q0 < c.n_queries; q0 += kGroupChunk) {
        const int32_t nq = std::min<int32_t>(kGroupChunk, c.n_queries - q0);
        if ((rc = run_chunk(g, c, q0, nq, dense_leg, h_out.data() + (size_t)q0 * width, h_cnt.data() + q0))) {
            (void)drain(g);  // nothing may still read the staged operands when the next call carves them again
            return rc;
        }
    }
    return ANRAG_OK;
}

// The batched dense route: a list of queries through K2 on every shard (the caller has checked the single index's gate on
// each of them).  Per chunk of up to 256 queries: the queries go up from pinned staging on every shard's primary stream,
// launch_dense_batched follows on that stream into result block (chunk & 1) of the shard's call pool, an event marks the
// block full; the home stream -- shard 0's primary -- waits for the events, merges (group_batched_merge_kernel; one shard:
// its block IS the answer) and copies the chunk to pinned memory.  The host enqueues chunk c + 1 before it waits for
// chunk c.  A pass that fills a block again waits, on the device, for the event behind the home stream's last read of it
// (with two blocks the host's own wait for chunk c already precedes the enqueue of chunk c + 2; the device wait keeps the
// rule local to the block).  `redo`: the queries a shard flagged (its survivor list overflowed) -- the caller answers
// them through the hot route once nothing of this one is in flight.
int run_batched(anrag_shard_group *g, const float *queries, int32_t n_queries, int32_t k, const uint8_t *allow_source,
                int32_t n_sources, int64_t *out_doc, float *out_score, int32_t *out_count, std::vector<int32_t> &redo) {
    const int32_t S = g->n, dim = g->dim;
    int rc;
    if (allow_source && (rc = pack_allow_bits(allow_source, n_sources, reinterpret_cast<uint32_t *>(g->h_pin)))) return rc;
    // the shards' own locks, in address order (shard_group_rank.hip): their workspaces and profiling state are also
    // reached through the borrowed handles
    std::vector<anrag_index *> owners(g->shard, g->shard + S);
    std::sort(owners.begin(), owners.end());
    std::vector<std::unique_lock<std::mutex>> locks;
    for (anrag_index *o : owners) locks.emplace_back(o->mu);

    float *d_q[ANRAG_GROUP_MAX_SHARDS] = {};
    anrag_candidate *d_rec[ANRAG_GROUP_MAX_SHARDS][kBatchedBlocks] = {};
    int32_t *d_flag[ANRAG_GROUP_MAX_SHARDS][kBatchedBlocks] = {};
    anrag_candidate *d_out = nullptr;
    int32_t *d_cnt = nullptr, *d_oflag = nullptr;
    const int32_t n_chunks = (n_queries + kBatchedQueries - 1) / kBatchedQueries;
    const int32_t tail_nq = n_queries - (n_chunks - 1) * kBatchedQueries;  // the last chunk's queries
    auto setup = [&](int32_t i) -> int {
        anrag_index *sh = g->shard[i];
        DeviceGuard guard(g->device[i]);
        if (!guard.ok) {
            set_error("hipSetDevice(%d) failed", g->device[i]);
            return ANRAG_ERR_HIP;
        }
        if ((rc = settle_pipeline(sh))) return rc;
        rc = carve_pool(sh, sh->call_pool, 256, [&](Carver &cv) {  // grow-only; nothing of the shard's is in flight
            d_q[i] = cv.take<float>((int64_t)kBatchedQueries * dim);
            for (int b = 0; b < kBatchedBlocks; ++b) {
                d_rec[i][b] = cv.take<anrag_candidate>((int64_t)kBatchedQueries * k);
                d_flag[i][b] = cv.take<int32_t>(kBatchedQueries);
            }
            if (i == 0 && S > 1) {
                d_out = cv.take<anrag_candidate>((int64_t)kBatchedQueries * k);
                d_cnt = cv.take<int32_t>(kBatchedQueries);
                d_oflag = cv.take<int32_t>(kBatchedQueries);
            }
        });
        if (rc) return rc;
        // K2's workspace for both pass sizes of the call (the sample grows when a pass has 128 queries or fewer): sized
        // here, where nothing is in flight, so that no pass replaces it under the one before
        if (n_chunks > 1 && (rc = reserve_dense_batched(sh, sh->primary, kBatchedQueries, k))) return rc;
        if ((rc = reserve_dense_batched(sh, sh->primary, tail_nq, k))) return rc;
        if (allow_source)
            ANRAG_HIP(hipMemcpyAsync(g->d_allow_a[i], g->h_pin, kAllowWords * sizeof(uint32_t), hipMemcpyHostToDevice, sh->primary));
        return ANRAG_OK;
    };
    hipStream_t home = g->shard[0]->primary;
    auto pin_rec = [&](int b) { return reinterpret_cast<anrag_candidate *>(g->h_pin + kPinOut + b * kPinBlock); };
    auto pin_cnt = [&](int b) { return reinterpret_cast<int32_t *>(pin_rec(b) + (size_t)kBatchedQueries * kListLen); };
    auto pin_flag = [&](int b) { return pin_cnt(b) + kBatchedQueries; };

    auto enqueue = [&](int32_t c) -> int {
        const int b = c % kBatchedBlocks;
        const int32_t q0 = c * kBatchedQueries, nq = std::min(kBatchedQueries, n_queries - q0);
        float *h_q = g->h_bq + (size_t)b * kBatchedQueries * dim;  // free: the host has waited for chunk c - 2
        memcpy(h_q, queries + (int64_t)q0 * dim, (size_t)nq * dim * sizeof(float));
        for (int32_t i = 0; i < S; ++i) {
            anrag_index *sh = g->shard[i];
            DeviceGuard guard(g->device[i]);
            // (the home shard's own stream orders its pass behind the merge that read the block)
            if (i > 0) ANRAG_HIP(hipStreamWaitEvent(sh->primary, g->ev_merged[b], 0));
            ANRAG_HIP(hipMemcpyAsync(d_q[i], h_q, (size_t)nq * dim * sizeof(float), hipMemcpyHostToDevice, sh->primary));
            if (int r = launch_dense_batched(sh, sh->primary, d_q[i], nq, k, allow_source ? g->d_allow_a[i] : nullptr,
                                             d_rec[i][b], d_flag[i][b]))
                return r;
            if (i > 0) ANRAG_HIP(hipEventRecord(g->ev_pass[i][b], sh->primary));
        }
        DeviceGuard guard(g->device[0]);
        const anrag_candidate *src_rec = d_rec[0][b];
        const int32_t *src_cnt = nullptr, *src_flag = d_flag[0][b];
        if (S > 1) {
            BatchedMergeArgs a;
            for (int32_t i = 0; i < ANRAG_GROUP_MAX_SHARDS; ++i) {
                a.list[i] = d_rec[0][b];
                a.flag[i] = d_flag[0][b];
            }
            for (int32_t i = 1; i < S; ++i) {
                ANRAG_HIP(hipStreamWaitEvent(home, g->ev_pass[i][b], 0));  // the device waits, not the host
                if (g->in_place[i]) {
                    a.list[i] = d_rec[i][b];
                    a.flag[i] = d_flag[i][b];
                } else {
                    char *st = g->d_bstage[i] + b * kStageBlock;
                    ANRAG_HIP(hipMemcpyPeerAsync(st, g->device[0], d_rec[i][b], g->device[i],
                                                 (size_t)nq * k * sizeof(anrag_candidate), home));
                    ANRAG_HIP(hipMemcpyPeerAsync(st + kStageFlags, g->device[0], d_flag[i][b], g->device[i],
                                                 (size_t)nq * sizeof(int32_t), home));
                    a.list[i] = reinterpret_cast<const anrag_candidate *>(st);
                    a.flag[i] = reinterpret_cast<const int32_t *>(st + kStageFlags);
                }
            }
            a.n_shards = S;
            a.k = k;
            a.out = d_out;
            a.count = d_cnt;
            a.out_flag = d_oflag;
            {
                LaunchTimer t(g->shard[0], ANRAG_KERNEL_SELECT, home, nq);
                group_batched_merge_kernel<<<nq, kWave, 0, home>>>(a);
                ANRAG_HIP(hipGetLastError());
            }
            src_rec = d_out;
            src_cnt = d_cnt;
            src_flag = d_oflag;
        }
        ANRAG_HIP(hipMemcpyAsync(pin_rec(b), src_rec, (size_t)nq * k * sizeof(anrag_candidate), hipMemcpyDeviceToHost, home));
        if (src_cnt) ANRAG_HIP(hipMemcpyAsync(pin_cnt(b), src_cnt, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, home));
        ANRAG_HIP(hipMemcpyAsync(pin_flag(b), src_flag, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, home));
        ANRAG_HIP(hipEventRecord(g->ev_merged[b], home));
        return ANRAG_OK;
    };
    auto run = [&]() -> int {
        for (int32_t i = 0; i < S; ++i)
            if (int r = setup(i)) return r;
        if (int r = enqueue(0)) return r;
        for (int32_t c = 0; c < n_chunks; ++c) {
            if (c + 1 < n_chunks)
                if (int r = enqueue(c + 1)) return r;
            const int b = c % kBatchedBlocks;
            const int32_t q0 = c * kBatchedQueries, nq = std::min(kBatchedQueries, n_queries - q0);
            {   // the chunk's one host wait: by the event chain it follows every shard's pass of the chunk
                DeviceGuard guard(g->device[0]);
                ANRAG_HIP(hipEventSynchronize(g->ev_merged[b]));
            }
            const anrag_candidate *rec = pin_rec(b);
            for (int32_t qi = 0; qi < nq; ++qi) {
                const int64_t at = (int64_t)(q0 + qi) * k;
                unpack_records(rec + (size_t)qi * k, k, out_doc + at, out_score + at, out_count + q0 + qi);
                if (S > 1) out_count[q0 + qi] = pin_cnt(b)[qi];  // the merge kernel's own count
                if (pin_flag(b)[qi] != 0) redo.push_back(q0 + qi);
            }
            g->b_passes += 1;
            g->b_queries += nq;
        }
        return ANRAG_OK;
    };
    rc = run();
    if (rc)  // nothing may still run on a shard's stream, or read the pinned staging, when the next call uses them again
        for (int32_t i = 0; i < S; ++i) {
            DeviceGuard guard(g->device[i]);
            (void)hipStreamSynchronize(g->shard[i]->primary);
        }
    return rc;
}

// cold routes: the lists the shards returned, shard after shard -> the first k by (score desc), stably
template <typename S>
void merge_host(const std::vector<int64_t> &doc, const std::vector<S> &score, int32_t k, int64_t *out_doc, S *out_score,
                int32_t *out_count) {
    std::vector<int32_t> order;
    for (size_t i = 0; i < doc.size(); ++i)
        if (doc[i] >= 0) order.push_back((int32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return score[x] > score[y]; });
    const int32_t cnt = (int32_t)std::min<size_t>(order.size(), (size_t)k);
    for (int32_t i = 0; i < k; ++i) {
        out_doc[i] = i < cnt ? doc[order[i]] : -1;
        out_score[i] = i < cnt ? score[order[i]] : -std::numeric_limits<S>::infinity();
    }
    *out_count = cnt;
}

}  // namespace

#define ANRAG_GROUP_ENTER(g)                                             \
    ANRAG_REQUIRE((g) != nullptr, "shard group handle is NULL");         \
    std::lock_guard<std::mutex> lock__((g)->mu)

extern "C" {

int anrag_shard_group_create(const int32_t *devices, int32_t n_shards, anrag_shard_group **out) {
    ANRAG_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    ANRAG_REQUIRE(devices != nullptr, "devices is NULL");
    ANRAG_REQUIRE(n_shards >= 1 && n_shards <= ANRAG_GROUP_MAX_SHARDS, "n_shards %d out of range [1, %d]", n_shards,
                  ANRAG_GROUP_MAX_SHARDS);
    anrag_shard_group *g = new (std::nothrow) anrag_shard_group();
    if (!g) {
        set_error("out of host memory");
        return ANRAG_ERR_NOMEM;
    }
    if (const char *e = getenv("ANRAG_GROUP_BATCHED"))  // "0": query lists stay on the hot route (A/B measurements)
        g->batched_on = !(e[0] == '0' && e[1] == 0);
    auto build = [&]() -> int {
        for (int32_t i = 0; i < n_shards; ++i) {
            g->device[i] = devices[i];
            if (int rc = anrag_index_create(devices[i], &g->shard[i])) return rc;  // no device: ANRAG_ERR_NODEVICE, no fallback
            g->n = i + 1;
        }
        for (int32_t i = 0; i < n_shards; ++i) {
            DeviceGuard guard(g->device[i]);
            Carver measure(nullptr);
            measure.take<anrag_candidate>(kSlabRecords);
            measure.take<uint32_t>(kAllowWords);
            measure.take<uint32_t>(kAllowWords);
            ANRAG_HIP(counted_malloc(&g->d_block[i], (size_t)measure.at));
            g->own_bytes += measure.at;
            Carver cv(g->d_block[i]);
            g->d_slab[i] = cv.take<anrag_candidate>(kSlabRecords);
            g->d_allow_a[i] = cv.take<uint32_t>(kAllowWords);
            g->d_allow_b[i] = cv.take<uint32_t>(kAllowWords);
            if (i > 0) {  // the home shard's records are ordered by its own streams
                for (hipEvent_t &e : g->ev_cand[i]) ANRAG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                for (hipEvent_t &e : g->ev_pass[i]) ANRAG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            }
        }
        DeviceGuard guard(g->device[0]);
        for (hipEvent_t &e : g->ev_tail) ANRAG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (hipEvent_t &e : g->ev_merged) ANRAG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ANRAG_HIP(counted_host_malloc(reinterpret_cast<void **>(&g->h_pin), kPinBytes, hipHostMallocDefault));
        g->in_place[0] = true;
        for (int32_t i = 1; i < n_shards; ++i) {
            if (g->device[i] == g->device[0]) {
                g->in_place[i] = true;
                continue;
            }
            int can = 0;
            ANRAG_HIP(hipDeviceCanAccessPeer(&can, g->device[0], g->device[i]));
            if (can) {
                const hipError_t e = hipDeviceEnablePeerAccess(g->device[i], 0);  // for the current (home) device
                if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
                g->in_place[i] = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
            }
            if (!g->in_place[i]) {
                ANRAG_HIP(counted_malloc(&g->d_stage[i], (size_t)kSlabRecords * sizeof(anrag_candidate)));
                g->own_bytes += kSlabRecords * (int64_t)sizeof(anrag_candidate);
                if (g->batched_on) {
                    ANRAG_HIP(counted_malloc(&g->d_bstage[i], kBatchedBlocks * kStageBlock));
                    g->own_bytes += (int64_t)(kBatchedBlocks * kStageBlock);
                }
            }
        }
        return ANRAG_OK;
    };
    g->n = 0;
    const int rc = build();
    if (rc) {
        destroy(g);
        return rc;
    }
    *out = g;
    return ANRAG_OK;
}

int anrag_shard_group_destroy(anrag_shard_group *g) {
    if (g) destroy(g);
    return ANRAG_OK;
}

int anrag_shard_group_dense_load(anrag_shard_group *g, const float *embeddings, int64_t n_rows, int32_t dim,
                                 const uint16_t *source_id, const int64_t *doc_id, int64_t doc_id_base) {
    ANRAG_GROUP_ENTER(g);
    ANRAG_REQUIRE(embeddings != nullptr, "embeddings is NULL");
    ANRAG_REQUIRE(dim > 0 && dim <= 65536, "dim %d out of range", dim);
    ANRAG_REQUIRE(n_rows >= g->n, "%lld rows cannot be cut into %d shards", (long long)n_rows, g->n);
    int rc;
    if ((rc = drain(g))) return rc;
    g->has_dense = false;
    if (dim != g->dim) {  // the pinned staging of the single query and of the batched route's chunks follows the dimension
        DeviceGuard guard(g->device[0]);
        if (g->h_query) (void)counted_host_free(g->h_query);
        if (g->h_bq) (void)counted_host_free(g->h_bq);
        g->h_query = g->h_bq = nullptr;
        g->dim = 0;
        ANRAG_HIP(counted_host_malloc(reinterpret_cast<void **>(&g->h_query), (size_t)dim * sizeof(float), hipHostMallocDefault));
        if (g->batched_on)
            ANRAG_HIP(counted_host_malloc(reinterpret_cast<void **>(&g->h_bq),
                                          (size_t)kBatchedBlocks * kBatchedQueries * dim * sizeof(float), hipHostMallocDefault));
        g->dim = dim;
    }
    shard_bounds(n_rows, g->n, g->dense_lo);
    for (int32_t i = 0; i < g->n; ++i) {
        const int64_t lo = g->dense_lo[i], hi = g->dense_lo[i + 1];
        if ((rc = anrag_dense_load(g->shard[i], embeddings + lo * dim, hi - lo, dim, source_id ? source_id + lo : nullptr,
                                   doc_id ? doc_id + lo : nullptr, doc_id_base + lo)))
            return rc;
    }
    g->has_dense = true;
    g->has_dense_src = source_id != nullptr;
    return ANRAG_OK;
}

int anrag_shard_group_bm25_load(anrag_shard_group *g, const int64_t *indptr, int64_t n_terms, const int32_t *post_doc,
                                const int32_t *post_tf, const double *idf, const int32_t *doc_len, int64_t n_docs,
                                double avgdl, double k1, double b, const uint16_t *source_id, const int64_t *doc_id,
                                int64_t doc_id_base) {
    ANRAG_GROUP_ENTER(g);
    ANRAG_REQUIRE(indptr && post_doc && post_tf && idf && doc_len, "NULL operand");
    ANRAG_REQUIRE(n_terms > 0 && n_terms < 0x7FFFFFFF, "n_terms %lld out of range", (long long)n_terms);
    ANRAG_REQUIRE(n_docs >= g->n, "%lld documents cannot be cut into %d shards", (long long)n_docs, g->n);
    ANRAG_REQUIRE(indptr[0] == 0, "indptr[0] must be 0");
    for (int64_t t = 0; t < n_terms; ++t)
        ANRAG_REQUIRE(indptr[t + 1] >= indptr[t], "indptr not monotone at term %lld", (long long)t);
    int rc;
    if ((rc = drain(g))) return rc;
    g->has_bm25 = false;
    shard_bounds(n_docs, g->n, g->bm25_lo);
    // cut[t * (S + 1) + i]: first posting of term t whose document is >= bm25_lo[i] (documents ascend inside a term)
    const int32_t S = g->n;
    std::vector<int64_t> cut((size_t)n_terms * (S + 1));
    for (int64_t t = 0; t < n_terms; ++t) {
        const int32_t *first = post_doc + indptr[t], *last = post_doc + indptr[t + 1];
        int64_t *c = cut.data() + (size_t)t * (S + 1);
        c[0] = indptr[t];
        c[S] = indptr[t + 1];
        for (int32_t i = 1; i < S; ++i)
            c[i] = indptr[t] + (std::lower_bound(first, last, (int32_t)g->bm25_lo[i]) - first);
    }
    std::vector<int64_t> s_indptr((size_t)n_terms + 1);
    std::vector<int32_t> s_doc, s_tf;
    for (int32_t i = 0; i < S; ++i) {
        const int64_t lo = g->bm25_lo[i], hi = g->bm25_lo[i + 1];
        s_indptr[0] = 0;
        for (int64_t t = 0; t < n_terms; ++t) {
            const int64_t *c = cut.data() + (size_t)t * (S + 1);
            ANRAG_REQUIRE(c[i + 1] >= c[i], "postings of term %lld do not ascend", (long long)t);
            s_indptr[t + 1] = s_indptr[t] + (c[i + 1] - c[i]);
        }
        const int64_t np = s_indptr[n_terms];
        s_doc.resize((size_t)std::max<int64_t>(np, 1));
        s_tf.resize((size_t)std::max<int64_t>(np, 1));
        for (int64_t t = 0; t < n_terms; ++t) {
            const int64_t a = cut[(size_t)t * (S + 1) + i], n = s_indptr[t + 1] - s_indptr[t];
            for (int64_t j = 0; j < n; ++j) {
                s_doc[s_indptr[t] + j] = post_doc[a + j] - (int32_t)lo;
                s_tf[s_indptr[t] + j] = post_tf[a + j];
            }
        }
        // idf, avgdl, k1, b as given: the GLOBAL statistics keep a score the single index's bits
        if ((rc = anrag_bm25_load(g->shard[i], s_indptr.data(), n_terms, s_doc.data(), s_tf.data(), idf, doc_len + lo, hi - lo,
                                  avgdl, k1, b, source_id ? source_id + lo : nullptr, doc_id ? doc_id + lo : nullptr,
                                  doc_id_base + lo)))
            return rc;
    }
    g->has_bm25 = true;
    g->has_bm25_src = source_id != nullptr;
    return ANRAG_OK;
}

int anrag_shard_group_hybrid_search(anrag_shard_group *g, const float *query, const int32_t *term_ids, int32_t n_terms,
                                    int32_t similarity_k, double w_dense, double w_bm25, double wrrf_k, int32_t top_n,
                                    const uint8_t *allow_dense, int32_t n_dense_sources, const uint8_t *allow_bm25,
                                    int32_t n_bm25_sources, int64_t *out_id, double *out_score, int32_t *out_count) {
    ANRAG_GROUP_ENTER(g);
    ANRAG_REQUIRE(out_id && out_score && out_count, "NULL operand");
    ANRAG_REQUIRE(g->has_dense || g->has_bm25, "hybrid search before a load");
    ANRAG_REQUIRE(top_n > 0 && top_n <= 2 * ANRAG_FUSED_K_MAX, "top_n %d out of range", top_n);
    ANRAG_REQUIRE(n_terms >= 0 && n_terms <= kGroupTermsMax, "n_terms %d out of range [0, %d]", n_terms, kGroupTermsMax);
    ANRAG_REQUIRE(n_terms == 0 || term_ids != nullptr, "term_ids is NULL");
    const int64_t off[2] = {0, n_terms};
    const HotCall c{kGroupFuse, query, term_ids, off, 1, similarity_k, w_dense, w_bm25, wrrf_k, top_n,
                    allow_dense, n_dense_sources, allow_bm25, n_bm25_sources};
    std::vector<anrag_candidate> h;
    std::vector<int32_t> cnt;
    if (int rc = run_hot(g, c, h, cnt)) return rc;
    const int32_t m = std::min(cnt[0], top_n);
    for (int32_t i = 0; i < m; ++i) {
        out_id[i] = h[i].doc;
        out_score[i] = h[i].score;
    }
    *out_count = m;
    return ANRAG_OK;
}

int anrag_shard_group_hybrid_search_batch(anrag_shard_group *g, const float *queries, const int32_t *term_ids,
                                          const int64_t *term_offsets, int32_t n_queries, int32_t similarity_k,
                                          double w_dense, double w_bm25, double wrrf_k, int32_t top_n,
                                          const uint8_t *allow_dense, int32_t n_dense_sources,
                                          const uint8_t *allow_bm25, int32_t n_bm25_sources, int64_t *out_id,
                                          double *out_score, int32_t *out_count) {
    ANRAG_GROUP_ENTER(g);
    ANRAG_REQUIRE(out_id && out_score && out_count && term_offsets, "NULL operand");
    ANRAG_REQUIRE(g->has_dense || g->has_bm25, "hybrid search before a load");
    ANRAG_REQUIRE(top_n > 0 && top_n <= 2 * ANRAG_FUSED_K_MAX, "top_n %d out of range", top_n);
    ANRAG_REQUIRE(n_queries >= 0, "n_queries %d out of range", n_queries);
    if (n_queries == 0) return ANRAG_OK;
    const HotCall c{kGroupFuse, queries, term_ids, term_offsets, n_queries, similarity_k, w_dense, w_bm25, wrrf_k, top_n,
                    allow_dense, n_dense_sources, allow_bm25, n_bm25_sources};
    std::vector<anrag_candidate> h;
    std::vector<int32_t> cnt;
    if (int rc = run_hot(g, c, h, cnt)) return rc;
    for (int32_t q = 0; q < n_queries; ++q) {
        const int32_t m = std::min(cnt[q], top_n);
        for (int32_t i = 0; i < top_n; ++i) {
            out_id[(int64_t)q * top_n + i] = i < m ? h[(size_t)q * top_n + i].doc : -1;
            out_score[(int64_t)q * top_n + i] = i < m ? h[(size_t)q * top_n + i].score : -__builtin_huge_val();
        }
        out_count[q] = m;
    }
    return ANRAG_OK;
}

int anrag_shard_group_dense_search(anrag_shard_group *g, const float *queries, int32_t n_queries, int32_t k,
                                   const uint8_t *allow_source, int32_t n_sources, int64_t *out_doc, float *out_score,
                                   int32_t *out_count) {
    ANRAG_GROUP_ENTER(g);
    ANRAG_REQUIRE(g->has_dense, "dense search before anrag_shard_group_dense_load");
    ANRAG_REQUIRE(queries && out_doc && out_score && out_count, "NULL operand");
    ANRAG_REQUIRE(n_queries > 0 && k > 0, "n_queries and k must be positive");
    ANRAG_REQUIRE(!(allow_source && !g->has_dense_src), "a source filter needs source ids");
    if (k > ANRAG_FUSED_K_MAX) {  // cold: shard by shard, merged here
        std::vector<int64_t> doc((size_t)g->n * k), d1(k);
        std::vector<float> score((size_t)g->n * k), s1(k);
        for (int32_t q = 0; q < n_queries; ++q) {
            for (int32_t i = 0; i < g->n; ++i) {
                int32_t cnt = 0;
                if (int rc = anrag_dense_search(g->shard[i], queries + (int64_t)q * g->dim, 1, k, allow_source, n_sources,
                                                doc.data() + (size_t)i * k, score.data() + (size_t)i * k, &cnt))
                    return rc;
                for (int32_t j = cnt; j < k; ++j) doc[(size_t)i * k + j] = -1;
            }
            merge_host<float>(doc, score, k, out_doc + (int64_t)q * k, out_score + (int64_t)q * k, out_count + q);
        }
        return ANRAG_OK;
    }
    bool batched = g->batched_on;  // the single index's own gate, on every shard
    for (int32_t i = 0; i < g->n; ++i) batched = batched && batched_path_applies(g->shard[i], n_queries, k);
    if (batched) {
        ANRAG_REQUIRE(n_queries <= (1 << 20), "n_queries %d out of range", n_queries);
        std::vector<int32_t> redo;
        if (int rc = run_batched(g, queries, n_queries, k, allow_source, n_sources, out_doc, out_score, out_count, redo)) return rc;
        if (redo.empty()) return ANRAG_OK;
        // a survivor list overflowed on some shard (batched_select_kernel): the batch = 1 scans answer these queries, on
        // every shard, as anrag_dense_search redoes them on one index
        std::vector<float> rq(redo.size() * (size_t)g->dim);
        for (size_t j = 0; j < redo.size(); ++j)
            memcpy(rq.data() + j * g->dim, queries + (int64_t)redo[j] * g->dim, (size_t)g->dim * sizeof(float));
        const HotCall c{kGroupDense, rq.data(), nullptr, nullptr, (int32_t)redo.size(), k, 0, 0, 0, 0,
                        allow_source, n_sources, nullptr, 0};
        std::vector<anrag_candidate> h;
        std::vector<int32_t> cnt;
        if (int rc = run_hot(g, c, h, cnt)) return rc;
        for (size_t j = 0; j < redo.size(); ++j) {
            const int64_t q = redo[j];
            for (int32_t i = 0; i < k; ++i) {
                out_doc[q * k + i] = h[j * k + i].doc;
                out_score[q * k + i] = (float)h[j * k + i].score;
            }
            out_count[q] = cnt[j];
        }
        g->b_redone += (int64_t)redo.size();
        return ANRAG_OK;
    }
    const HotCall c{kGroupDense, queries, nullptr, nullptr, n_queries, k, 0, 0, 0, 0, allow_source, n_sources, nullptr, 0};
    std::vector<anrag_candidate> h;
    std::vector<int32_t> cnt;
    if (int rc = run_hot(g, c, h, cnt)) return rc;
    for (int32_t q = 0; q < n_queries; ++q) {
        for (int32_t i = 0; i < k; ++i) {
            out_doc[(int64_t)q * k + i] = h[(size_t)q * k + i].doc;
            out_score[(int64_t)q * k + i] = (float)h[(size_t)q * k + i].score;
        }
        out_count[q] = cnt[q];
    }
    return ANRAG_OK;
}

int anrag_shard_group_dense_search_f64(anrag_shard_group *g, const double *query, int32_t k, const uint8_t *allow_source,
                                       int32_t n_sources, int64_t *out_doc, double *out_score, int32_t *out_count) {
    ANRAG_GROUP_ENTER(g);
    ANRAG_REQUIRE(g->has_dense, "dense search before anrag_shard_group_dense_load");
    ANRAG_REQUIRE(query && out_doc && out_score && out_count, "NULL operand");
    ANRAG_REQUIRE(k > 0, "k must be positive");
    std::vector<int64_t> doc((size_t)g->n * k);
    std::vector<double> score((size_t)g->n * k);
    for (int32_t i = 0; i < g->n; ++i) {
        int32_t cnt = 0;
        if (int rc = anrag_dense_search_f64(g->shard[i], query, k, allow_source, n_sources, doc.data() + (size_t)i * k,
                                            score.data() + (size_t)i * k, &cnt))
            return rc;
        for (int32_t j = cnt; j < k; ++j) doc[(size_t)i * k + j] = -1;
    }
    merge_host<double>(doc, score, k, out_doc, out_score, out_count);
    return ANRAG_OK;
}

int anrag_shard_group_bm25_search(anrag_shard_group *g, const int32_t *term_ids, int32_t n_terms, int32_t k,
                                  const uint8_t *allow_source, int32_t n_sources, int64_t *out_doc, double *out_score,
                                  int32_t *out_count) {
    ANRAG_GROUP_ENTER(g);
    ANRAG_REQUIRE(g->has_bm25, "BM25 search before anrag_shard_group_bm25_load");
    ANRAG_REQUIRE(out_doc && out_score && out_count, "NULL operand");
    ANRAG_REQUIRE(k > 0, "k must be positive");
    ANRAG_REQUIRE(n_terms >= 0 && n_terms <= kGroupTermsMax, "n_terms %d out of range [0, %d]", n_terms, kGroupTermsMax);
    ANRAG_REQUIRE(n_terms == 0 || term_ids != nullptr, "term_ids is NULL");
    ANRAG_REQUIRE(!(allow_source && !g->has_bm25_src), "a source filter needs source ids");
    if (k > ANRAG_FUSED_K_MAX) {
        std::vector<int64_t> doc((size_t)g->n * k);
        std::vector<double> score((size_t)g->n * k);
        for (int32_t i = 0; i < g->n; ++i) {
            int32_t cnt = 0;
            if (int rc = anrag_bm25_search(g->shard[i], term_ids, n_terms, k, allow_source, n_sources,
                                           doc.data() + (size_t)i * k, score.data() + (size_t)i * k, &cnt))
                return rc;
            for (int32_t j = cnt; j < k; ++j) doc[(size_t)i * k + j] = -1;
        }
        merge_host<double>(doc, score, k, out_doc, out_score, out_count);
        return ANRAG_OK;
    }
    const int64_t off[2] = {0, n_terms};
    const HotCall c{kGroupBm25, nullptr, term_ids, off, 1, k, 0, 0, 0, 0, nullptr, 0, allow_source, n_sources};
    std::vector<anrag_candidate> h;
    std::vector<int32_t> cnt;
    if (int rc = run_hot(g, c, h, cnt)) return rc;
    for (int32_t i = 0; i < k; ++i) {
        out_doc[i] = h[i].doc;
        out_score[i] = h[i].score;
    }
    *out_count = cnt[0];
    return ANRAG_OK;
}

int anrag_shard_group_debug_enqueue(anrag_shard_group *g, int64_t *out_groups, int64_t *out_ns) {
    ANRAG_GROUP_ENTER(g);
    if (out_groups) *out_groups = (int64_t)g->seq;
    if (out_ns) *out_ns = g->enqueue_ns;
    return ANRAG_OK;
}

int anrag_shard_group_set_dense_prefilter(anrag_shard_group *g, int32_t mode) {
    ANRAG_GROUP_ENTER(g);
    for (int32_t i = 0; i < g->n; ++i)
        if (int rc = anrag_set_dense_prefilter(g->shard[i], mode)) return rc;
    return ANRAG_OK;
}

int anrag_shard_group_set_batched_precision(anrag_shard_group *g, int32_t mode) {
    ANRAG_GROUP_ENTER(g);
    for (int32_t i = 0; i < g->n; ++i)
        if (int rc = anrag_set_batched_precision(g->shard[i], mode)) return rc;
    return ANRAG_OK;
}

int anrag_shard_group_batched_stats(anrag_shard_group *g, int64_t *passes, int64_t *queries, int64_t *redone) {
    ANRAG_GROUP_ENTER(g);
    if (passes) *passes = g->b_passes;
    if (queries) *queries = g->b_queries;
    if (redone) *redone = g->b_redone;
    return ANRAG_OK;
}

int anrag_shard_group_sync(anrag_shard_group *g) {
    ANRAG_GROUP_ENTER(g);
    return drain(g);
}

int anrag_shard_group_info(anrag_shard_group *g, int32_t *n_shards, int64_t *dense_row_lo, int64_t *bm25_doc_lo,
                           int64_t *hbm_bytes) {
    ANRAG_GROUP_ENTER(g);
    if (n_shards) *n_shards = g->n;
    for (int32_t i = 0; i <= g->n; ++i) {
        if (dense_row_lo) dense_row_lo[i] = g->has_dense ? g->dense_lo[i] : 0;
        if (bm25_doc_lo) bm25_doc_lo[i] = g->has_bm25 ? g->bm25_lo[i] : 0;
    }
    if (hbm_bytes) {
        int64_t total = g->own_bytes;
        for (int32_t i = 0; i < g->n; ++i) {
            int64_t b = 0;
            if (int rc = anrag_index_info(g->shard[i], nullptr, nullptr, nullptr, nullptr, &b)) return rc;
            total += b;
        }
        *hbm_bytes = total;
    }
    return ANRAG_OK;
}

int anrag_shard_group_shard(anrag_shard_group *g, int32_t i, anrag_index **out) {
    ANRAG_GROUP_ENTER(g);
    ANRAG_REQUIRE(out != nullptr, "out is NULL");
    ANRAG_REQUIRE(i >= 0 && i < g->n, "shard %d out of range (%d shards)", i, g->n);
    *out = g->shard[i];
    return ANRAG_OK;
}

}  // extern "C"
