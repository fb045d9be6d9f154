// Full ranking for LISTS of queries across the shards of a shard group: anrag_shard_group_rank_batch (include/anrag.h).
//
// Per chunk of queries and per leg every shard runs the single index's score tiles and per-query sort over ITS rows,
// on its own primary stream and out of its own rank_pool, and leaves a list per query in its HBM: local rows, fp64
// scores, a count, in (score desc, local row asc) order.  It records an event; the home stream (leg 0's shard 0) waits
// for it -- the host does not -- and runs ONE shard_list_merge_kernel per leg, which merges the S sorted lists of every
// query into the leg's global list, in the buffers the single index's fusion and emit consume (rank_batch.hip:
// launch_rank_tail).  One host sync per chunk, on the home stream.
//
// The merge ranks by counting: entry p of shard s has global rank
//     p + sum over t < s of #{entries of t with score >= mine} + sum over t > s of #{entries of t with score > mine}
// -- among equal scores the earlier shard, then the earlier position, stays ahead; shards are ascending contiguous row
// blocks, so that is (score desc, global row asc), the single index's order, whatever the document map (shard_group.hip,
// "Why the merge is in SHARD ORDER").  Each term is a binary search over a sorted peer list; every output slot is
// written exactly once, nothing is atomic.  Peer lists are read where they are (peer access) or staged to the home device
// with hipMemcpyPeerAsync on the home stream.
//
// One leg and out_id == NULL ("only the rank of the expected document"): the single index counts instead of sorting
// (rank_count_kernel); across shards the lists are formed and the rank is read from them.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"

namespace anrag {

constexpr int kMergeThreads = 256;
constexpr int kMergeFields = 5;  // table: field f of shard s at tab[f * ANRAG_GROUP_MAX_SHARDS + s]
                                 // 0 rows (uint32 *)  1 keys (double *)  2 counts (int32 *)  3 list stride  4 first global row

// order-preserving bits of a score, as the sort kernels compare them: -0.0 == +0.0
__device__ __forceinline__ uint64_t merge_order_bits(double v) {
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if ((b << 1) == 0) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// grid (queries, ceil(longest list / 256), shards): a thread owns entry p of shard s of query q.  s and q are uniform in
// a workgroup, so the table reads are scalar loads.
__global__ __launch_bounds__(kMergeThreads) void shard_list_merge_kernel(const uint64_t *__restrict__ tab, int32_t n_shards,
                                                                         int32_t leg_k, uint32_t *__restrict__ out_rows,
                                                                         double *__restrict__ out_keys,
                                                                         int32_t *__restrict__ out_cnt) {
    constexpr int S = ANRAG_GROUP_MAX_SHARDS;
    const int64_t q = blockIdx.x;
    const int s = blockIdx.z;
    const int32_t p = blockIdx.y * kMergeThreads + threadIdx.x;
    auto count_of = [&](int t) __attribute__((always_inline)) { return reinterpret_cast<const int32_t *>(tab[2 * S + t])[q]; };
    auto keys_of = [&](int t) __attribute__((always_inline)) {
        return reinterpret_cast<const double *>(tab[S + t]) + q * (int64_t)tab[3 * S + t];
    };
    if (blockIdx.y == 0 && s == 0 && threadIdx.x == 0) {
        int64_t total = 0;
        for (int t = 0; t < n_shards; ++t) total += count_of(t);
        out_cnt[q] = (int32_t)(total < leg_k ? total : leg_k);
    }
    if (p >= count_of(s) || p >= leg_k) return;  // rank >= p: an entry at or past leg_k is never part of the answer
    const double key = keys_of(s)[p];
    const uint64_t x = merge_order_bits(key);
    int32_t r = p;
    for (int t = 0; t < n_shards; ++t) {
        if (t == s) continue;
        // entries of t ahead of mine; more than leg_k - r of them put mine outside the list, so the search stops there
        const int32_t n_t = count_of(t), room = leg_k - r;
        int32_t lo = 0, hi = n_t < room ? n_t : room;
        const double *__restrict__ kt = keys_of(t);
        const bool strict = t > s;  // a later shard stays behind an equal score
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            const uint64_t u = merge_order_bits(kt[mid]);
            if (strict ? u > x : u >= x) lo = mid + 1;
            else hi = mid;
        }
        r += lo;
        if (r >= leg_k) return;
    }
    const uint32_t row = (reinterpret_cast<const uint32_t *>(tab[s]) + q * (int64_t)tab[3 * S + s])[p];
    out_rows[q * leg_k + r] = (uint32_t)tab[4 * S + s] + row;
    if (out_keys) out_keys[q * leg_k + r] = key;
}

namespace {

struct ShardDev {  // one shard's share of one leg
    anrag_index *ix = nullptr;
    int device = 0;
    int64_t lo = 0, rows = 0, stride = 0;
    int32_t k = 0;  // min(similarity_k, rows)
    bool in_place = true;
    uint32_t *allow = nullptr;
    float *q = nullptr;
    int32_t *terms = nullptr, *seg_k = nullptr;
    int64_t *term_off = nullptr;
    void *scores = nullptr;
    uint32_t *list_rows = nullptr;
    double *list_keys = nullptr;
    int32_t *list_cnt = nullptr;
    uint32_t *stage_rows = nullptr;  // on the home device, for a shard it cannot map
    double *stage_keys = nullptr;
    int32_t *stage_cnt = nullptr;
    std::vector<int32_t> h_segk;
    std::vector<int64_t> h_off;
    RankWide wide;  // the wide select's scratch, where the mode takes it for this shard's block
};

struct LegDev {
    int32_t n_shards = 0;
    bool merged = true;  // false: one shard on the home device, its lists ARE the leg's
    ShardDev sh[ANRAG_GROUP_MAX_SHARDS];
    int32_t *doc_of_row = nullptr;
    uint64_t *tab = nullptr;
    uint32_t *rows = nullptr;
    double *row_keys = nullptr;
    int32_t *cnt = nullptr;
};

struct PoolUse {
    anrag_index *ix;
    Carver cv;
};

}  // namespace
}  // namespace anrag

using namespace anrag;

extern "C" int anrag_shard_group_rank_batch(const anrag_group_rank_leg *legs, int32_t n_legs, int32_t n_queries,
                                            int32_t similarity_k, double wrrf_k, int32_t top_n, int64_t id_space,
                                            int64_t *out_id, double *out_score, int32_t *out_count,
                                            const int64_t *expect_id, int32_t *out_rank) {
    ANRAG_REQUIRE(legs != nullptr && n_legs >= 1 && n_legs <= ANRAG_WRRF_MAX_LISTS, "n_legs %d out of range [1, %d]", n_legs,
                  ANRAG_WRRF_MAX_LISTS);
    ANRAG_REQUIRE(n_queries >= 0 && n_queries <= (1 << 22), "n_queries %d out of range", n_queries);
    ANRAG_REQUIRE(similarity_k > 0 && top_n > 0, "similarity_k and top_n must be positive");
    ANRAG_REQUIRE(out_count != nullptr, "out_count is NULL");
    ANRAG_REQUIRE(!out_score || out_id, "out_score without out_id");
    ANRAG_REQUIRE((expect_id != nullptr) == (out_rank != nullptr), "expect_id and out_rank come together");
    ANRAG_REQUIRE(out_id || out_rank, "nothing to return: out_id and out_rank are both NULL");
    for (int l = 0; l < n_legs; ++l) {
        const anrag_group_rank_leg &g = legs[l];
        ANRAG_REQUIRE((g.group != nullptr) != (g.idx != nullptr), "leg %d: exactly one of group and idx must be set", l);
        ANRAG_REQUIRE(g.kind == ANRAG_LEG_DENSE || g.kind == ANRAG_LEG_BM25, "leg %d: kind %d", l, g.kind);
        ANRAG_REQUIRE(g.weight > 0.0 && g.weight < __builtin_huge_val(), "leg %d: weight must be positive and finite", l);
    }
    if (n_queries == 0) return ANRAG_OK;
    const bool fuse = n_legs > 1;

    // ---- locks: the groups in address order, then every inner index in address order
    std::vector<std::mutex *> group_mu;
    for (int l = 0; l < n_legs; ++l)
        if (legs[l].group) {
            std::mutex *m = shard_group_view(legs[l].group).mu;
            if (std::find(group_mu.begin(), group_mu.end(), m) == group_mu.end()) group_mu.push_back(m);
        }
    std::sort(group_mu.begin(), group_mu.end());
    std::vector<std::unique_lock<std::mutex>> locks;
    for (std::mutex *m : group_mu) locks.emplace_back(*m);
    std::vector<LegDev> ld((size_t)n_legs);
    std::vector<anrag_index *> owners;
    int64_t leg_rows[ANRAG_WRRF_MAX_LISTS];
    for (int l = 0; l < n_legs; ++l) {
        const anrag_group_rank_leg &g = legs[l];
        const bool dense = g.kind == ANRAG_LEG_DENSE;
        if (g.group) {
            const GroupView v = shard_group_view(g.group);
            ANRAG_REQUIRE(dense ? v.has_dense : v.has_bm25, "leg %d: ranking before the group's %s load", l,
                          dense ? "dense" : "BM25");
            ANRAG_REQUIRE(!(g.allow_source && !(dense ? v.has_dense_src : v.has_bm25_src)),
                          "leg %d: a source filter needs source ids", l);
            const int64_t *lo = dense ? v.dense_lo : v.bm25_lo;
            ld[l].n_shards = v.n;
            for (int32_t s = 0; s < v.n; ++s) {
                ld[l].sh[s].ix = v.shard[s];
                ld[l].sh[s].device = v.device[s];
                ld[l].sh[s].lo = lo[s];
                ld[l].sh[s].rows = lo[s + 1] - lo[s];
            }
            leg_rows[l] = lo[v.n];
        } else {
            ld[l].n_shards = 1;
            ld[l].sh[0].ix = g.idx;
            ld[l].sh[0].device = g.idx->device;
        }
        for (int32_t s = 0; s < ld[l].n_shards; ++s)
            if (std::find(owners.begin(), owners.end(), ld[l].sh[s].ix) == owners.end()) owners.push_back(ld[l].sh[s].ix);
    }
    std::sort(owners.begin(), owners.end());
    for (anrag_index *o : owners) locks.emplace_back(o->mu);

    // ---- operands and the envelope, on the GLOBAL list of every leg
    int32_t leg_k[ANRAG_WRRF_MAX_LISTS];
    int64_t sum_k = 0;
    for (int l = 0; l < n_legs; ++l) {
        const anrag_group_rank_leg &g = legs[l];
        const bool dense = g.kind == ANRAG_LEG_DENSE;
        if (g.idx) {
            if (dense) {
                ANRAG_REQUIRE(g.idx->d_emb != nullptr, "leg %d: dense ranking before anrag_dense_load", l);
                ANRAG_REQUIRE(!(g.allow_source && !g.idx->d_dense_src), "leg %d: a source filter needs source ids", l);
            } else {
                ANRAG_REQUIRE(g.idx->d_post_doc != nullptr, "leg %d: BM25 ranking before anrag_bm25_load", l);
                ANRAG_REQUIRE(!(g.allow_source && !g.idx->d_bm25_src), "leg %d: a source filter needs source ids", l);
            }
            leg_rows[l] = ld[l].sh[0].rows = dense ? g.idx->n_rows : g.idx->n_docs;
        }
        if (dense) {
            ANRAG_REQUIRE(g.queries != nullptr, "leg %d: queries is NULL", l);
        } else {
            ANRAG_REQUIRE(g.term_offsets != nullptr && g.term_offsets[0] == 0, "leg %d: bad term offsets", l);
            ANRAG_REQUIRE(g.term_offsets[n_queries] == 0 || g.term_ids != nullptr, "leg %d: term_ids is NULL", l);
            for (int32_t q = 0; q < n_queries; ++q)
                ANRAG_REQUIRE(g.term_offsets[q + 1] >= g.term_offsets[q] && g.term_offsets[q + 1] - g.term_offsets[q] <= 4096,
                              "leg %d, query %d: term count out of range [0, 4096]", l, q);
        }
        ANRAG_REQUIRE(leg_rows[l] > 0 && leg_rows[l] < 0x7FFFFFFFll, "leg %d: %lld rows (the batched ranking takes < 2^31)", l,
                      (long long)leg_rows[l]);
        ANRAG_REQUIRE(!g.allow_source || (g.n_sources >= 0 && g.n_sources <= 65536), "leg %d: n_sources out of range", l);
        leg_k[l] = (int32_t)std::min<int64_t>(similarity_k, leg_rows[l]);
        const int32_t cap = rank_list_cap(!dense);
        ANRAG_REQUIRE(leg_k[l] <= cap, "leg %d: min(similarity_k, rows) = %d is outside the batched ranking's envelope (%d)",
                      l, leg_k[l], cap);
        for (int32_t s = 0; s < ld[l].n_shards; ++s) {
            ShardDev &sd = ld[l].sh[s];
            sd.stride = (sd.rows + 63) / 64 * 64;
            sd.k = (int32_t)std::min<int64_t>(similarity_k, sd.rows);
        }
        sum_k += leg_k[l];
    }
    bool fuse_in_lds = false;
    int32_t fuse_n = 0;
    if (fuse) {
        ANRAG_REQUIRE(id_space > 0 && id_space < 0x7FFFFFFFll, "id_space %lld out of range", (long long)id_space);
        fuse_n = (int32_t)std::min<int64_t>(std::min<int64_t>(top_n, sum_k), id_space);
        ANRAG_REQUIRE(fuse_n <= rank_list_cap(true), "min(top_n, entries) = %d is outside the batched ranking's envelope (%d)",
                      fuse_n, rank_list_cap(true));
        fuse_in_lds = id_space <= rank_list_cap(true) && !getenv("ANRAG_RANK_FUSE_IN_HBM");
        const int64_t *maps[ANRAG_WRRF_MAX_LISTS];
        for (int l = 0; l < n_legs; ++l) maps[l] = legs[l].doc_of_row;
        if (int rc = rank_check_maps(n_legs, maps, leg_rows, id_space)) return rc;
    }
    for (anrag_index *o : owners) {
        DeviceGuard guard(o->device);
        if (int rc = settle_pipeline(o)) return rc;
    }

    // ---- the home device: leg 0's shard 0.  Which shards' lists it reads in place
    anrag_index *home_ix = ld[0].sh[0].ix;
    const int home_dev = ld[0].sh[0].device;
    hipStream_t home = home_ix->primary;
    DeviceGuard home_guard(home_dev);
    if (!home_guard.ok) {
        set_error("hipSetDevice(%d) failed", home_dev);
        return ANRAG_ERR_HIP;
    }
    for (int l = 0; l < n_legs; ++l) {
        for (int32_t s = 0; s < ld[l].n_shards; ++s) {
            ShardDev &sd = ld[l].sh[s];
            if (sd.device == home_dev) continue;
            int can = 0;
            ANRAG_HIP(hipDeviceCanAccessPeer(&can, home_dev, sd.device));
            sd.in_place = false;
            if (can) {
                const hipError_t e = hipDeviceEnablePeerAccess(sd.device, 0);  // for the current (home) device
                if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
                sd.in_place = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
            }
        }
        ld[l].merged = !(ld[l].n_shards == 1 && ld[l].sh[0].device == home_dev);
    }

    // ---- sizes: the chunk from the global leg sizes, as anrag_rank_batch computes it
    const int32_t out_n = fuse ? fuse_n : (int32_t)std::min<int64_t>(top_n, leg_k[0]);
    int64_t per_query = 0, fixed = 0;
    for (int l = 0; l < n_legs; ++l) {
        const bool dense = legs[l].kind == ANRAG_LEG_DENSE;
        for (int32_t s = 0; s < ld[l].n_shards; ++s) {
            const ShardDev &sd = ld[l].sh[s];
            per_query += sd.stride * (dense ? 4 : 8) + (int64_t)sd.k * 12 + 768 + 4 + 4;
            per_query += dense ? (int64_t)sd.ix->dim * 4 : 8;
            if (!sd.in_place) per_query += (int64_t)sd.k * 12 + 768;
            fixed += 2048 * 4 + 256 + 8 + 256;
        }
        if (ld[l].merged) per_query += (int64_t)leg_k[l] * 12 + 768;
        fixed += kMergeFields * ANRAG_GROUP_MAX_SHARDS * 8 + 256 + (legs[l].doc_of_row ? leg_rows[l] * 4 + 256 : 0);
    }
    if (fuse && !fuse_in_lds) per_query += id_space * 12 + 512 + (int64_t)fuse_n * 12 + 512 + 4;
    if (fuse) per_query += 4 + 256;
    fixed += 1024;
    per_query += (int64_t)out_n * 16 + 4 + 512 + 16;
    int64_t budget = 6ll << 30;
    if (const char *e = getenv("ANRAG_RANK_CHUNK_BUDGET"))  // measurements and tests: bytes of scratch a chunk may take
        budget = std::max<int64_t>(1, atoll(e));
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_queries, (budget - fixed) / std::max<int64_t>(per_query, 1)));
    if (chunk > 8) chunk = chunk / 8 * 8;
    int64_t max_terms_chunk = 0;
    for (int l = 0; l < n_legs; ++l)
        if (legs[l].kind == ANRAG_LEG_BM25)
            for (int64_t q0 = 0; q0 < n_queries; q0 += chunk) {
                const int64_t q1 = std::min<int64_t>(n_queries, q0 + chunk);
                max_terms_chunk = std::max(max_terms_chunk, legs[l].term_offsets[q1] - legs[l].term_offsets[q0]);
            }

    // ---- carve: every shard's pieces out of ITS rank_pool, the home pieces out of the home index's; once to measure,
    // once for real
    double *d_f = nullptr, *d_skey = nullptr, *d_out_score = nullptr;
    uint32_t *d_t = nullptr, *d_stie = nullptr;
    int32_t *d_scnt = nullptr, *d_out_cnt = nullptr, *d_rank = nullptr;
    uint64_t *d_fuse_legs = nullptr;
    int64_t *d_out_id = nullptr, *d_expect = nullptr;
    RankWide fuse_wide;
    const int32_t c_full = (int32_t)std::min<int64_t>(chunk, n_queries);  // segments of a full chunk's sort launches
    std::vector<PoolUse> pools;
    for (anrag_index *o : owners) pools.push_back(PoolUse{o, Carver(nullptr)});
    auto pool_of = [&](anrag_index *ix) -> Carver & {
        for (PoolUse &p : pools)
            if (p.ix == ix) return p.cv;
        return pools[0].cv;  // (every index of the call is an owner)
    };
    auto carve = [&]() {
        Carver &hv = pool_of(home_ix);
        for (int l = 0; l < n_legs; ++l) {
            const bool dense = legs[l].kind == ANRAG_LEG_DENSE;
            for (int32_t s = 0; s < ld[l].n_shards; ++s) {
                ShardDev &sd = ld[l].sh[s];
                Carver &cv = pool_of(sd.ix);
                sd.allow = legs[l].allow_source ? cv.take<uint32_t>(2048) : nullptr;
                if (dense) {
                    sd.q = cv.take<float>(chunk * sd.ix->dim);
                    sd.scores = cv.take<float>(chunk * sd.stride);
                } else {
                    sd.terms = cv.take<int32_t>(std::max<int64_t>(max_terms_chunk, 1));
                    sd.seg_k = cv.take<int32_t>(chunk);
                    sd.term_off = cv.take<int64_t>(chunk + 1);
                    sd.scores = cv.take<double>(chunk * sd.stride);
                }
                sd.list_rows = cv.take<uint32_t>(chunk * sd.k);
                sd.list_keys = cv.take<double>(chunk * sd.k);
                sd.list_cnt = cv.take<int32_t>(chunk);
                sd.wide.bytes = rank_wide_wanted(!dense, c_full, (int32_t)sd.rows) ? rank_wide_bytes(!dense, c_full) : 0;
                sd.wide.scratch = sd.wide.bytes ? cv.take<char>(sd.wide.bytes) : nullptr;
                if (!sd.in_place) {
                    sd.stage_rows = hv.take<uint32_t>(chunk * sd.k);
                    sd.stage_keys = hv.take<double>(chunk * sd.k);
                    sd.stage_cnt = hv.take<int32_t>(chunk);
                }
            }
            ld[l].doc_of_row = legs[l].doc_of_row ? hv.take<int32_t>(leg_rows[l]) : nullptr;
            if (ld[l].merged) {
                ld[l].tab = hv.take<uint64_t>(kMergeFields * ANRAG_GROUP_MAX_SHARDS);
                ld[l].rows = hv.take<uint32_t>(chunk * leg_k[l]);
                ld[l].row_keys = fuse ? nullptr : hv.take<double>(chunk * leg_k[l]);
                ld[l].cnt = hv.take<int32_t>(chunk);
            } else {
                ld[l].rows = ld[l].sh[0].list_rows;
                ld[l].row_keys = ld[l].sh[0].list_keys;
                ld[l].cnt = ld[l].sh[0].list_cnt;
            }
        }
        if (fuse && !fuse_in_lds) {
            d_f = hv.take<double>(chunk * id_space);
            d_t = hv.take<uint32_t>(chunk * id_space);
            d_stie = hv.take<uint32_t>(chunk * fuse_n);
            d_skey = hv.take<double>(chunk * fuse_n);
        }
        if (fuse) d_scnt = hv.take<int32_t>(chunk);
        d_fuse_legs = fuse_in_lds ? hv.take<uint64_t>(6 * ANRAG_WRRF_MAX_LISTS) : nullptr;
        d_out_id = hv.take<int64_t>(chunk * out_n);
        d_out_score = hv.take<double>(chunk * out_n);
        d_out_cnt = fuse ? d_scnt : hv.take<int32_t>(chunk);
        d_expect = expect_id ? hv.take<int64_t>(chunk) : nullptr;
        d_rank = expect_id ? hv.take<int32_t>(chunk) : nullptr;
        fuse_wide.bytes = fuse && !fuse_in_lds && rank_wide_wanted(true, c_full, (int32_t)id_space) ? rank_wide_bytes(true, c_full) : 0;
        fuse_wide.scratch = fuse_wide.bytes ? hv.take<char>(fuse_wide.bytes) : nullptr;
    };
    carve();
    int rc;
    for (PoolUse &p : pools) {
        DeviceGuard guard(p.ix->device);
        if ((rc = ensure_pool(p.ix, p.ix->rank_pool, p.cv.at + 256))) return rc;
        p.cv = Carver(p.ix->rank_pool.p);
    }
    carve();
    for (PoolUse &p : pools)
        if (p.cv.at > p.ix->rank_pool.bytes) {
            set_error("internal: rank scratch carve %lld > pool %lld", (long long)p.cv.at, (long long)p.ix->rank_pool.bytes);
            return ANRAG_ERR_STATE;
        }

    // ---- per-call uploads: allow bitmaps to every shard, document maps and the merge tables to the home device
    std::vector<uint32_t> h_bits(2048);
    std::vector<int32_t> h_map;
    for (int l = 0; l < n_legs; ++l) {
        const anrag_group_rank_leg &g = legs[l];
        if (g.allow_source) {
            if (int rc = pack_allow_bits(g.allow_source, g.n_sources, h_bits.data())) return rc;
            for (int32_t s = 0; s < ld[l].n_shards; ++s) {
                ShardDev &sd = ld[l].sh[s];
                DeviceGuard guard(sd.device);
                ANRAG_HIP(hipMemcpyAsync(sd.allow, h_bits.data(), 2048 * 4, hipMemcpyHostToDevice, sd.ix->primary));
                ANRAG_HIP(hipStreamSynchronize(sd.ix->primary));  // h_bits is reused by the next leg
            }
        }
        if (g.doc_of_row) {
            h_map.resize((size_t)leg_rows[l]);
            for (int64_t r = 0; r < leg_rows[l]; ++r) h_map[(size_t)r] = (int32_t)g.doc_of_row[r];
            ANRAG_HIP(hipMemcpyAsync(ld[l].doc_of_row, h_map.data(), (size_t)leg_rows[l] * 4, hipMemcpyHostToDevice, home));
            ANRAG_HIP(hipStreamSynchronize(home));
        }
        if (ld[l].merged) {
            constexpr int S = ANRAG_GROUP_MAX_SHARDS;
            uint64_t tab[kMergeFields * S] = {};
            for (int32_t s = 0; s < ld[l].n_shards; ++s) {
                const ShardDev &sd = ld[l].sh[s];
                tab[s] = reinterpret_cast<uint64_t>(sd.in_place ? sd.list_rows : sd.stage_rows);
                tab[S + s] = reinterpret_cast<uint64_t>(sd.in_place ? sd.list_keys : sd.stage_keys);
                tab[2 * S + s] = reinterpret_cast<uint64_t>(sd.in_place ? sd.list_cnt : sd.stage_cnt);
                tab[3 * S + s] = (uint64_t)sd.k;
                tab[4 * S + s] = (uint64_t)sd.lo;
            }
            ANRAG_HIP(hipMemcpyAsync(ld[l].tab, tab, sizeof(tab), hipMemcpyHostToDevice, home));
            ANRAG_HIP(hipStreamSynchronize(home));
        }
    }
    RankTail tail;
    tail.device = home_dev;
    tail.st = home;
    tail.n_legs = n_legs;
    for (int l = 0; l < n_legs; ++l)
        tail.leg[l] = RankTailLeg{ld[l].rows, ld[l].row_keys, ld[l].cnt, ld[l].doc_of_row, leg_k[l], legs[l].weight};
    tail.fuse_in_lds = fuse_in_lds;
    tail.wrrf_k = wrrf_k;
    tail.id_space = id_space;
    tail.fuse_n = fuse_n;
    tail.out_n = out_n;
    tail.d_f = d_f;
    tail.d_t = d_t;
    tail.d_stie = d_stie;
    tail.d_skey = d_skey;
    tail.d_scnt = d_scnt;
    tail.d_fuse_legs = d_fuse_legs;
    tail.d_out_id = d_out_id;
    tail.d_out_score = d_out_score;
    tail.d_out_cnt = d_out_cnt;
    tail.d_expect = d_expect;
    tail.d_rank = d_rank;
    tail.wide = fuse_wide;
    if (fuse_in_lds) {
        uint64_t tab[6 * ANRAG_WRRF_MAX_LISTS];
        rank_fuse_table(tail, tab);
        ANRAG_HIP(hipMemcpyAsync(d_fuse_legs, tab, sizeof(tab), hipMemcpyHostToDevice, home));
        ANRAG_HIP(hipStreamSynchronize(home));
    }

    // one chunk of one leg on one shard: operands up, score tiles, the sort -- all on the shard's primary stream
    auto run_shard = [&](const anrag_group_rank_leg &g, ShardDev &sd, int64_t q0, int32_t c) -> int {
        DeviceGuard guard(sd.device);
        if (!guard.ok) {
            set_error("hipSetDevice(%d) failed", sd.device);
            return ANRAG_ERR_HIP;
        }
        anrag_index *ix = sd.ix;
        hipStream_t st = ix->primary;
        int r;
        if (g.kind == ANRAG_LEG_DENSE) {
            ANRAG_HIP(hipMemcpyAsync(sd.q, g.queries + q0 * ix->dim, (size_t)c * ix->dim * sizeof(float), hipMemcpyHostToDevice,
                                     st));
            float *tile = static_cast<float *>(sd.scores);
            const int tile_n = getenv("ANRAG_RANK_SCAN_TILES") ? 0 : dense_tile_group_max(ix);
            for (int32_t g0 = 0; tile_n > 0 && g0 < c; g0 += kTileLaunchMax)  // K1T: the rows once per launch
                if ((r = launch_dense_tile(ix, st, sd.q + (int64_t)g0 * ix->dim, ix->dim, std::min<int32_t>(kTileLaunchMax, c - g0),
                                           sd.allow, tile + (int64_t)g0 * sd.stride, sd.stride)))
                    return r;
            for (int32_t g0 = tile_n > 0 ? c : 0; g0 < c; g0 += kScanGroupMax) {  // other dimensions: a pass per query
                const int n = std::min<int32_t>(kScanGroupMax, c - g0);
                const float *qs[kScanGroupMax];
                int sets[kScanGroupMax];
                for (int i = 0; i < n; ++i) {
                    qs[i] = sd.q + (int64_t)(g0 + i) * ix->dim;
                    sets[i] = 0;  // unused: scores are written, no lists
                }
                if ((r = launch_dense_scan_group(ix, st, qs, n, 0, sd.allow, tile + (int64_t)g0 * sd.stride, sets, sd.stride)))
                    return r;
            }
            return launch_rank_sort(sd.device, st, c, tile, false, sd.stride, (int32_t)sd.rows, sd.k, nullptr, sd.list_rows,
                                    sd.list_keys, sd.k, sd.list_cnt, sd.wide);
        }
        const int64_t t0 = g.term_offsets[q0];
        const int64_t nt = g.term_offsets[q0 + c] - t0;
        if (nt > 0) ANRAG_HIP(hipMemcpyAsync(sd.terms, g.term_ids + t0, (size_t)nt * 4, hipMemcpyHostToDevice, st));
        sd.h_segk.resize((size_t)c);  // (the shard's own staging: it stays as it is until the chunk's host sync)
        sd.h_off.resize((size_t)c + 1);
        for (int32_t q = 0; q < c; ++q) {
            const int32_t n_terms = (int32_t)(g.term_offsets[q0 + q + 1] - g.term_offsets[q0 + q]);
            sd.h_segk[(size_t)q] = n_terms > 0 ? sd.k : 0;  // no tokens: the leg is skipped (search_engine.py:216-217)
        }
        for (int32_t q = 0; q <= c; ++q) sd.h_off[(size_t)q] = g.term_offsets[q0 + q] - t0;
        ANRAG_HIP(hipMemcpyAsync(sd.seg_k, sd.h_segk.data(), (size_t)c * 4, hipMemcpyHostToDevice, st));
        ANRAG_HIP(hipMemcpyAsync(sd.term_off, sd.h_off.data(), ((size_t)c + 1) * 8, hipMemcpyHostToDevice, st));
        double *tile = static_cast<double *>(sd.scores);
        for (int32_t g0 = 0; g0 < c; g0 += 32768)
            if ((r = launch_bm25_scores_table(ix, st, sd.terms, sd.term_off + g0, std::min<int32_t>(32768, c - g0), sd.allow,
                                              tile + (int64_t)g0 * sd.stride, sd.stride)))
                return r;
        return launch_rank_sort(sd.device, st, c, tile, true, sd.stride, (int32_t)sd.rows, sd.k, sd.seg_k, sd.list_rows,
                                sd.list_keys, sd.k, sd.list_cnt, sd.wide);
    };
    auto run = [&]() -> int {
        for (int64_t q0 = 0; q0 < n_queries; q0 += chunk) {
            const int32_t c = (int32_t)std::min<int64_t>(chunk, n_queries - q0);
            if (expect_id) {
                ANRAG_HIP(hipMemcpyAsync(d_expect, expect_id + q0, (size_t)c * 8, hipMemcpyHostToDevice, home));
                ANRAG_HIP(hipMemsetAsync(d_rank, 0xFF, (size_t)c * 4, home));  // -1: not in the answer
            }
            for (int l = 0; l < n_legs; ++l) {
                int32_t longest = 0;
                for (int32_t s = 0; s < ld[l].n_shards; ++s) {
                    ShardDev &sd = ld[l].sh[s];
                    if ((rc = run_shard(legs[l], sd, q0, c))) return rc;
                    longest = std::max(longest, sd.k);
                    if (sd.ix->primary == home) continue;  // the home stream's own order
                    {
                        DeviceGuard guard(sd.device);
                        if (!sd.ix->ev_order) ANRAG_HIP(hipEventCreateWithFlags(&sd.ix->ev_order, hipEventDisableTiming));
                        ANRAG_HIP(hipEventRecord(sd.ix->ev_order, sd.ix->primary));
                    }
                    ANRAG_HIP(hipStreamWaitEvent(home, sd.ix->ev_order, 0));  // the device waits, not the host
                    if (!sd.in_place) {
                        ANRAG_HIP(hipMemcpyPeerAsync(sd.stage_rows, home_dev, sd.list_rows, sd.device, (size_t)c * sd.k * 4, home));
                        ANRAG_HIP(hipMemcpyPeerAsync(sd.stage_keys, home_dev, sd.list_keys, sd.device, (size_t)c * sd.k * 8, home));
                        ANRAG_HIP(hipMemcpyPeerAsync(sd.stage_cnt, home_dev, sd.list_cnt, sd.device, (size_t)c * 4, home));
                    }
                }
                if (!ld[l].merged) continue;
                longest = std::min(longest, leg_k[l]);
                const dim3 grid((unsigned)c, (unsigned)((longest + kMergeThreads - 1) / kMergeThreads), (unsigned)ld[l].n_shards);
                shard_list_merge_kernel<<<grid, kMergeThreads, 0, home>>>(ld[l].tab, ld[l].n_shards, leg_k[l], ld[l].rows,
                                                                         ld[l].row_keys, ld[l].cnt);
                ANRAG_HIP(hipGetLastError());
            }
            if ((rc = launch_rank_tail(tail, c, out_id != nullptr))) return rc;
            // by the event chain the home stream's sync follows every shard's work of the chunk
            if ((rc = rank_copy_out(tail, c, q0, top_n, out_id, out_score, out_count, out_rank))) return rc;
        }
        return ANRAG_OK;
    };
    rc = run();
    if (rc)  // nothing may still run on a shard's stream when the next call carves its pool again
        for (anrag_index *o : owners) {
            DeviceGuard guard(o->device);
            (void)hipStreamSynchronize(o->primary);
        }
    return rc;
}
