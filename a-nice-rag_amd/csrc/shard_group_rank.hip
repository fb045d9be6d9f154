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

struct ShardDev : RankLegRun {  // one shard's share of one leg
    int device = 0;
    int64_t lo = 0;
    bool in_place = true;
    uint32_t *stage_rows = nullptr;  // on the home device, for a shard it cannot map
    double *stage_keys = nullptr;
    int32_t *stage_cnt = nullptr;
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
    RankPlan p;
    int rc;
    if ((rc = rank_plan_call(p, legs != nullptr, n_legs, n_queries, similarity_k, wrrf_k, top_n, id_space, out_id, out_score,
                             out_count, expect_id, out_rank)))
        return rc;
    RankLegOps ops[ANRAG_WRRF_MAX_LISTS];
    for (int l = 0; l < n_legs; ++l) {
        const anrag_group_rank_leg &g = legs[l];
        ANRAG_REQUIRE((g.group != nullptr) != (g.idx != nullptr), "leg %d: exactly one of group and idx must be set", l);
        ops[l] = rank_leg_ops(g);
        if ((rc = rank_plan_kind(l, ops[l], 1u << ANRAG_LEG_DENSE | 1u << ANRAG_LEG_BM25))) return rc;
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
    for (int l = 0; l < n_legs; ++l) {
        const anrag_group_rank_leg &g = legs[l];
        if (g.idx) {
            if ((rc = rank_plan_index(l, ops[l], g.idx))) return rc;
            leg_rows[l] = ld[l].sh[0].rows = g.kind == ANRAG_LEG_DENSE ? g.idx->n_rows : g.idx->n_docs;
        }
        if ((rc = rank_plan_leg(p, l, ops[l], leg_rows[l]))) return rc;
        for (int32_t s = 0; s < ld[l].n_shards; ++s) {
            ShardDev &sd = ld[l].sh[s];
            sd.st = sd.ix->primary;
            sd.kind = g.kind;
            sd.stride = (sd.rows + 63) / 64 * 64;
            sd.k = (int32_t)std::min<int64_t>(similarity_k, sd.rows);
        }
    }
    if ((rc = rank_plan_fusion(p, ops))) return rc;
    const int32_t *leg_k = p.leg_k;
    for (anrag_index *o : owners) {
        DeviceGuard guard(o->device);
        if ((rc = settle_pipeline(o))) return rc;
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
    for (int l = 0; l < n_legs; ++l) {
        const bool dense = legs[l].kind == ANRAG_LEG_DENSE;
        for (int32_t s = 0; s < ld[l].n_shards; ++s) {
            const ShardDev &sd = ld[l].sh[s];
            p.per_query += sd.stride * (dense ? 4 : 8) + (int64_t)sd.k * 12 + 768 + 4 + 4;
            p.per_query += dense ? (int64_t)sd.ix->dim * 4 : 8;
            if (!sd.in_place) p.per_query += (int64_t)sd.k * 12 + 768;
            p.fixed += 2048 * 4 + 256 + 8 + 256;
        }
        if (ld[l].merged) p.per_query += (int64_t)leg_k[l] * 12 + 768;
        p.fixed += kMergeFields * ANRAG_GROUP_MAX_SHARDS * 8 + 256 + (legs[l].doc_of_row ? leg_rows[l] * 4 + 256 : 0);
    }
    rank_plan_chunk(p, ops);
    const int64_t chunk = p.chunk;

    // ---- carve: every shard's pieces out of ITS rank_pool, the home pieces out of the home index's; once to measure,
    // once for real
    RankTail tail;
    tail.device = home_dev;
    tail.st = home;
    std::vector<PoolUse> pools;
    for (anrag_index *o : owners) pools.push_back(PoolUse{o, Carver(nullptr)});
    auto pool_of = [&](anrag_index *ix) -> Carver & {
        for (PoolUse &u : pools)
            if (u.ix == ix) return u.cv;
        return pools[0].cv;  // (every index of the call is an owner)
    };
    auto carve = [&]() {
        Carver &hv = pool_of(home_ix);
        for (int l = 0; l < n_legs; ++l) {
            for (int32_t s = 0; s < ld[l].n_shards; ++s) {
                ShardDev &sd = ld[l].sh[s];
                sd.carve(pool_of(sd.ix), p, legs[l].allow_source != nullptr, true);
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
        tail.carve(hv, p, expect_id != nullptr);
    };
    carve();
    for (PoolUse &u : pools) {
        DeviceGuard guard(u.ix->device);
        if ((rc = ensure_pool(u.ix, u.ix->rank_pool, u.cv.at + 256))) return rc;
        u.cv = Carver(u.ix->rank_pool.p);
    }
    carve();
    for (PoolUse &u : pools)
        if (u.cv.at > u.ix->rank_pool.bytes) {
            set_error("internal: rank scratch carve %lld > pool %lld", (long long)u.cv.at, (long long)u.ix->rank_pool.bytes);
            return ANRAG_ERR_STATE;
        }

    // ---- per-call uploads: allow bitmaps to every shard, document maps and the merge tables to the home device
    for (int l = 0; l < n_legs; ++l) {
        for (int32_t s = 0; legs[l].allow_source && s < ld[l].n_shards; ++s) {
            DeviceGuard guard(ld[l].sh[s].device);
            if ((rc = rank_stage_allow(ld[l].sh[s], ops[l]))) return rc;
        }
        if (ld[l].doc_of_row && (rc = rank_stage_map(home, legs[l].doc_of_row, leg_rows[l], ld[l].doc_of_row))) return rc;
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
    for (int l = 0; l < n_legs; ++l)
        tail.leg[l] = RankTailLeg{ld[l].rows, ld[l].row_keys, ld[l].cnt, ld[l].doc_of_row, leg_k[l], legs[l].weight};
    if ((rc = rank_stage_fuse_table(tail))) return rc;

    auto run = [&]() -> int {
        for (int64_t q0 = 0; q0 < n_queries; q0 += chunk) {
            const int32_t c = (int32_t)std::min<int64_t>(chunk, n_queries - q0);
            if ((rc = rank_stage_expect(tail, expect_id, q0, c))) return rc;
            for (int l = 0; l < n_legs; ++l) {
                int32_t longest = 0;
                for (int32_t s = 0; s < ld[l].n_shards; ++s) {
                    ShardDev &sd = ld[l].sh[s];
                    longest = std::max(longest, sd.k);
                    {  // operands up, score tiles, the sort -- all on the shard's primary stream
                        DeviceGuard guard(sd.device);
                        if (!guard.ok) {
                            set_error("hipSetDevice(%d) failed", sd.device);
                            return ANRAG_ERR_HIP;
                        }
                        if ((rc = rank_leg_chunk(sd, ops[l], q0, c, nullptr))) return rc;
                        if (sd.ix->primary == home) continue;  // the home stream's own order
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
