// K1TD -- fp64 score TILES for lists of float64 queries (rank_batch.hip, leg kind ANRAG_LEG_DENSE_F64): every score of n
// fp64 queries against every fp32 row, row-stationary like K1T (dense_tile.hip).  A wave takes a batch of R whole rows
// into registers, converts them to fp64 ONCE, and runs the NQ queries of the group over them; the queries sit in LDS as
// doubles (NQ * CH * 2 KB, staged per workgroup).  HBM traffic per query falls by NQ against the one-query routes.
//
// The arithmetic is K1D's (dense_scan_f64.hip) and dense_scores_f64_kernel's (dense_scan.hip), for every D % 4 == 0:
//   * 64 lanes per row; lane l runs ONE chain acc = fma(double(e[c]), q[c], acc) from 0.0 over c = 4l .. 4l+3, then the
//     same four offsets of every following 256-float chunk, ascending; a lane whose offsets lie past D in the last chunk
//     leaves its accumulator alone (its load is taken from the row's last float4: in bounds, not used);
//   * the 64 accumulators are summed by the tree "distance 32, then 16, 8, 4, 2, 1";
//   * nan_first.
// The tree is run TRANSPOSED.  A batch yields V = R * NQ independent (row, query) accumulator vectors, value t = query *
// R + row.  Instead of six exchanges and six adds per value, two vectors are merged into one per level:
//   distance 32: (X, Y) -> v_permlane32_swap -> {X.lo, Y.lo} + {X.hi, Y.hi}: lanes 0..31 hold X's partial sums, lanes
//                32..63 Y's, each lane the sum its own lane of the plain butterfly holds (both partners of a butterfly
//                step add the same two values, and IEEE addition commutes: the same bits);
//   distance 16: v_permlane16_swap in the same way (rows of 16 lanes);
//   distance d = 8, 4, 2, 1: lane & d picks whose value the lane keeps (0: X, else Y); it adds its own copy of that
//                vector to what lane ^ d sends of it (wave_topk.hpp's VALU exchanges).
// Vectors merge like the carries of a binary counter (values 2j and 2j+1 at distance 32, the results of 4j..4j+1 and
// 4j+2..4j+3 at distance 16, ...), so at most one vector per level waits.  After L = log2(min(V, 64)) levels every lane
// holds a partial sum of ONE value; the 6 - L remaining distances are plain butterfly steps.  V - 1 merge adds per V
// values instead of 6 V.  The lane that ends up with value t: bit (5 - j) of the lane = bit j of t for j < L (a bit
// reversal); tests/test_rank_f64_leg_cpu.py models the schedule and holds the store indexing below to it.
// Streaming as in K1D: nt dwordx4 loads, two register sets, the next batch issued unconditionally before the current one is
// reduced (counted waits), the allow bitmap in LDS for the filtered form.  A wave owns a contiguous block of rows.
// Geometry ("K1TD"): CH = ceil(D / 256) in {1, 2, 3, 4, 8}; other dimensions take per-query passes of
// dense_scores_f64_kernel (rank_batch.hip), same bits.
#include "common.hpp"
#include "wave_topk.hpp"
#include "dense_scan_common.hpp"

namespace anrag {

// 8 waves share a group's queries: two waves per SIMD beside up to 128 KB of LDS (one workgroup per CU)
constexpr int kTile64Threads = 512;
constexpr int kTile64Waves = kTile64Threads / kWave;

// rows per wave and batch, queries per LDS group
template <int CH>
constexpr int tile64_r() { return CH == 1 ? 8 : (CH == 2 ? 4 : (CH <= 4 ? 2 : 1)); }
template <int CH>
constexpr int tile64_nq() { return CH <= 4 ? 16 : 8; }
constexpr bool tile64_has(int ch) { return ch == 1 || ch == 2 || ch == 3 || ch == 4 || ch == 8; }

// one level of the transposed tree: x (the earlier value(s)) and y (the later) -> one vector
template <int DIST>
__device__ __forceinline__ double tile64_merge(double x, double y, int lane) {
    const unsigned long long bx = (unsigned long long)__double_as_longlong(x), by = (unsigned long long)__double_as_longlong(y);
    if constexpr (DIST == 32) {
        const auto lo = __builtin_amdgcn_permlane32_swap((uint32_t)bx, (uint32_t)by, false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap((uint32_t)(bx >> 32), (uint32_t)(by >> 32), false, false);
        return __longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0])) +
               __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1]));
    } else if constexpr (DIST == 16) {
        const auto lo = __builtin_amdgcn_permlane16_swap((uint32_t)bx, (uint32_t)by, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap((uint32_t)(bx >> 32), (uint32_t)(by >> 32), false, false);
        return __longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0])) +
               __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1]));
    } else {
        const bool second = (lane & DIST) != 0;
        const double own = second ? y : x, send = second ? x : y;
        return own + lane_xor<DIST>(send);
    }
}

template <int LEVEL>
__device__ __forceinline__ double tile64_merge_level(double x, double y, int lane) {
    return tile64_merge<(32 >> LEVEL)>(x, y, lane);
}

// value t of a batch joins the counter; true when a vector of 2^L values is complete (then in v)
template <int L>
__device__ __forceinline__ bool tile64_push(double (&st)[6], int t, double &v, int lane) {
#pragma unroll
    for (int lev = 0; lev < L; ++lev) {
        if (((t >> lev) & 1) == 0) {
            st[lev] = v;
            return false;
        }
        if (lev == 0) v = tile64_merge_level<0>(st[0], v, lane);
        else if (lev == 1) v = tile64_merge_level<1>(st[1], v, lane);
        else if (lev == 2) v = tile64_merge_level<2>(st[2], v, lane);
        else if (lev == 3) v = tile64_merge_level<3>(st[3], v, lane);
        else if (lev == 4) v = tile64_merge_level<4>(st[4], v, lane);
        else v = tile64_merge_level<5>(st[5], v, lane);
    }
    return true;
}

template <int CH, bool FILTER>
__global__ __launch_bounds__(kTile64Threads) void dense_tile_f64_kernel(
    const float *__restrict__ emb, const double *__restrict__ queries, int64_t q_stride, int32_t n_q, int64_t n_rows,
    int32_t dim, const uint16_t *__restrict__ src, const uint32_t *__restrict__ allow_bits,
    double *__restrict__ scores_out, int64_t scores_stride) {
    constexpr int R = tile64_r<CH>(), NQ = tile64_nq<CH>();
    constexpr int V = R * NQ < kWave ? R * NQ : kWave;  // values per finished vector
    constexpr int L = V == 64 ? 6 : (V == 32 ? 5 : (V == 16 ? 4 : 3));
    static_assert((1 << L) == V && (R * NQ) % V == 0, "whole vectors per batch");
    constexpr int SLICE = CH * 256;  // doubles per query in LDS
    extern __shared__ __attribute__((aligned(16))) double tile64_lds[];
    __shared__ uint32_t lds_allow[FILTER ? kAllowWords : 1];
    const int lane = lane_id();
    const int32_t row_f4 = dim / 4;
    // the lane's float4 of the last chunk may lie past the row's end (D % 256 != 0): it is read from the row's last
    // float4 instead (in bounds) and not used
    const bool last_ok = (CH - 1) * kWave + lane < row_f4;
    const int32_t last_at = last_ok ? (CH - 1) * kWave + lane : row_f4 - 1;

    const int64_t total_waves = (int64_t)gridDim.x * kTile64Waves;
    const int64_t wave_global = (int64_t)blockIdx.x * kTile64Waves + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int64_t rows_per_wave = ((n_rows + total_waves - 1) / total_waves + R - 1) / R * R;
    const int64_t base0 = wave_global * rows_per_wave;
    const bool has_rows = base0 < n_rows;  // (a wave without rows still stages queries and meets the barriers)
    const int64_t lim = base0 + rows_per_wave < n_rows ? base0 + rows_per_wave : n_rows;

    // what this lane stores of finished vector j: value t = j * V + (the lane's upper L bits, reversed), for the lanes
    // whose lower 6 - L bits are zero (the butterfly steps leave the same sum in all 2^(6-L) of them)
    int t_lane = 0;
#pragma unroll
    for (int j = 0; j < L; ++j) t_lane |= ((lane >> (5 - j)) & 1) << j;
    const bool stores = (lane & ((1 << (6 - L)) - 1)) == 0;

    const f32x4 *__restrict__ ev = reinterpret_cast<const f32x4 *>(emb);
    struct Batch {
        f32x4 v[R][CH];
        uint32_t sid[R];
    };
    auto issue = [&](int64_t base, Batch &bt) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = base + r;
            const int64_t rc = row < n_rows ? row : n_rows - 1;  // clamp: rows past the end re-read the last row
            if constexpr (FILTER) bt.sid[r] = src[rc];
            const f32x4 *p = ev + rc * row_f4;
#pragma unroll
            for (int c = 0; c < CH; ++c)
                bt.v[r][c] = __builtin_nontemporal_load(p + (c < CH - 1 ? c * kWave + lane : last_at));
        }
    };
    Batch b0, b1;
    if (has_rows) issue(base0, b0);  // in flight while the first queries are staged
    if constexpr (FILTER)
        for (int i = threadIdx.x; i < kAllowWords; i += kTile64Threads) lds_allow[i] = allow_bits[i];

    for (int32_t g0 = 0; g0 < n_q; g0 += NQ) {
        const int32_t n_g = n_q - g0 < NQ ? n_q - g0 : NQ;
        if (g0 > 0) __syncthreads();  // every wave is done with the previous group's slices
        // query i of the group at [i * SLICE, i * SLICE + dim); the slots behind the group's last query keep what they
        // held (computed like any other, never stored)
        for (int32_t i = 0; i < n_g; ++i) {
            const double *q = queries + (int64_t)(g0 + i) * q_stride;
            for (int32_t j = threadIdx.x; j < dim; j += kTile64Threads) tile64_lds[i * SLICE + j] = q[j];
        }
        __syncthreads();
        if (!has_rows) continue;
        double *__restrict__ out = scores_out + (int64_t)g0 * scores_stride;
        auto reduce = [&](int64_t base, const Batch &bt) {
            uint32_t okm = 0xFFFFFFFFu;  // bit r: row r of the batch passes the filter
            if constexpr (FILTER) {
                okm = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) okm |= source_ok(lds_allow, bt.sid[r]) ? 1u << r : 0u;
            }
            double e[R][CH][4];  // the batch's rows as doubles: converted once, not once per query
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const f32x4 v = bt.v[r][c];
                    e[r][c][0] = (double)v.x;
                    e[r][c][1] = (double)v.y;
                    e[r][c][2] = (double)v.z;
                    e[r][c][3] = (double)v.w;
                }
            double st[6];
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                double acc[R];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = 0.0;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int32_t at = i * SLICE + 4 * (c < CH - 1 ? c * kWave + lane : last_at);
                    const double q0 = tile64_lds[at], q1 = tile64_lds[at + 1], q2 = tile64_lds[at + 2],
                                 q3 = tile64_lds[at + 3];
                    // (the R chains of a query are independent: the scheduler interleaves them)
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        double a = acc[r];
                        a = __builtin_fma(e[r][c][0], q0, a);
                        a = __builtin_fma(e[r][c][1], q1, a);
                        a = __builtin_fma(e[r][c][2], q2, a);
                        a = __builtin_fma(e[r][c][3], q3, a);
                        acc[r] = (c < CH - 1 || last_ok) ? a : acc[r];
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int t = i * R + r;
                    double v = acc[r];
                    if (tile64_push<L>(st, t % V, v, lane)) {
                        // the distances the transposed levels did not cover: the plain butterfly
                        if constexpr (L < 4) v += lane_xor<4>(v);
                        if constexpr (L < 5) v += lane_xor<2>(v);
                        if constexpr (L < 6) v += lane_xor<1>(v);
                        v = nan_first(v);
                        const int tv = (t / V) * V + t_lane;  // this lane's value of the vector
                        const int qi = tv / R, r_l = tv % R;
                        if constexpr (FILTER) v = ((okm >> r_l) & 1u) ? v : neg_inf<double>();
                        const int64_t row = base + r_l;
                        if (stores && qi < n_g && row < lim) out[(int64_t)qi * scores_stride + row] = v;
                    }
                }
                // two queries (2 R independent chains) between barriers: without any the scheduler hoists every query's
                // LDS reads (500+ registers, spills)
                if (i % 2 == 1) __builtin_amdgcn_sched_barrier(0);
            }
        };
        // two register sets, the next batch issued before this one is reduced (behind the wave's last batch: its
        // first rows again, unconditionally -- see K1D's loop; they are the next group's first batch)
        for (int64_t base = base0;;) {
            int64_t next = base + R;
            issue(next < lim ? next : base0, b1);
            reduce(base, b0);
            if (next >= lim) {  // b1 holds the first batch again
                b0 = b1;
                break;
            }
            base = next;
            next = base + R;
            issue(next < lim ? next : base0, b0);
            reduce(base, b1);
            if (next >= lim) break;  // b0 holds the first batch again
            base = next;
        }
    }
}

// Queries one K1TD workgroup holds in LDS at a time at this index's dimension (0: no tile kernel for it -- rank_batch.hip
// then scores each query of the list with one dense_scores_f64_kernel pass, same bits).
int dense_tile_f64_group_max(const anrag_index *idx) {
    if (idx->d_emb == nullptr || idx->dim < 4 || idx->dim % 4 != 0) return 0;
    switch ((idx->dim + 255) / 256) {
        case 1: return tile64_nq<1>();
        case 2: return tile64_nq<2>();
        case 3: return tile64_nq<3>();
        case 4: return tile64_nq<4>();
        case 8: return tile64_nq<8>();
        default: return 0;
    }
}

template <int CH>
static int launch_k1td(anrag_index *idx, hipStream_t st, const double *d_queries, int64_t q_stride, int32_t n_queries,
                       const uint32_t *allow, double *d_scores_out, int64_t scores_stride) {
    constexpr int R = tile64_r<CH>();
    const int lds = tile64_nq<CH>() * CH * 256 * (int)sizeof(double);
    // one workgroup of 8 waves per CU (the LDS of the long rows leaves room for one; a wave holds up to 256 registers)
    const int64_t need = (idx->n_rows + kTile64Waves * R - 1) / (kTile64Waves * R);
    const int64_t cap = (int64_t)idx->n_cus;
    const unsigned grid = (unsigned)(need < cap ? (need > 0 ? need : 1) : cap);
    if (allow) {
        if (int rc = ensure_dynamic_lds(idx->device, reinterpret_cast<const void *>(&dense_tile_f64_kernel<CH, true>), lds))
            return rc;
        dense_tile_f64_kernel<CH, true><<<grid, kTile64Threads, lds, st>>>(idx->d_emb, d_queries, q_stride, n_queries,
                                                                         idx->n_rows, idx->dim, idx->d_dense_src, allow,
                                                                         d_scores_out, scores_stride);
    } else {
        if (int rc = ensure_dynamic_lds(idx->device, reinterpret_cast<const void *>(&dense_tile_f64_kernel<CH, false>), lds))
            return rc;
        dense_tile_f64_kernel<CH, false><<<grid, kTile64Threads, lds, st>>>(idx->d_emb, d_queries, q_stride, n_queries,
                                                                          idx->n_rows, idx->dim, nullptr, nullptr,
                                                                          d_scores_out, scores_stride);
    }
    return ANRAG_OK;
}

// fp64 scores of n queries (d_queries + i * q_stride doubles) against every row: query i's to d_scores_out + i *
// scores_stride.  One launch; inside it the queries go through LDS in groups of dense_tile_f64_group_max().
int launch_dense_tile_f64(anrag_index *idx, hipStream_t st, const double *d_queries, int64_t q_stride, int32_t n_queries,
                          const uint32_t *d_allow_bits, double *d_scores_out, int64_t scores_stride) {
    ANRAG_REQUIRE(dense_tile_f64_group_max(idx) > 0, "no fp64 tile kernel for dimension %d", idx->dim);
    ANRAG_REQUIRE(n_queries >= 1 && n_queries <= kTileLaunchMax, "fp64 tile launch of %d queries (at most %d)", n_queries,
                  kTileLaunchMax);
    ANRAG_REQUIRE(n_queries == 1 || scores_stride >= idx->n_rows, "score tile rows overlap");
    ANRAG_REQUIRE(q_stride >= idx->dim, "fp64 tile launch: query stride %lld < dim %d", (long long)q_stride, idx->dim);
    const uint32_t *allow = (idx->d_dense_src != nullptr) ? d_allow_bits : nullptr;
    LaunchTimer t(idx, ANRAG_KERNEL_DENSE_SCAN, st, n_queries);
    int rc = ANRAG_OK;
    switch ((idx->dim + 255) / 256) {
        case 1: rc = launch_k1td<1>(idx, st, d_queries, q_stride, n_queries, allow, d_scores_out, scores_stride); break;
        case 2: rc = launch_k1td<2>(idx, st, d_queries, q_stride, n_queries, allow, d_scores_out, scores_stride); break;
        case 3: rc = launch_k1td<3>(idx, st, d_queries, q_stride, n_queries, allow, d_scores_out, scores_stride); break;
        case 4: rc = launch_k1td<4>(idx, st, d_queries, q_stride, n_queries, allow, d_scores_out, scores_stride); break;
        default: rc = launch_k1td<8>(idx, st, d_queries, q_stride, n_queries, allow, d_scores_out, scores_stride); break;
    }
    if (rc) return rc;
    ANRAG_HIP(hipGetLastError());
    return ANRAG_OK;
}

}  // namespace anrag
