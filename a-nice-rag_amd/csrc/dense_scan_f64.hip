// K1D -- the dense scan for ONE fp64 query (the reference's text path: the embedding API returns float64 and np.dot
// then promotes the fp32 matrix and scores in fp64, src/search_engine.py:157, :129), keeping lists like K1.
//
// The corpus stays fp32 in HBM; a row's score is the fp64 dot product of dense_scores_f64_kernel (dense_scan.hip), bit
// for bit -- that kernel stays the route of k > 64 and of the dimensions this one does not serve, and one query must
// not score differently on the two:
//   * 64 lanes per row; lane l runs ONE chain acc = fma(double(e[c]), q[c], acc) from 0.0 over c = 4l .. 4l+3, then the
//     same four offsets of every following 256-float chunk, ascending; a lane whose offsets lie past D in the last
//     chunk leaves its accumulator alone;
//   * acc += (acc of lane ^ 32), ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 -- the exchanges are wave_topk.hpp's VALU moves instead of
//     __shfl_xor's LDS round trips: both partners add the same two values, so the bits are the same and every lane ends
//     with the row's score;
//   * nan_first.
// Streaming as in K1: nt dwordx4 loads, two register sets, the next batch issued unconditionally before the current
// one is reduced (counted waits), the allow bitmap in LDS for the filtered form, K1's grid, one sorted 64-entry list
// (fp64 score + row) per wave for the tail (tail.hip) -- no score array.
// Geometry ("K1D"): whole rows, CH = ceil(D / 256) <= 12 loads per lane and row, scan_r<CH>() rows per batch
// (6-12 loads per lane and batch, twice that in flight), the lane's query slice in registers (8 * CH VGPRs).  This
// route runs with the pipeline settled: nothing shares the CU, so there is no 128-VGPR budget and long rows are not
// split in halves.
#include "common.hpp"
#include "wave_topk.hpp"
#include "dense_scan_common.hpp"

namespace anrag {

constexpr int kF64ScanMaxDim = 3072;
constexpr int kF64ScanMaxCH = kF64ScanMaxDim / 256;

template <int CH, bool FILTER>
__global__ __launch_bounds__(kScanThreads) void dense_scan_f64_kernel(
    const float *__restrict__ emb, const double *__restrict__ query, int64_t n_rows, int32_t dim, int32_t k,
    const uint16_t *__restrict__ src, const uint32_t *__restrict__ allow_bits, double *__restrict__ blk_s,
    uint32_t *__restrict__ blk_r) {
    constexpr int R = scan_r<CH>();  // rows per wave and batch
    __shared__ uint32_t lds_allow[FILTER ? kAllowWords : 1];
    const int lane = lane_id();
    const int wave = threadIdx.x / kWave;
    if constexpr (FILTER) {
        for (int i = threadIdx.x; i < kAllowWords; i += kScanThreads) lds_allow[i] = allow_bits[i];
        __syncthreads();
    }
    const int32_t row_f4 = dim / 4;
    // the lane's float4 of the last chunk may lie past the row's end (D % 256 != 0): it is read from the row's last
    // float4 instead (in bounds) and not used
    const bool last_ok = (CH - 1) * kWave + lane < row_f4;
    const int32_t last_at = last_ok ? (CH - 1) * kWave + lane : row_f4 - 1;
    double q[CH][4];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int32_t at = 4 * (c < CH - 1 ? c * kWave + lane : last_at);
#pragma unroll
        for (int j = 0; j < 4; ++j) q[c][j] = query[at + j];
    }
    WaveTopK<double> top;
    top.init(k);
    top.thr_s = neg_inf_opaque();  // signed scores: wave_topk.hpp
    const int64_t wave_global = (int64_t)blockIdx.x * kScanWaves + wave;
    const int64_t step = (int64_t)gridDim.x * kScanWaves * R;
    const int64_t base0 = wave_global * R;
    double *out_s = blk_s + wave_global * kListLen;
    uint32_t *out_r = blk_r + wave_global * kListLen;
    if (base0 >= n_rows) {  // a wave without rows: an empty list
        out_s[lane] = top.s;
        out_r[lane] = top.r;
        return;
    }
    struct Batch {
        f32x4 v[R][CH];
        uint32_t sid[R];
    };
    const f32x4 *__restrict__ ev = reinterpret_cast<const f32x4 *>(emb);
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
    auto reduce = [&](int64_t base, const Batch &bt) {
        // the batch's R candidates, row r's in lane r: ONE offer per batch
        double cs = neg_inf<double>();
        uint32_t cr = kNoRow;
        bool cf = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const f32x4 v = bt.v[r][c];
                double a = acc;
                a = __builtin_fma((double)v.x, q[c][0], a);
                a = __builtin_fma((double)v.y, q[c][1], a);
                a = __builtin_fma((double)v.z, q[c][2], a);
                a = __builtin_fma((double)v.w, q[c][3], a);
                acc = (c < CH - 1 || last_ok) ? a : acc;
            }
            acc += lane_xor<32>(acc);
            acc += lane_xor<16>(acc);
            acc += lane_xor<8>(acc);
            acc += lane_xor<4>(acc);
            acc += lane_xor<2>(acc);
            acc += lane_xor<1>(acc);
            acc = nan_first(acc);
            const int64_t row = base + r;
            // a score of -inf is what the score-array route gives a filtered row: that route reports such a row as
            // padding, and so does this one
            bool ok = row < n_rows && acc != neg_inf<double>();
            if constexpr (FILTER) ok = ok && source_ok(lds_allow, bt.sid[r]);
            if (lane == r) {
                cs = acc;
                cr = (uint32_t)row;
                cf = ok;
            }
        }
        top.offer_lanes(cf && top.admits(cs, cr), cs, cr);
    };
    Batch b0, b1;
    issue(base0, b0);
    int64_t base = base0;
    // every step issues the NEXT batch unconditionally (behind the last one it re-reads the wave's first rows) and only
    // then reduces the current one: dense_scan.hip says why
    for (;;) {
        int64_t next = base + step;
        bool last = next >= n_rows;
        if (last) next = base0;
        issue(next, b1);
        reduce(base, b0);
        if (last) break;
        base = next;
        next = base + step;
        last = next >= n_rows;
        if (last) next = base0;
        issue(next, b0);
        reduce(base, b1);
        if (last) break;
        base = next;
    }
    out_s[lane] = top.s;
    out_r[lane] = top.r;
}

bool dense_scan_f64_serves(const anrag_index *idx) {
    return idx->d_emb != nullptr && idx->dim % 4 == 0 && idx->dim >= 4 && idx->dim <= kF64ScanMaxDim;
}

// the fp64 list set (one: this route is not pipelined) and, behind it, the fused count of anrag_hybrid_search_f64
int ensure_dense_f64_lists(anrag_index *idx) {
    if (idx->d_blk_score_f64q) return ANRAG_OK;
    const int64_t bytes = (int64_t)kMaxScanLists * kListLen * sizeof(double) + 256;
    ANRAG_HIP(counted_malloc(reinterpret_cast<void **>(&idx->d_blk_score_f64q), (size_t)bytes));
    idx->hbm_bytes += bytes;
    return ANRAG_OK;
}

void free_dense_f64_lists(anrag_index *idx) {
    if (!idx->d_blk_score_f64q) return;
    (void)counted_free(idx->d_blk_score_f64q);
    idx->hbm_bytes -= (int64_t)kMaxScanLists * kListLen * sizeof(double) + 256;
    idx->d_blk_score_f64q = nullptr;
}

int ensure_query_f64(anrag_index *idx) {
    if (!idx->d_query_f64) ANRAG_HIP(counted_malloc(reinterpret_cast<void **>(&idx->d_query_f64), 65536 * sizeof(double)));
    return ANRAG_OK;
}

int32_t *dense_f64_count(const anrag_index *idx) {
    return reinterpret_cast<int32_t *>(idx->d_blk_score_f64q + (int64_t)kMaxScanLists * kListLen);
}

template <int CH>
static void launch_k1d(anrag_index *idx, hipStream_t st, int grid, const double *d_query, int32_t k,
                       const uint32_t *allow) {
    if (allow)
        dense_scan_f64_kernel<CH, true><<<grid, kScanThreads, 0, st>>>(idx->d_emb, d_query, idx->n_rows, idx->dim, k,
                                                                       idx->d_dense_src, allow, idx->d_blk_score_f64q,
                                                                       idx->d_blk_row_a);
    else
        dense_scan_f64_kernel<CH, false><<<grid, kScanThreads, 0, st>>>(idx->d_emb, d_query, idx->n_rows, idx->dim, k,
                                                                        nullptr, nullptr, idx->d_blk_score_f64q,
                                                                        idx->d_blk_row_a);
}

// K1D into the fp64 list set (scores) and set 0 of d_blk_row_a (rows): dense_scan_lists(idx) lists
int launch_dense_scan_f64(anrag_index *idx, hipStream_t st, const double *d_query, int32_t k,
                          const uint32_t *d_allow_bits) {
    ANRAG_REQUIRE(dense_scan_f64_serves(idx), "fp64 dense scan: dim %d is not served (dim %% 4 == 0, dim <= %d)", idx->dim,
                  kF64ScanMaxDim);
    ANRAG_REQUIRE(k >= 1 && k <= kListLen, "fp64 dense scan: 1 <= k <= %d (got %d)", kListLen, k);
    ANRAG_REQUIRE(idx->d_blk_score_f64q && idx->d_blk_row_a, "fp64 dense scan: no list buffers");
    const uint32_t *allow = idx->d_dense_src ? d_allow_bits : nullptr;
    const int grid = dense_scan_grid(idx);
    LaunchTimer t(idx, ANRAG_KERNEL_DENSE_SCAN, st);
    switch ((idx->dim + 255) / 256) {
        case 1: launch_k1d<1>(idx, st, grid, d_query, k, allow); break;
        case 2: launch_k1d<2>(idx, st, grid, d_query, k, allow); break;
        case 3: launch_k1d<3>(idx, st, grid, d_query, k, allow); break;
        case 4: launch_k1d<4>(idx, st, grid, d_query, k, allow); break;
        case 5: launch_k1d<5>(idx, st, grid, d_query, k, allow); break;
        case 6: launch_k1d<6>(idx, st, grid, d_query, k, allow); break;
        case 7: launch_k1d<7>(idx, st, grid, d_query, k, allow); break;
        case 8: launch_k1d<8>(idx, st, grid, d_query, k, allow); break;
        case 9: launch_k1d<9>(idx, st, grid, d_query, k, allow); break;
        case 10: launch_k1d<10>(idx, st, grid, d_query, k, allow); break;
        case 11: launch_k1d<11>(idx, st, grid, d_query, k, allow); break;
        default: launch_k1d<kF64ScanMaxCH>(idx, st, grid, d_query, k, allow); break;
    }
    ANRAG_HIP(hipGetLastError());
    return ANRAG_OK;
}

}  // namespace anrag
