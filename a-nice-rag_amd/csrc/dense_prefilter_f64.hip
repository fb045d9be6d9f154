// K1FD -- the shadow prefilter (dense_prefilter.hip) for ONE fp64 query: the same shadow scan and threshold kernel, run
// with q^ = fl32(q), then the survivors rescored with K1D's arithmetic (dense_scan_f64.hip) -- the same bits as K1D --
// into K1D's per-wave fp64 lists, which the fp64 tail (tail.hip) merges as it merges K1D's.
//
// The bound ("K1FD").  The scan's intervals [lo, hi] hold K1's fp32 score of q^ and, by the same
// derivation, the exact real product q^.e (K1F: m >= ||e - e~|| + gamma ||e~||; K1F8: m1 >= ||e - e~||, the query term is
// in the radius).  K1D's score s64 of the fp64 query q is D FMAs and a 6-step butterfly on exactly converted values:
//   |s64 - q^.e| <= |s64 - q.e| + |(q - q^).e| <= (gamma64 ||q|| + delta) ||e||,
// gamma64 = D 2^-53 / (1 - D 2^-53), delta = ||q - q^|| (each component difference is exact in fp64).  With Emax the
// largest ||e|| over the rows whose norm is finite and at most 2^60 (every other row has an infinite radius already),
//   w = (delta + gamma64 ||q||) Emax + D 2^-1000      (the last term: fp64 underflow of products and partial sums)
// evaluated on the host in fp64 with every rounding pushed upward, lo - w <= s64 <= hi + w for every row.
// Why T stays safe: k rows have s64 >= lo - w >= T - w, so K1D's k-th score is >= T - w and every row of K1D's top k
// (ties included) has hi + w >= s64 >= T - w.  The survivors are the rows with hi >= T - 2w (fp64, rounded toward -inf):
// a superset of K1D's top k, rescored with K1D's bits; the top k of a superset under (score desc, row asc) is the top k.
// Rows the source filter rejects carry hi = NaN and never pass; T = -inf lets every allowed row pass; a non-finite w
// lets every row with a non-NaN hi pass.
#include "common.hpp"
#include "wave_topk.hpp"
#include "dense_scan_common.hpp"

namespace anrag {

constexpr double kNormCapF64 = 0x1p60;  // dense_prefilter.hip's kRadiusCap: rows past it have an infinite radius
constexpr int kSweepF64 = 4;            // dwordx4 of hi per lane and step, as in dense_prefilter_rescore_kernel

// what lies behind the fp64 list set (ensure_dense_f64_lists leaves 256 bytes): the fused call's count, then these
struct PrefilterF64Tail {
    int32_t count, pad;
    unsigned long long emax_bits;  // Emax: a non-negative double, so its bits order like the value (atomicMax)
    unsigned long long survivors;  // cumulative rows rescored by this route
};
static PrefilterF64Tail *f64_tail(const anrag_index *idx) {
    return reinterpret_cast<PrefilterF64Tail *>(idx->d_blk_score_f64q + (int64_t)kMaxScanLists * kListLen);
}

// Emax: one wave per row, fp64 sums of exact squares (relative error < 2^-42 at D <= 2,048); rows whose norm is not
// finite or past the cap are skipped; the wave's maximum is widened by 2^-30 (sum, sqrt) and joins by atomicMax.
__global__ __launch_bounds__(kScanThreads) void dense_row_norm_max_kernel(const float *__restrict__ emb, int64_t n_rows,
                                                                         int32_t dim,
                                                                         unsigned long long *__restrict__ out_bits) {
    const int lane = lane_id();
    const int64_t total_waves = (int64_t)gridDim.x * kScanWaves;
    double mx = 0.0;
    for (int64_t row = (int64_t)blockIdx.x * kScanWaves + threadIdx.x / kWave; row < n_rows; row += total_waves) {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(emb + row * dim);
        double e2 = 0.0;
        for (int c = lane; c < dim / 4; c += kWave) {
            const f32x4 x = p[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) e2 += (double)x[j] * (double)x[j];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) e2 += __shfl_xor(e2, off, kWave);
        const double ne = __builtin_sqrt(e2);
        if (ne <= kNormCapF64 && ne > mx) mx = ne;  // NaN and +inf fail the first comparison
    }
    mx *= 1.0 + 0x1p-30;
    if (lane == 0 && mx > 0.0) atomicMax(out_bits, (unsigned long long)__double_as_longlong(mx));
}

// K1's grid.  The sweep over hi is dense_prefilter_rescore_kernel's (4 dwordx4 per lane and step, the buffer padded
// to 64 rows); each survivor is rescored by the WHOLE wave with K1D's mapping: lane l runs one chain over c = 4l .. 4l+3
// of every 256-float chunk, ascending, then the ^32 .. ^1 butterfly, then nan_first; -inf is not offered (K1D).
template <int CH>
__global__ __launch_bounds__(kScanThreads) void dense_prefilter_rescore_f64_kernel(
    const float *__restrict__ emb, const double *__restrict__ query, const float *__restrict__ hi,
    const float *__restrict__ thr, double w2, int64_t n_rows, int32_t k, double *__restrict__ blk_s,
    uint32_t *__restrict__ blk_r, unsigned long long *__restrict__ survivors) {
    constexpr int STEP = kWave * 4 * kSweepF64;
    constexpr int64_t ROW_F4 = CH * kWave;
    const int lane = lane_id();
    const int wave = threadIdx.x / kWave;
    double q[CH][4];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) q[c][j] = query[4 * (c * kWave + lane) + j];
    // T2 = T - 2w toward -inf: the difference is within 2^-53 of its rounded value d (exact when d is subnormal or 0),
    // and d - 2^-52 |d| is at most d's predecessor.  T is never +inf or NaN (lo = a - r is finite or -inf).
    double T2 = -__builtin_huge_val();
    if (__builtin_isfinite(w2)) {
        const double d = (double)*thr - w2;
        T2 = __builtin_fma(-__builtin_fabs(d), 0x1p-52, d);
    }
    WaveTopK<double> top;
    top.init(k);
    top.thr_s = neg_inf_opaque();  // signed scores: wave_topk.hpp
    const f32x4 *__restrict__ ev = reinterpret_cast<const f32x4 *>(emb);
    const f32x4 *__restrict__ hv = reinterpret_cast<const f32x4 *>(hi);
    const int64_t total_waves = (int64_t)gridDim.x * kScanWaves;
    const int64_t wave_global = (int64_t)blockIdx.x * kScanWaves + wave;
    unsigned long long count = 0;
    for (int64_t b = wave_global * STEP; b < n_rows; b += total_waves * STEP) {
        f32x4 h[kSweepF64];
#pragma unroll
        for (int u = 0; u < kSweepF64; ++u) {  // rows b + 4 (u 64 + lane) .. +3
            const int64_t r0 = b + 4 * (u * kWave + lane);
            h[u] = r0 < n_rows ? hv[r0 / 4] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < kSweepF64; ++u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t row = b + 4 * (u * kWave + lane) + j;
                unsigned long long mask = __ballot(row < n_rows && (double)h[u][j] >= T2);  // NaN: never
                if (mask == 0) continue;
                count += __builtin_popcountll(mask);
                while (mask) {
                    const int l = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const int64_t mine = b + 4 * (u * kWave + l) + j;  // < n_rows: the ballot checked it
                    const f32x4 *p = ev + mine * ROW_F4 + lane;
                    f32x4 v[CH];
#pragma unroll
                    for (int c = 0; c < CH; ++c) v[c] = p[c * kWave];
                    double acc = 0.0;
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        acc = __builtin_fma((double)v[c].x, q[c][0], acc);
                        acc = __builtin_fma((double)v[c].y, q[c][1], acc);
                        acc = __builtin_fma((double)v[c].z, q[c][2], acc);
                        acc = __builtin_fma((double)v[c].w, q[c][3], acc);
                    }
                    acc += lane_xor<32>(acc);
                    acc += lane_xor<16>(acc);
                    acc += lane_xor<8>(acc);
                    acc += lane_xor<4>(acc);
                    acc += lane_xor<2>(acc);
                    acc += lane_xor<1>(acc);
                    const double s = read_lane(nan_first(acc), 0);  // every lane holds the same bits
                    const uint32_t r32 = (uint32_t)mine;
                    if (s != neg_inf<double>() && top.admits(s, r32)) top.insert(s, r32);
                }
            }
        }
    }
    blk_s[wave_global * kListLen + lane] = top.s;
    blk_r[wave_global * kListLen + lane] = top.r;
    if (lane == 0 && count) atomicAdd(survivors, count);
}

// ---------------------------------------------------------------- host
// Emax of the loaded corpus, once per dense load (free_dense clears the flag): the first fp64 prefilter query pays for
// it, with one host wait.
int ensure_dense_prefilter_f64(anrag_index *idx, hipStream_t st) {
    if (idx->f64_pf_ready) return ANRAG_OK;
    ANRAG_REQUIRE(idx->d_blk_score_f64q != nullptr && idx->d_emb != nullptr && idx->dim % 256 == 0,
                  "fp64 prefilter: no list buffers, or dim %d is no multiple of 256", idx->dim);
    PrefilterF64Tail *t = f64_tail(idx);
    ANRAG_HIP(hipMemsetAsync(&t->emax_bits, 0, 2 * sizeof(unsigned long long), st));
    const int64_t need = (idx->n_rows + kScanWaves - 1) / kScanWaves;
    const int64_t cap = (int64_t)idx->n_cus * 8;
    dense_row_norm_max_kernel<<<(unsigned)(need < cap ? need : cap), kScanThreads, 0, st>>>(idx->d_emb, idx->n_rows,
                                                                                           idx->dim, &t->emax_bits);
    ANRAG_HIP(hipGetLastError());
    ANRAG_HIP(hipMemcpyAsync(&idx->f64_pf_emax, &t->emax_bits, sizeof(double), hipMemcpyDeviceToHost, st));
    ANRAG_HIP(hipStreamSynchronize(st));
    idx->f64_pf_queries = 0;
    idx->f64_pf_ready = true;
    return ANRAG_OK;
}

int dense_prefilter_f64_survivors(anrag_index *idx, int64_t *out) {
    unsigned long long s = 0;
    if (idx->f64_pf_ready && idx->d_blk_score_f64q)
        ANRAG_HIP(hipMemcpy(&s, &f64_tail(idx)->survivors, sizeof(s), hipMemcpyDeviceToHost));
    *out = (int64_t)s;
    return ANRAG_OK;
}

// the survivors of list set 0's hi and T (the shadow scan and the threshold kernel ran with q^ on this stream), rescored
// with d_query into the fp64 list set and set 0 of d_blk_row_a: dense_scan_lists(idx) lists, as K1D leaves them
int launch_dense_prefilter_rescore_f64(anrag_index *idx, hipStream_t st, const double *d_query, double w, int32_t k) {
    ANRAG_REQUIRE(idx->pf_on && idx->f64_pf_ready && idx->dim % 256 == 0 && idx->dim <= 2048,
                  "fp64 prefilter: not ready for dim %d", idx->dim);
    ANRAG_REQUIRE(k >= 1 && k <= kListLen, "fp64 prefilter: 1 <= k <= %d (got %d)", kListLen, k);
    const int grid = dense_scan_grid(idx);
    const double w2 = 2.0 * w;  // exact, or +inf: every row with a non-NaN hi
    unsigned long long *surv = &f64_tail(idx)->survivors;
#define ANRAG_RESCORE_F64(CH)                                                                                   \
    dense_prefilter_rescore_f64_kernel<CH><<<grid, kScanThreads, 0, st>>>(idx->d_emb, d_query, idx->d_pf_hi,   \
                                                                          idx->d_pf_thr, w2, idx->n_rows, k,   \
                                                                          idx->d_blk_score_f64q, idx->d_blk_row_a, surv)
    switch (idx->dim / 256) {
        case 1: ANRAG_RESCORE_F64(1); break;
        case 2: ANRAG_RESCORE_F64(2); break;
        case 3: ANRAG_RESCORE_F64(3); break;
        case 4: ANRAG_RESCORE_F64(4); break;
        case 6: ANRAG_RESCORE_F64(6); break;
        case 8: ANRAG_RESCORE_F64(8); break;
        default: ANRAG_REQUIRE(false, "fp64 prefilter: no kernel for dim %d", idx->dim);
    }
#undef ANRAG_RESCORE_F64
    ANRAG_HIP(hipGetLastError());
    idx->f64_pf_queries += 1;
    return ANRAG_OK;
}

}  // namespace anrag
