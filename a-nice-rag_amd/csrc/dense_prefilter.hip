// K1F -- the dense top-k leg read through an fp16 shadow of the corpus, the survivors rescored with K1's own arithmetic.
//
// K1 (dense_scan.hip) streams N*D*4 bytes per query at ~90 % of HBM peak: the only lever left on it is the byte count.
// K1F answers the same top-k from N*D*2 bytes plus a few survivors:
//   1. scan  (dense_prefilter_scan_kernel): every row's approximate score a = q . fp16(e) (fp32 FMAs on exactly converted
//      fp16 values) and, from a per-row error radius m (load time) and ||q|| (in the kernel), an interval [lo, hi] that
//      provably holds K1's fp32 score s of the row.  hi is stored per row; each wave keeps its top-k of lo.
//   2. threshold  (dense_prefilter_threshold_kernel): T = the k-th largest lo over the allowed rows (-inf when fewer).
//   3. rescore  (dense_prefilter_rescore_kernel): rows with hi >= T are rescored from the fp32 rows with K1's lane mapping,
//      dot4 chain, group_sum and nan_first -- the same bits as K1 -- and leave K1's per-wave sorted lists, so the tail
//      kernel and the deferred merge see exactly what K1 would have left.
//
// The bound ("K1F").  D = dim, u = 2^-24, gamma = D u / (1 - D u), e~ = fp16(e) (round to nearest even):
//   |s - q.e|    <= gamma ||q|| ||e||          (K1: D products summed by FMA chains and a DPP tree, any order)
//   |a - q.e~|   <= gamma ||q|| ||e~||         (this scan: the same, on e~)
//   |q.e~ - q.e| <= ||q|| ||e - e~||           (Cauchy-Schwarz)
// so lo = a - ||q|| m <= s <= a + ||q|| m = hi with m = ||e - e~|| + gamma (||e|| + ||e~||).  m is computed in fp64 at load
// and rounded up to fp32; ||q|| likewise in the scan; lo / hi are evaluated in fp32 with every rounding pushed outward,
// widened by eta = D 2^-120 (subnormal products and partial sums carry an absolute error, which the relative gamma
// misses).  No partial sum can overflow: rows with ||e|| > 2^60 and queries with ||q|| > 2^60 get an
// infinite radius.  A non-finite m, a or ||q|| gives [-inf, +inf]: such a row always survives (a NaN or inf row, an fp16
// overflow past 65504), and a non-finite query rescores every row -- correct, and as slow as that sounds.
//
// Why T is safe: k rows have s >= lo >= T, so K1's k-th score is >= T and every row of K1's top k (ties included) has
// hi >= s >= T.  The survivors are a superset of K1's top k with K1's exact scores, and a top k under the lists' total
// order (score desc, row asc) of a superset of the top k is the top k.  Rows the source filter rejects store hi = NaN
// (never >= T) and offer no lo.
#include "common.hpp"
#include "wave_topk.hpp"
#include "dense_scan_common.hpp"

namespace anrag {

struct PrefilterQueries {
    const float *q[kScanGroupMax];
    float *hi[kScanGroupMax];        // per row: upper bound of K1's score (NaN: filtered out)
    float *blk_s[kScanGroupMax];     // scan: per-wave lists of lo; rescore: K1's per-wave lists
    uint32_t *blk_r[kScanGroupMax];
    float *thr[kScanGroupMax];       // T
    int32_t n;
};

constexpr double kRadiusCap = 0x1p60;  // ||e|| or ||q|| past this: infinite radius (no partial sum can overflow)

__device__ __forceinline__ float prefilter_eta(int32_t dim) { return (float)dim * 0x1p-120f; }

// [lo, hi] around K1's score of a row whose approximate score is a (see the header), in fp32 with every rounding
// pushed outward: r = fl(qn m + eta) is within 2^-24 r of its exact value (r >= eta is normal), r (1 + 2^-22) is above
// it; a +- r_up is within 2^-24 of its rounded value (an exact sum that is subnormal or 0 is rounded exactly), and one
// more factor (1 + 2^-22) away from zero covers that.  Nothing overflows: |a|, r < 2^122.
__device__ __forceinline__ void row_bounds(float a, float m, float qn, float eta, float &lo, float &hi) {
    if (!(__builtin_isfinite(a) && __builtin_isfinite(m) && __builtin_isfinite(qn))) {
        lo = -__builtin_huge_valf();
        hi = __builtin_huge_valf();
        return;
    }
    float r = __builtin_fmaf(qn, m, eta);
    r = __builtin_fmaf(r, 0x1p-22f, r);
    const float h = a + r, l = a - r;
    hi = __builtin_fmaf(__builtin_fabsf(h), 0x1p-22f, h);
    lo = __builtin_fmaf(-__builtin_fabsf(l), 0x1p-22f, l);
}

// ---------------------------------------------------------------- load time: fp16 image + per-row radius m
__global__ __launch_bounds__(kScanThreads) void dense_prefilter_convert_kernel(
    const float *__restrict__ emb, int64_t n_rows, int32_t dim, _Float16 *__restrict__ img, float *__restrict__ m_out) {
    const int lane = lane_id();
    const int64_t total_waves = (int64_t)gridDim.x * kScanWaves;
    const double u = 0x1p-24, gamma = dim * u / (1.0 - dim * u);
    for (int64_t row = (int64_t)blockIdx.x * kScanWaves + threadIdx.x / kWave; row < n_rows; row += total_waves) {
        const float *p = emb + row * dim;
        _Float16 *h = img + row * dim;
        double d2 = 0.0, e2 = 0.0, h2 = 0.0;
        for (int c = lane; c < dim; c += kWave) {
            const float e = p[c];
            const _Float16 t = (_Float16)e;  // v_cvt_f16_f32: round to nearest even
            h[c] = t;
            const double ed = e, hd = (double)(float)t;
            d2 += (ed - hd) * (ed - hd);
            e2 += ed * ed;
            h2 += hd * hd;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            d2 += __shfl_xor(d2, off, kWave);
            e2 += __shfl_xor(e2, off, kWave);
            h2 += __shfl_xor(h2, off, kWave);
        }
        if (lane == 0) {
            const double ne = __builtin_sqrt(e2), nh = __builtin_sqrt(h2);
            // fp64 sums of <= 65536 squares: relative error < 2^-36; widened by 2^-30, then rounded up to fp32
            double m = (__builtin_sqrt(d2) + gamma * (ne + nh)) * (1.0 + 0x1p-30);
            if (!(ne <= kRadiusCap) || !(nh <= kRadiusCap) || !__builtin_isfinite(m)) m = __builtin_huge_val();
            m_out[row] = __double2float_ru(m);
        }
    }
}

// ---------------------------------------------------------------- 1. the approximate scan
// G, CH, R: the byte geometry of K1 for a row of 2*dim bytes (scan_dispatch(dim / 2)): a lane's dwordx4 holds 8 fp16
// values, elements 8 (c G + sub) .. +7 of the row.  Rows: a CONTIGUOUS block per wave (K1's SCORES form), so that hi
// leaves 64 rows at a time as one 256-byte store (stores count in vmcnt: one per row would break the counted waits).
template <int G, int CH, int R, bool FILTER>
__global__ __launch_bounds__(kScanThreads) void dense_prefilter_scan_kernel(
    const f32x4 *__restrict__ img, const float *__restrict__ mrow, PrefilterQueries Q, int64_t n_rows, int32_t dim,
    int32_t k, const uint16_t *__restrict__ src, const uint32_t *__restrict__ allow_bits) {
    constexpr int GROUPS = kWave / G;
    constexpr int RW = GROUPS * R;
    constexpr int WAVES = kScanWaves;
    __shared__ uint32_t lds_allow[FILTER ? 2048 : 1];

    const int lane = lane_id();
    const int wave = threadIdx.x / kWave;
    const int sub = lane % G, grp = lane / G;
    const bool leader = sub == G - 1;
    if constexpr (FILTER) {
        for (int i = threadIdx.x; i < 2048; i += kScanThreads) lds_allow[i] = allow_bits[i];
        __syncthreads();
    }
    const int64_t row_f4 = dim / 8;
    const float eta = prefilter_eta(dim);
    float q[CH][8];
    float qn = 0.f;
    WaveTopK<float> top;
    struct Batch {
        f32x4 v[R][CH];
        float m[R];
        uint32_t sid[R];
    };
    auto next_query = [&](int32_t qi) {
        const f32x4 *__restrict__ query = reinterpret_cast<const f32x4 *>(Q.q[qi]);
        double ss = 0.0;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const f32x4 a = query[2 * (c * G + sub)], b = query[2 * (c * G + sub) + 1];
            q[c][0] = a.x; q[c][1] = a.y; q[c][2] = a.z; q[c][3] = a.w;
            q[c][4] = b.x; q[c][5] = b.y; q[c][6] = b.z; q[c][7] = b.w;
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += (double)q[c][j] * (double)q[c][j];
        }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) ss += __shfl_xor(ss, off, kWave);
        const double nq = __builtin_sqrt(ss) * (1.0 + 0x1p-30);
        qn = nq <= kRadiusCap ? __double2float_ru(nq) : __builtin_huge_valf();  // NaN / inf / huge: +inf
        top.init(k);
    };
    const int64_t total_waves = (int64_t)gridDim.x * WAVES;
    const int64_t wave_global = (int64_t)blockIdx.x * WAVES + wave;
    const int64_t rows_per_wave = ((n_rows + total_waves - 1) / total_waves + RW - 1) / RW * RW;
    const int64_t base0 = wave_global * rows_per_wave;
    const int64_t lim = base0 + rows_per_wave < n_rows ? base0 + rows_per_wave : n_rows;
    float hb = 0.f;  // lane j <- hi of row hbase + j
    int64_t hbase = base0;
    int32_t qi = 0;
    auto flush = [&](int32_t qe) {
        Q.blk_s[qe][(blockIdx.x * WAVES + wave) * kListLen + lane] = top.s;
        Q.blk_r[qe][(blockIdx.x * WAVES + wave) * kListLen + lane] = top.r;
        if (hbase + lane < lim) Q.hi[qe][hbase + lane] = hb;
        hbase = base0;
    };
    auto issue = [&](int64_t base, Batch &bt) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = base + r * GROUPS + grp;
            const int64_t rc = row < n_rows ? row : n_rows - 1;
            if constexpr (FILTER) bt.sid[r] = src[rc];
            bt.m[r] = mrow[rc];
            const f32x4 *p = img + rc * row_f4 + sub;
#pragma unroll
            for (int c = 0; c < CH; ++c) bt.v[r][c] = __builtin_nontemporal_load(p + c * G);
        }
    };
    auto finish_row = [&](int64_t row, float acc, float m, uint32_t sid) {
        acc = group_sum<G>(acc);
        bool ok = row < lim;
        if constexpr (FILTER) ok = ok && source_ok(lds_allow, sid);
        float lo, hi;
        row_bounds(acc, m, qn, eta, lo, hi);
        const float hv = ok ? hi : __builtin_nanf("");
        const int64_t row0 = row - grp;  // the row of lane group 0: wave-uniform
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const float sg = read_lane(hv, g * G + G - 1);
            const int64_t rg = row0 + g;
            if (rg < lim) {
                const int slot = (int)(rg - hbase);
                hb = lane == slot ? sg : hb;
                if (slot == kWave - 1) {
                    Q.hi[qi][hbase + lane] = hb;
                    hbase += kWave;
                }
            }
        }
        const uint32_t r32 = (uint32_t)row;
        top.offer_lanes(leader && ok && top.admits(lo, r32), lo, r32);
    };
    auto reduce = [&](int64_t base, const Batch &bt) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const uint32_t w[4] = {__float_as_uint(bt.v[r][c].x), __float_as_uint(bt.v[r][c].y),
                                       __float_as_uint(bt.v[r][c].z), __float_as_uint(bt.v[r][c].w)};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const _Float16 h0 = __builtin_bit_cast(_Float16, (uint16_t)(w[j] & 0xFFFFu));
                    const _Float16 h1 = __builtin_bit_cast(_Float16, (uint16_t)(w[j] >> 16));
                    acc = __builtin_fmaf((float)h0, q[c][2 * j], acc);
                    acc = __builtin_fmaf((float)h1, q[c][2 * j + 1], acc);
                }
            }
            finish_row(base + r * GROUPS + grp, acc, bt.m[r], bt.sid[r]);
        }
    };
    if (base0 >= n_rows) {  // a wave without rows (tiny corpora): empty lists
        top.init(1);
        for (int32_t qe = 0; qe < Q.n; ++qe) {
            Q.blk_s[qe][(blockIdx.x * WAVES + wave) * kListLen + lane] = top.s;
            Q.blk_r[qe][(blockIdx.x * WAVES + wave) * kListLen + lane] = top.r;
        }
        return;
    }
    next_query(0);
    Batch b0, b1;
    issue(base0, b0);
    int64_t base = base0;
    // K1's loop: the next batch is issued unconditionally before the current one is reduced (dense_scan.hip)
    for (;;) {
        int32_t nq = qi;
        int64_t next = base + RW;
        if (next >= lim) {
            next = base0;
            ++nq;
        }
        issue(next, b1);
        reduce(base, b0);
        if (nq != qi) {
            flush(qi);
            if (nq >= Q.n) break;
            qi = nq;
            next_query(qi);
        }
        base = next;
        next = base + RW;
        if (next >= lim) {
            next = base0;
            ++nq;
        }
        issue(next, b0);
        reduce(base, b1);
        if (nq != qi) {
            flush(qi);
            if (nq >= Q.n) break;
            qi = nq;
            next_query(qi);
        }
        base = next;
    }
}

// ---------------------------------------------------------------- K1F8: the same scan over an int8 shadow
// DESIGN.md §3, "K1F8".  Row e: scale s_e and u = rint(e / s_e) in [-127, 127], e~ = s_e u (exact in fp64).  Query q
// (per query, in the wave prologue): s_q, v likewise, q~ = s_q v.  The scan computes the integer S = v . u exactly
// (|S| <= 2048 127^2 < 2^25, v_dot4_i32_i8 and an integer DPP tree) and a = fl(fl(S) fl(s_q s_e)), |a - q~.e~| <=
// 2^-22 |a| + 2^-124 (three roundings of <= u each; the absolute part: subnormal s_q s_e or a).  With
//   |s - q.e| <= gamma ||q|| ||e||,   q.e - q~.e~ = q.(e - e~) + (q - q~).e~
// K1's score s lies in a +- (||q|| m1 + ||q - q~|| m2 + 2^-22 |a| + eta), m1 = ||e - e~|| + gamma ||e||, m2 = ||e~||.
// m1, m2 (load time) and ||q||, ||q - q~|| (prologue) are fp64 sums rounded up to fp32; every fp32 step below is
// pushed outward.  Non-finite and past-the-cap rows / queries get [-inf, +inf], as in K1F.
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void row_bounds_i8(float a, float m1, float m2, float qn, float eqn, float eta, float &lo,
                                              float &hi) {
    if (!(__builtin_isfinite(a) && __builtin_isfinite(m1) && __builtin_isfinite(m2) && __builtin_isfinite(qn) &&
          __builtin_isfinite(eqn))) {
        lo = -__builtin_huge_valf();
        hi = __builtin_huge_valf();
        return;
    }
    // three FMAs of non-negative terms (>= eta: normal), each within 2^-24 of its exact value: the sum is below
    // r (1 - 2^-24)^-3; one more rounding of r (1 + 2^-21) stays above that.  Nothing overflows: every term < 2^122.
    float r = __builtin_fmaf(qn, m1, eta);
    r = __builtin_fmaf(eqn, m2, r);
    r = __builtin_fmaf(__builtin_fabsf(a), 0x1p-22f, r);
    r = __builtin_fmaf(r, 0x1p-21f, r);
    const float h = a + r, l = a - r;
    hi = __builtin_fmaf(__builtin_fabsf(h), 0x1p-22f, h);
    lo = __builtin_fmaf(-__builtin_fabsf(l), 0x1p-22f, l);
}

// group_sum<G> of integers: the same DPP tree, exact
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int32_t dpp_add_i32(int32_t v) {
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
}
template <int G>
__device__ __forceinline__ int32_t group_sum_i32(int32_t v) {
    if constexpr (G >= 2) v = dpp_add_i32<0xB1, 0xF>(v);
    if constexpr (G >= 4) v = dpp_add_i32<0x4E, 0xF>(v);
    if constexpr (G >= 8) v = dpp_add_i32<0x141, 0xF>(v);
    if constexpr (G >= 16) v = dpp_add_i32<0x140, 0xF>(v);
    if constexpr (G >= 32) v = dpp_add_i32<0x142, 0xA>(v);
    if constexpr (G >= 64) v = dpp_add_i32<0x143, 0xC>(v);
    return v;
}

// x -> the int8 step count of scale s (NaN -> -127: such a query or row has an infinite radius anyway)
__device__ __forceinline__ float quantise(float x, float inv_s) {
    return __builtin_fminf(__builtin_fmaxf(__builtin_rintf(x * inv_s), -127.f), 127.f);
}
__device__ __forceinline__ uint32_t pack_i8(float y, int j) { return ((uint32_t)(int32_t)y & 0xFFu) << (8 * j); }

// scale of a row or query: max|x| / 127 (any positive finite scale is correct: the radii are measured from the codes
// actually stored); a zero, subnormal-to-nothing or non-finite maximum takes 1
__device__ __forceinline__ float i8_scale(float mx) {
    const float s = mx / 127.f;
    return (s > 0.f && __builtin_isfinite(s)) ? s : 1.f;
}

// load time: one wave per row, 4 values per lane and step (dim % 256 == 0).  meta[row] = {s_e, m1, m2, 0}.
__global__ __launch_bounds__(kScanThreads) void dense_prefilter_i8_convert_kernel(
    const float *__restrict__ emb, int64_t n_rows, int32_t dim, uint32_t *__restrict__ img, f32x4 *__restrict__ meta) {
    const int lane = lane_id();
    const int64_t total_waves = (int64_t)gridDim.x * kScanWaves;
    const double u = 0x1p-24, gamma = dim * u / (1.0 - dim * u);
    for (int64_t row = (int64_t)blockIdx.x * kScanWaves + threadIdx.x / kWave; row < n_rows; row += total_waves) {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(emb + row * dim);
        uint32_t *w = img + row * dim / 4;
        float mx = 0.f;
        double e2 = 0.0;
        for (int c = lane; c < dim / 4; c += kWave) {
            const f32x4 x = p[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mx = __builtin_fmaxf(mx, __builtin_fabsf(x[j]));
                e2 += (double)x[j] * (double)x[j];
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, off, kWave));
            e2 += __shfl_xor(e2, off, kWave);
        }
        const float s = i8_scale(mx), inv = 1.f / s;
        double d2 = 0.0, t2 = 0.0;
        for (int c = lane; c < dim / 4; c += kWave) {
            const f32x4 x = p[c];
            uint32_t b = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float y = quantise(x[j], inv);
                const double t = (double)s * (double)y, d = (double)x[j] - t;  // s y: exact in fp64
                d2 += d * d;
                t2 += t * t;
                b |= pack_i8(y, j);
            }
            w[c] = b;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            d2 += __shfl_xor(d2, off, kWave);
            t2 += __shfl_xor(t2, off, kWave);
        }
        if (lane == 0) {
            const double ne = __builtin_sqrt(e2), nt = __builtin_sqrt(t2);
            // fp64 sums of <= 2048 squares: relative error < 2^-40; widened by 2^-30, then rounded up to fp32
            double m1 = (__builtin_sqrt(d2) + gamma * ne) * (1.0 + 0x1p-30), m2 = nt * (1.0 + 0x1p-30);
            if (!(ne <= kRadiusCap) || !(nt <= kRadiusCap) || !__builtin_isfinite(m1)) m1 = __builtin_huge_val();
            meta[row] = f32x4{s, __double2float_ru(m1), __double2float_ru(m2), 0.f};
        }
    }
}

// G, CH, R: the byte geometry of K1 for a row of dim bytes (scan_dispatch(dim / 4)): a lane's dwordx4 holds 16 codes,
// elements 16 (c G + sub) .. +15 of the row.  Rows: a contiguous block per wave, as in the fp16 scan.  Per batch of RW
// rows, lane j < RW also loads the metadata (and source id) of row base + j -- one coalesced load, issued with the
// batch so that every batch issues the same loads -- and the RW integer sums are gathered to those lanes: bounds, hi
// and the top-k offer are then computed once per batch for all its rows.
// amdgpu_waves_per_eu(4): <= 128 VGPRs, so that K3's waves fit beside a scan wave on every SIMD (bm25.hip); the
// unconstrained schedule of the 768-d shape took 133-136.
//
// QP, queries per pass ("K1F8 pair pass").  QP == 1: one query per walk of the wave's row block, its codes
// in registers (qv).  QP == 2: queries qi and qi + 1 share one walk -- every batch is loaded once and reduced twice, so
// a pair reads the image once.  The wave waits out its loads for more than half of an iteration, which is where the
// second query's dot products, bounds and offer go.  A second qv does not fit under 128 VGPRs: both queries' codes
// live in LDS instead, each lane's own CH dwordx4 per query (a register file extension: written in next_query, read
// back by the same lane with one ds_read_b128 per chunk and batch -- no cross-lane traffic, no barrier; LDS reads
// count in lgkmcnt, so the counted vmcnt waits on the batches stay what they were).  Per query nothing changes: the same
// integer chain, gather, bounds, hi placement and offers in the same order, hence the same bits everywhere.
template <int G, int CH, int R, bool FILTER, int QP>
__device__ __forceinline__ void i8_scan_body(const i32x4 *__restrict__ img, const f32x4 *__restrict__ meta,
                                             const PrefilterQueries Q, int64_t n_rows, int32_t dim, int32_t k,
                                             const uint16_t *__restrict__ src, const uint32_t *__restrict__ allow_bits) {
    constexpr int GROUPS = kWave / G;
    constexpr int RW = GROUPS * R;
    static_assert(RW <= kWave, "a batch's rows fit the lanes of one wave");
    static_assert(QP == 1 || QP == 2, "one or two queries per pass");
    constexpr int WAVES = kScanWaves;
    __shared__ uint32_t lds_allow[FILTER ? 2048 : 1];
    __shared__ i32x4 lds_q[QP == 2 ? WAVES * QP * CH * kWave : 1];  // [wave][query][chunk][lane]

    const int lane = lane_id();
    // QP == 2: the wave index as a scalar, so that the walk (base, lim, hbase, the query index and with it the loads of
    // the queries' pointers) stays in SGPRs and s_loads; QP == 1 keeps the code it had
    const int wave = QP == 2 ? __builtin_amdgcn_readfirstlane(threadIdx.x / kWave) : threadIdx.x / kWave;
    const int sub = lane % G, grp = lane / G;
    if constexpr (FILTER) {
        for (int i = threadIdx.x; i < 2048; i += kScanThreads) lds_allow[i] = allow_bits[i];
        __syncthreads();
    }
    const int64_t row_i4 = dim / 16;
    const float eta = prefilter_eta(dim);
    int32_t qv[QP == 1 ? CH : 1][4];  // QP == 1: this lane's query codes, 4 per dword (the image's byte order)
    float sq[QP], qn[QP], eqn[QP];
    WaveTopK<float> top[QP];
    struct Batch {
        i32x4 v[R][CH];
        f32x4 m;  // {s_e, m1, m2, -} of row base + lane
        uint32_t sid;
    };
    auto next_query = [&](int32_t qi) {
#pragma unroll
        for (int p = 0; p < QP; ++p) {
            const f32x4 *__restrict__ query = reinterpret_cast<const f32x4 *>(Q.q[qi + p]);
            double ss = 0.0;
            float mx = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                // one chunk (16 floats) in registers at a time, beside the batch in flight; the second pass reads the
                // slice again (L2 hits) -- the fences keep the compiler from merging or hoisting the loads
                asm volatile("" ::: "memory");
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f32x4 x = query[4 * (c * G + sub) + t];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        ss += (double)x[j] * (double)x[j];
                        mx = __builtin_fmaxf(mx, __builtin_fabsf(x[j]));
                    }
                }
            }
#pragma unroll
            for (int off = 1; off < G; off <<= 1) {
                ss += __shfl_xor(ss, off, kWave);
                mx = __builtin_fmaxf(mx, __shfl_xor(mx, off, kWave));
            }
            sq[p] = i8_scale(mx);
            const float inv = 1.f / sq[p];
            double d2 = 0.0;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                asm volatile("" ::: "memory");
                i32x4 codes;  // QP == 2: this lane's chunk, on its way to LDS
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f32x4 x = query[4 * (c * G + sub) + t];
                    uint32_t b = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float y = quantise(x[j], inv);
                        const double d = (double)x[j] - (double)sq[p] * (double)y;
                        d2 += d * d;
                        b |= pack_i8(y, j);
                    }
                    if constexpr (QP == 1) qv[c][t] = (int32_t)b;
                    else codes[t] = (int32_t)b;
                }
                if constexpr (QP == 2) lds_q[((wave * QP + p) * CH + c) * kWave + lane] = codes;
            }
#pragma unroll
            for (int off = 1; off < G; off <<= 1) d2 += __shfl_xor(d2, off, kWave);
            const double nq = __builtin_sqrt(ss) * (1.0 + 0x1p-30), ne = __builtin_sqrt(d2) * (1.0 + 0x1p-30);
            qn[p] = nq <= kRadiusCap ? __double2float_ru(nq) : __builtin_huge_valf();  // NaN / inf / huge: +inf
            eqn[p] = ne <= kRadiusCap ? __double2float_ru(ne) : __builtin_huge_valf();
            sq[p] = read_lane(sq[p], 0);  // equal in every lane: held in SGPRs
            qn[p] = read_lane(qn[p], 0);
            eqn[p] = read_lane(eqn[p], 0);
            top[p].init(k);
        }
    };
    const int64_t total_waves = (int64_t)gridDim.x * WAVES;
    const int64_t wave_global = (int64_t)blockIdx.x * WAVES + wave;
    const int64_t rows_per_wave = ((n_rows + total_waves - 1) / total_waves + RW - 1) / RW * RW;
    const int64_t base0 = wave_global * rows_per_wave;
    const int64_t lim = base0 + rows_per_wave < n_rows ? base0 + rows_per_wave : n_rows;
    float hb[QP];  // lane j <- hi of row hbase + j (both queries of a pair are at the same row)
#pragma unroll
    for (int p = 0; p < QP; ++p) {
        sq[p] = 1.f;
        qn[p] = eqn[p] = hb[p] = 0.f;
    }
    int64_t hbase = base0;
    int32_t qi = 0;
    auto flush = [&](int32_t qe) {
#pragma unroll
        for (int p = 0; p < QP; ++p) {
            Q.blk_s[qe + p][(blockIdx.x * WAVES + wave) * kListLen + lane] = top[p].s;
            Q.blk_r[qe + p][(blockIdx.x * WAVES + wave) * kListLen + lane] = top[p].r;
            if (hbase + lane < lim) Q.hi[qe + p][hbase + lane] = hb[p];
        }
        hbase = base0;
    };
    // addresses: a wave-uniform 64-bit base and 32-bit lane offsets (rows past the end clamp to the last row)
    auto issue = [&](int64_t base, Batch &bt) {
        const int64_t left = n_rows - 1 - base;  // >= 0: base < n_rows
        const int32_t last = left < RW ? (int32_t)left : RW;
        const i32x4 *pb = img + base * row_i4;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int32_t o = r * GROUPS + grp;
            const i32x4 *p = pb + (int32_t)((o < last ? o : last) * (int32_t)row_i4 + sub);
#pragma unroll
            for (int c = 0; c < CH; ++c) bt.v[r][c] = __builtin_nontemporal_load(p + c * G);
        }
        const int32_t mo = lane < RW ? lane : RW - 1;
        const int32_t mc = mo < last ? mo : last;
        const float *pm = reinterpret_cast<const float *>(meta + base) + 4 * mc;  // one dwordx3: the fourth is padding
        bt.m = f32x4{pm[0], pm[1], pm[2], 0.f};
        if constexpr (FILTER) bt.sid = src[base + mc];
    };
    auto reduce = [&](int64_t base, const Batch &bt) {
        int32_t sum[QP];  // lane j < RW: v . u of row base + j
        if constexpr (QP == 1) {
            sum[0] = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                int32_t acc = 0;
#pragma unroll
                for (int c = 0; c < CH; ++c)
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_sdot4(bt.v[r][c][t], qv[c][t], acc, false);
                acc = group_sum_i32<G>(acc);
#pragma unroll
                for (int g = 0; g < GROUPS; ++g) {
                    const int32_t sg = (int32_t)read_lane((uint32_t)acc, g * G + G - 1);
                    sum[0] = lane == r * GROUPS + g ? sg : sum[0];
                }
            }
        } else {
            // a chunk of both queries' codes from LDS, then every row of the batch against it: the same chain per
            // (query, row) as above, c ascending, t ascending
            int32_t acc[QP][R];
#pragma unroll
            for (int p = 0; p < QP; ++p)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[p][r] = 0;
            // the codes of chunk c + 1 are on their way from LDS while chunk c is multiplied (one wave per SIMD: nothing
            // else would cover a ds_read's latency)
            i32x4 qc[2][QP];
#pragma unroll
            for (int p = 0; p < QP; ++p) qc[0][p] = lds_q[((wave * QP + p) * CH + 0) * kWave + lane];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                if (c + 1 < CH) {
#pragma unroll
                    for (int p = 0; p < QP; ++p) qc[(c + 1) & 1][p] = lds_q[((wave * QP + p) * CH + c + 1) * kWave + lane];
                }
#pragma unroll
                for (int p = 0; p < QP; ++p)
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            acc[p][r] = __builtin_amdgcn_sdot4(bt.v[r][c][t], qc[c & 1][p][t], acc[p][r], false);
            }
#pragma unroll
            for (int p = 0; p < QP; ++p) {
                sum[p] = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int32_t a = group_sum_i32<G>(acc[p][r]);
#pragma unroll
                    for (int g = 0; g < GROUPS; ++g) {
                        const int32_t sg = (int32_t)read_lane((uint32_t)a, g * G + G - 1);
                        sum[p] = lane == r * GROUPS + g ? sg : sum[p];
                    }
                }
            }
        }
        const int64_t row = base + lane;
        bool ok = lane < RW && row < lim;
        if constexpr (FILTER) ok = ok && source_ok(lds_allow, bt.sid);
        // rows base .. base + RW - 1 take slots off .. off + RW - 1 of the 64-row store, the overflow the next one's
#pragma unroll
        for (int p = 0; p < QP; ++p) {
            const float a = (float)sum[p] * (sq[p] * bt.m.x);
            float lo, hi;
            row_bounds_i8(a, bt.m.y, bt.m.z, qn[p], eqn[p], eta, lo, hi);
            const float hv = ok ? hi : __builtin_nanf("");
            const int off = (int)(base - hbase);
            const float sh = __shfl(hv, (lane - off) & (kWave - 1), kWave);
            if (lane >= off && lane < off + RW) hb[p] = sh;
            if (off + RW >= kWave) {
                if (hbase + lane < lim) Q.hi[qi + p][hbase + lane] = hb[p];
                if (p == QP - 1) hbase += kWave;  // (both queries of a pair store at the same batch)
                if (lane < off + RW - kWave) hb[p] = sh;
            }
            const uint32_t r32 = (uint32_t)row;
            top[p].offer_lanes(ok && top[p].admits(lo, r32), lo, r32);
        }
    };
    if (base0 >= n_rows) {  // a wave without rows (tiny corpora): empty lists
        top[0].init(1);
        for (int32_t qe = 0; qe < Q.n; ++qe) {
            Q.blk_s[qe][(blockIdx.x * WAVES + wave) * kListLen + lane] = top[0].s;
            Q.blk_r[qe][(blockIdx.x * WAVES + wave) * kListLen + lane] = top[0].r;
        }
        return;
    }
    Batch b0, b1;
    issue(base0, b0);  // in flight during the first prologue
    next_query(0);
    int64_t base = base0;
    // K1's loop: the next batch is issued unconditionally before the current one is reduced (dense_scan.hip); after the
    // last batch of a pass the walk wraps to the block's first row for the next QP queries (Q.n is a multiple of QP)
    for (;;) {
        int32_t nq = qi;
        int64_t next = base + RW;
        if (next >= lim) {
            next = base0;
            nq += QP;
        }
        issue(next, b1);
        reduce(base, b0);
        if (nq != qi) {
            flush(qi);
            if (nq >= Q.n) break;
            qi = nq;
            next_query(qi);
        }
        base = next;
        next = base + RW;
        if (next >= lim) {
            next = base0;
            nq += QP;
        }
        issue(next, b0);
        reduce(base, b1);
        if (nq != qi) {
            flush(qi);
            if (nq >= Q.n) break;
            qi = nq;
            next_query(qi);
        }
        base = next;
    }
}

template <int G, int CH, int R, bool FILTER>
__global__ __launch_bounds__(kScanThreads) __attribute__((amdgpu_waves_per_eu(4))) void dense_prefilter_i8_scan_kernel(
    const i32x4 *__restrict__ img, const f32x4 *__restrict__ meta, PrefilterQueries Q, int64_t n_rows, int32_t dim,
    int32_t k, const uint16_t *__restrict__ src, const uint32_t *__restrict__ allow_bits) {
    i8_scan_body<G, CH, R, FILTER, 1>(img, meta, Q, n_rows, dim, k, src, allow_bits);
}

// the pair pass: Q.n is even (launch_dense_prefilter_scan sends an odd last query through the kernel above)
template <int G, int CH, int R, bool FILTER>
__global__ __launch_bounds__(kScanThreads) __attribute__((amdgpu_waves_per_eu(4))) void dense_prefilter_i8_pair_kernel(
    const i32x4 *__restrict__ img, const f32x4 *__restrict__ meta, PrefilterQueries Q, int64_t n_rows, int32_t dim,
    int32_t k, const uint16_t *__restrict__ src, const uint32_t *__restrict__ allow_bits) {
    i8_scan_body<G, CH, R, FILTER, 2>(img, meta, Q, n_rows, dim, k, src, allow_bits);
}

// ---------------------------------------------------------------- 2. T per query: one workgroup of 16 waves each
constexpr int kThrWaves = 16;
__global__ __launch_bounds__(kThrWaves * kWave) void dense_prefilter_threshold_kernel(PrefilterQueries Q, int32_t n_lists,
                                                                                     int32_t k) {
    __shared__ float ls[kThrWaves * kListLen];
    __shared__ uint32_t lr[kThrWaves * kListLen];
    const int qi = blockIdx.x;
    const int wave = threadIdx.x / kWave;
    WaveTopK<float> t;
    t.init(k);
    merge_lists(t, Q.blk_s[qi], Q.blk_r[qi], n_lists, k, wave, kThrWaves);
    block_merge(t, ls, lr, kThrWaves);
    if (wave == 0) {
        const float T = read_lane(t.s, k - 1);  // -inf when fewer than k rows are allowed
        if (lane_id() == 0) *Q.thr[qi] = T;
    }
}

// ---------------------------------------------------------------- 3. exact rescoring of the survivors
// G, CH: K1's shape for dim (scan_dispatch(dim)).  A wave sweeps 1,024 hi values per step (4 dwordx4 per lane: the
// whole sweep is one round trip per wave at 1M rows); each survivor is rescored by one lane group with K1's mapping.
constexpr int kSweepU = 4;
template <int G, int CH>
__global__ __launch_bounds__(kScanThreads) void dense_prefilter_rescore_kernel(
    const float *__restrict__ emb, PrefilterQueries Q, int64_t n_rows, int32_t dim, int32_t k,
    unsigned long long *__restrict__ survivors, DeferredTail dt) {
    constexpr int GROUPS = kWave / G;
    constexpr int STEP = kWave * 4 * kSweepU;
    int scan_blocks = gridDim.x;
    if (dt.out != nullptr) {  // the last workgroup merges the previous single query's lists (as K1 does)
        scan_blocks -= 1;
        if ((int)blockIdx.x == scan_blocks) {
            dense_tail_block(dt);
            return;
        }
    }
    const int lane = lane_id();
    const int wave = threadIdx.x / kWave;
    const int sub = lane % G, grp = lane / G;
    const bool leader = sub == G - 1;
    const f32x4 *__restrict__ ev = reinterpret_cast<const f32x4 *>(emb);
    const int64_t row_f4 = dim / 4;
    const int64_t total_waves = (int64_t)scan_blocks * kScanWaves;
    const int64_t wave_global = (int64_t)blockIdx.x * kScanWaves + wave;
    unsigned long long count = 0;
    for (int32_t qi = 0; qi < Q.n; ++qi) {
        f32x4 q[CH];
        const f32x4 *__restrict__ query = reinterpret_cast<const f32x4 *>(Q.q[qi]);
#pragma unroll
        for (int c = 0; c < CH; ++c) q[c] = query[c * G + sub];
        const float T = *Q.thr[qi];
        const f32x4 *__restrict__ hv = reinterpret_cast<const f32x4 *>(Q.hi[qi]);
        WaveTopK<float> top;
        top.init(k);
        for (int64_t b = wave_global * STEP; b < n_rows; b += total_waves * STEP) {
            f32x4 h[kSweepU];
#pragma unroll
            for (int u = 0; u < kSweepU; ++u) {  // rows b + 4 (u 64 + lane) .. +3; the buffer is padded to 64 rows
                const int64_t r0 = b + 4 * (u * kWave + lane);
                h[u] = r0 < n_rows ? hv[r0 / 4] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < kSweepU; ++u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t row = b + 4 * (u * kWave + lane) + j;
                    unsigned long long mask = __ballot(row < n_rows && h[u][j] >= T);
                    if (mask == 0) continue;
                    count += __builtin_popcountll(mask);
                    while (mask) {  // GROUPS survivors per pass: lane group g takes the g-th lowest bit
                        int64_t mine = -1;
#pragma unroll
                        for (int g = 0; g < GROUPS; ++g) {
                            if (mask) {
                                const int l = __builtin_ctzll(mask);
                                mask &= mask - 1;
                                if (grp == g) mine = b + 4 * (u * kWave + l) + j;
                            }
                        }
                        const bool has = mine >= 0;
                        const f32x4 *p = ev + (has ? mine : 0) * row_f4 + sub;
                        float acc = 0.f;
#pragma unroll
                        for (int c = 0; c < CH; ++c) acc = dot4(p[c * G], q[c], acc);  // K1: dot4(row, query, acc)
                        acc = nan_first(group_sum<G>(acc));
                        const uint32_t r32 = (uint32_t)mine;
                        top.offer_lanes(leader && has && top.admits(acc, r32), acc, r32);
                    }
                }
            }
        }
        Q.blk_s[qi][(blockIdx.x * kScanWaves + wave) * kListLen + lane] = top.s;
        Q.blk_r[qi][(blockIdx.x * kScanWaves + wave) * kListLen + lane] = top.r;
    }
    if (lane == 0 && count) atomicAdd(survivors, count);
}

// ---------------------------------------------------------------- host
// The dimensions served: the fp16 row of dim values has K1's byte geometry of a dim / 2 row (Half), the int8 row that of
// a dim / 4 row (Quarter), shapes of up to 4 dwordx4 per lane and row (dim <= 2,048); the rescore kernel takes K1's own
// shape for dim (Full).  An explicit table, so that only the kernels these six dimensions run are compiled.
template <class H, class Q4, class F32>
struct PrefilterShape {
    using Half = H;
    using Quarter = Q4;
    using Full = F32;
};
template <class F>
static bool prefilter_dispatch(int d, F &&f) {
    switch (d) {
        case 256: f(PrefilterShape<ScanShape<32, 1>, ScanShape<16, 1>, ScanShape<32, 2>>{}); return true;
        case 512: f(PrefilterShape<ScanShape<32, 2>, ScanShape<32, 1>, ScanShape<64, 2>>{}); return true;
        case 768: f(PrefilterShape<ScanShape<32, 3>, ScanShape<16, 3>, ScanShape<64, 3>>{}); return true;
        case 1024: f(PrefilterShape<ScanShape<64, 2>, ScanShape<32, 2>, ScanShape<64, 4>>{}); return true;
        case 1536: f(PrefilterShape<ScanShape<64, 3>, ScanShape<32, 3>, ScanShape<64, 6>>{}); return true;
        case 2048: f(PrefilterShape<ScanShape<64, 4>, ScanShape<64, 2>, ScanShape<64, 8>>{}); return true;
        default: return false;
    }
}

// ... and the table agrees with scan_dispatch: Half is the shape of dim / 2, Quarter that of dim / 4, Full (the bits of
// K1's score) that of dim
bool dense_prefilter_has_shape(const anrag_index *idx) {
    const int d = idx->dim;
    bool ok = false;
    prefilter_dispatch(d, [&](auto ps) {
        using P = decltype(ps);
        bool half = false, quarter = false, full = false;
        scan_dispatch(d / 2, [&](auto s) { half = decltype(s)::kG == P::Half::kG && decltype(s)::kCH == P::Half::kCH; });
        scan_dispatch(d / 4, [&](auto s) {
            quarter = decltype(s)::kG == P::Quarter::kG && decltype(s)::kCH == P::Quarter::kCH;
        });
        scan_dispatch(d, [&](auto s) { full = decltype(s)::kG == P::Full::kG && decltype(s)::kCH == P::Full::kCH; });
        ok = half && quarter && full;
    });
    return ok;
}

int dense_prefilter_vgprs(const anrag_index *idx) {
    int regs = 0;
    auto take = [&](const void *fn) {
        hipFuncAttributes attr;
        if (hipFuncGetAttributes(&attr, fn) == hipSuccess && attr.numRegs > regs) regs = attr.numRegs;
    };
    prefilter_dispatch(idx->dim, [&](auto ps) {
        using H = typename decltype(ps)::Half;
        using Q4 = typename decltype(ps)::Quarter;
        using F = typename decltype(ps)::Full;
        if (idx->pf_form == kPrefilterInt8)
            take(reinterpret_cast<const void *>(&dense_prefilter_i8_scan_kernel<Q4::kG, Q4::kCH, Q4::kR, true>));
        else
            take(reinterpret_cast<const void *>(&dense_prefilter_scan_kernel<H::kG, H::kCH, H::kR, true>));
        take(reinterpret_cast<const void *>(&dense_prefilter_rescore_kernel<F::kG, F::kCH>));
    });
    return regs;
}

// one block per form: the image and its per-row data (fp16: the radius m; int8: {s_e, m1, m2, 0}), then what both
// forms share -- hi per list set, T, the survivor count
int64_t dense_prefilter_bytes(int64_t n_rows, int32_t dim, int32_t form) {
    Carver c(nullptr);
    if (form == kPrefilterInt8) {
        c.take<int8_t>(n_rows * dim);
        c.take<float>(4 * n_rows);
    } else {
        c.take<_Float16>(n_rows * dim);
        c.take<float>(n_rows);
    }
    c.take<float>((int64_t)kPipeSlots * ((n_rows + 63) / 64 * 64));
    c.take<float>(kPipeSlots);
    c.take<unsigned long long>(1);
    return c.at;
}

void free_dense_prefilter(anrag_index *idx) {
    if (idx->pf_block) {
        (void)counted_free(idx->pf_block);
        idx->hbm_bytes -= idx->pf_bytes;
    }
    idx->pf_block = nullptr;
    idx->pf_bytes = 0;
    idx->pf_form = 0;
    idx->d_pf_img = nullptr;
    idx->d_pf_m = idx->d_pf_hi = idx->d_pf_thr = nullptr;
    idx->d_pf_survivors = nullptr;
}

int build_dense_prefilter(anrag_index *idx, int32_t form) {
    if (idx->pf_block && idx->pf_form == form) return ANRAG_OK;
    ANRAG_REQUIRE(dense_prefilter_has_shape(idx), "dense prefilter: no kernel shape for dim %d", idx->dim);
    free_dense_prefilter(idx);  // the other form's block: one at a time
    const int64_t n = idx->n_rows, bytes = dense_prefilter_bytes(n, idx->dim, form);
    void *p = nullptr;
    hipError_t e = counted_malloc(&p, (size_t)bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipMalloc(%lld bytes) for the dense prefilter failed: %s", (long long)bytes, hipGetErrorString(e));
        return ANRAG_ERR_NOMEM;
    }
    idx->pf_block = p;
    idx->pf_bytes = bytes;
    idx->pf_form = form;
    idx->hbm_bytes += bytes;
    Carver c(static_cast<char *>(p));
    if (form == kPrefilterInt8) {
        idx->d_pf_img = c.take<int8_t>(n * idx->dim);
        idx->d_pf_m = c.take<float>(4 * n);
    } else {
        idx->d_pf_img = c.take<_Float16>(n * idx->dim);
        idx->d_pf_m = c.take<float>(n);
    }
    idx->pf_hi_stride = (n + 63) / 64 * 64;
    idx->d_pf_hi = c.take<float>((int64_t)kPipeSlots * idx->pf_hi_stride);
    idx->d_pf_thr = c.take<float>(kPipeSlots);
    idx->d_pf_survivors = c.take<unsigned long long>(1);
    hipStream_t st = idx->primary;
    ANRAG_HIP(hipMemsetAsync(idx->d_pf_survivors, 0, sizeof(unsigned long long), st));
    const int64_t need = (n + kScanWaves - 1) / kScanWaves;
    const int64_t cap = (int64_t)idx->n_cus * 8;
    const unsigned grid = (unsigned)(need < cap ? need : cap);
    if (form == kPrefilterInt8)
        dense_prefilter_i8_convert_kernel<<<grid, kScanThreads, 0, st>>>(
            idx->d_emb, n, idx->dim, static_cast<uint32_t *>(idx->d_pf_img), reinterpret_cast<f32x4 *>(idx->d_pf_m));
    else
        dense_prefilter_convert_kernel<<<grid, kScanThreads, 0, st>>>(idx->d_emb, n, idx->dim,
                                                                     static_cast<_Float16 *>(idx->d_pf_img), idx->d_pf_m);
    ANRAG_HIP(hipGetLastError());
    ANRAG_HIP(hipStreamSynchronize(st));
    idx->pf_queries = 0;
    return ANRAG_OK;
}

// The three launches come in two halves so that the hybrid pipeline can keep `primary` for the scans alone: the scan
// half writes hi[set] and the lo lists of the set; the finish half (threshold, rescore) reads them, the query vectors and
// the fp32 rows, and leaves the set's exact lists.  Everything the finish half touches is the set's own (hi row, T,
// lists), so it may run on another stream, behind an event recorded after the scan half, while later scans proceed.
static PrefilterQueries prefilter_queries(const anrag_index *idx, const float *const *d_queries, int32_t n_queries,
                                          const int *sets) {
    PrefilterQueries Q;
    Q.n = n_queries;
    for (int i = 0; i < kScanGroupMax; ++i) {
        const int j = i < n_queries ? i : 0;
        Q.q[i] = d_queries[j];
        Q.hi[i] = idx->d_pf_hi + (int64_t)sets[j] * idx->pf_hi_stride;
        Q.blk_s[i] = idx->d_blk_score_f32 + (int64_t)sets[j] * kMaxScanLists * kListLen;
        Q.blk_r[i] = idx->d_blk_row_a + (int64_t)sets[j] * kMaxScanLists * kListLen;
        Q.thr[i] = idx->d_pf_thr + sets[j];
    }
    return Q;
}

// The shapes with a pair instantiation of the int8 scan (dense_prefilter_i8_pair_kernel): every one that stays within 128
// VGPRs without spills.  A shape that is not listed keeps single passes for every query of a group.
template <int G, int CH, bool FILTER>
constexpr bool i8_pair_shape() {
    return true;
}

bool dense_prefilter_pairs(const anrag_index *idx, bool filtered) {
    bool ok = false;
    if (idx->pf_form != kPrefilterInt8) return false;
    prefilter_dispatch(idx->dim, [&](auto ps) {
        using Q4 = typename decltype(ps)::Quarter;
        ok = filtered ? i8_pair_shape<Q4::kG, Q4::kCH, true>() : i8_pair_shape<Q4::kG, Q4::kCH, false>();
    });
    return ok;
}

// the queries [first, first + n) of Q as a group of their own
static PrefilterQueries prefilter_queries_slice(const PrefilterQueries &Q, int first, int n) {
    PrefilterQueries S;
    S.n = n;
    for (int i = 0; i < kScanGroupMax; ++i) {
        const int j = first + (i < n ? i : 0);
        S.q[i] = Q.q[j];
        S.hi[i] = Q.hi[j];
        S.blk_s[i] = Q.blk_s[j];
        S.blk_r[i] = Q.blk_r[j];
        S.thr[i] = Q.thr[j];
    }
    return S;
}

// The int8 form takes the queries of a group two at a time through one walk of the image (the pair kernel) wherever the
// shape has a pair instantiation and pairing is on; an odd last query follows in a launch of the single kernel on the
// same stream (a run-time branch into the single code inside the pair kernel would hold both forms' registers).
int launch_dense_prefilter_scan(anrag_index *idx, hipStream_t st, const float *const *d_queries, int32_t n_queries,
                                int32_t k, const uint32_t *allow, const int *sets) {
    const PrefilterQueries Q = prefilter_queries(idx, d_queries, n_queries, sets);
    const int grid = dense_scan_grid(idx);
    prefilter_dispatch(idx->dim, [&](auto ps) {
        using H = typename decltype(ps)::Half;
        using Q4 = typename decltype(ps)::Quarter;
        if (idx->pf_form == kPrefilterInt8) {
            const i32x4 *img = reinterpret_cast<const i32x4 *>(idx->d_pf_img);
            const f32x4 *meta = reinterpret_cast<const f32x4 *>(idx->d_pf_m);
            const uint16_t *src = allow ? idx->d_dense_src : nullptr;
            int32_t paired = 0;  // queries taken by the pair kernel
            if (idx->scan_pair_mode != 0 && n_queries >= 2) {
                if constexpr (i8_pair_shape<Q4::kG, Q4::kCH, true>())
                    if (allow) {
                        paired = n_queries & ~1;
                        dense_prefilter_i8_pair_kernel<Q4::kG, Q4::kCH, Q4::kR, true><<<grid, kScanThreads, 0, st>>>(
                            img, meta, prefilter_queries_slice(Q, 0, paired), idx->n_rows, idx->dim, k, src, allow);
                    }
                if constexpr (i8_pair_shape<Q4::kG, Q4::kCH, false>())
                    if (!allow) {
                        paired = n_queries & ~1;
                        dense_prefilter_i8_pair_kernel<Q4::kG, Q4::kCH, Q4::kR, false><<<grid, kScanThreads, 0, st>>>(
                            img, meta, prefilter_queries_slice(Q, 0, paired), idx->n_rows, idx->dim, k, src, allow);
                    }
            }
            idx->pf_pair_passes += paired / 2;
            idx->pf_single_passes += n_queries - paired;
            if (paired == n_queries) return;
            const PrefilterQueries S = paired ? prefilter_queries_slice(Q, paired, n_queries - paired) : Q;
            if (allow)
                dense_prefilter_i8_scan_kernel<Q4::kG, Q4::kCH, Q4::kR, true><<<grid, kScanThreads, 0, st>>>(
                    img, meta, S, idx->n_rows, idx->dim, k, src, allow);
            else
                dense_prefilter_i8_scan_kernel<Q4::kG, Q4::kCH, Q4::kR, false><<<grid, kScanThreads, 0, st>>>(
                    img, meta, S, idx->n_rows, idx->dim, k, nullptr, nullptr);
        } else {
            const f32x4 *img = reinterpret_cast<const f32x4 *>(idx->d_pf_img);
            if (allow)
                dense_prefilter_scan_kernel<H::kG, H::kCH, H::kR, true><<<grid, kScanThreads, 0, st>>>(
                    img, idx->d_pf_m, Q, idx->n_rows, idx->dim, k, idx->d_dense_src, allow);
            else
                dense_prefilter_scan_kernel<H::kG, H::kCH, H::kR, false><<<grid, kScanThreads, 0, st>>>(
                    img, idx->d_pf_m, Q, idx->n_rows, idx->dim, k, nullptr, nullptr);
        }
    });
    ANRAG_HIP(hipGetLastError());
    idx->pf_queries += n_queries;
    return ANRAG_OK;
}

// the threshold launch of the finish half, on its own for anrag_debug_prefilter_bounds
static hipError_t launch_threshold(const PrefilterQueries &Q, hipStream_t st, int32_t n_queries, int grid, int32_t k) {
    dense_prefilter_threshold_kernel<<<n_queries, kThrWaves * kWave, 0, st>>>(Q, grid * kScanWaves, k);
    return hipGetLastError();
}

int launch_dense_prefilter_threshold(anrag_index *idx, hipStream_t st, const float *const *d_queries, int32_t n_queries,
                                     int32_t k, const int *sets) {
    const PrefilterQueries Q = prefilter_queries(idx, d_queries, n_queries, sets);
    ANRAG_HIP(launch_threshold(Q, st, n_queries, dense_scan_grid(idx), k));
    return ANRAG_OK;
}

int launch_dense_prefilter_finish(anrag_index *idx, hipStream_t st, const float *const *d_queries, int32_t n_queries,
                                  int32_t k, const int *sets, const DeferredTail &dt) {
    const PrefilterQueries Q = prefilter_queries(idx, d_queries, n_queries, sets);
    const int grid = dense_scan_grid(idx);
    hipError_t err = hipSuccess;  // of the first launch that failed
    prefilter_dispatch(idx->dim, [&](auto ps) {
        using F = typename decltype(ps)::Full;
        if ((err = launch_threshold(Q, st, n_queries, grid, k)) != hipSuccess) return;
        dense_prefilter_rescore_kernel<F::kG, F::kCH><<<grid + (dt.out ? 1 : 0), kScanThreads, 0, st>>>(
            idx->d_emb, Q, idx->n_rows, idx->dim, k, idx->d_pf_survivors, dt);
        err = hipGetLastError();
    });
    ANRAG_HIP(err);
    return ANRAG_OK;
}

// The scan's row geometry for this index's form: a wave owns rows [w * rows_per_wave, (w + 1) * rows_per_wave) and
// walks them in batches of batch_rows (RW of the scan kernel).  For tests that plant rows at the edges of a block.
void dense_prefilter_geometry(const anrag_index *idx, int64_t *rows_per_wave, int32_t *batch_rows) {
    *rows_per_wave = 0;
    *batch_rows = 0;
    prefilter_dispatch(idx->dim, [&](auto ps) {
        using H = typename decltype(ps)::Half;
        using Q4 = typename decltype(ps)::Quarter;
        const int rw = idx->pf_form == kPrefilterInt8 ? kWave / Q4::kG * Q4::kR : kWave / H::kG * H::kR;
        const int64_t total_waves = (int64_t)dense_scan_grid(idx) * kScanWaves;
        *batch_rows = rw;
        *rows_per_wave = ((idx->n_rows + total_waves - 1) / total_waves + rw - 1) / rw * rw;
    });
}

}  // namespace anrag
