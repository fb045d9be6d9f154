// The fp64 vector FMA rate of the part, measured: the ceiling K1TD (dense_tile_f64.hip) is held against in DESIGN.md.
// Every lane runs CHAINS independent chains acc = fma(acc, a, b) (v_fma_f64, nothing else in the loop but the counter),
// WAVES waves per SIMD on every CU, long enough that launch and ramp vanish.  Printed per (chains, waves per SIMD): FMA/s
// over the whole device and per CU and clock-free per second.  The chains are kept alive by one store per lane at the end.
// Build + run:  hipcc --offload-arch=gfx950 -O3 scripts/exp/fma_f64_rate.hip -o scripts/exp/fma_f64_rate && scripts/exp/fma_f64_rate
#include <hip/hip_runtime.h>
#include <cstdio>

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

template <int CHAINS>
__global__ __launch_bounds__(256) void fma_kernel(double *out, double a, double b, int iters) {
    double acc[CHAINS];
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) acc[c] = (double)(threadIdx.x + c);
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_fma(acc[c], a, b);
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) s += acc[c];
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}

template <int CHAINS>
static int run(int cus, int wgs_per_cu, double *d_out) {
    const int iters = 4096;
    const int grid = cus * wgs_per_cu;  // a workgroup of 256 = one wave per SIMD
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    fma_kernel<CHAINS><<<grid, 256>>>(d_out, 0.999999, 1e-9, 64);  // warm
    CHECK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        CHECK(hipEventRecord(e0));
        fma_kernel<CHAINS><<<grid, 256>>>(d_out, 0.999999, 1e-9, iters);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    const double fmas = (double)grid * 256 * CHAINS * 8.0 * iters;
    printf("chains %2d, waves/SIMD %d: %.3f ms, %.2f T FMA/s (%.2f TFLOP/s), %.1f G FMA/s per CU\n", CHAINS, wgs_per_cu, best,
           fmas / best / 1e9, 2 * fmas / best / 1e9, fmas / best / 1e6 / cus);
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    return 0;
}

int main() {
    int cus = 0;
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    int khz = 0;
    CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0));
    printf("%d CUs, clock attribute %.0f MHz\n", cus, khz / 1e3);
    double *d_out = nullptr;
    CHECK(hipMalloc(&d_out, (size_t)cus * 8 * 256 * sizeof(double)));
    for (int w = 1; w <= 4; w *= 2) {
        if (run<1>(cus, w, d_out)) return 1;
        if (run<2>(cus, w, d_out)) return 1;
        if (run<4>(cus, w, d_out)) return 1;
        if (run<8>(cus, w, d_out)) return 1;
        if (run<16>(cus, w, d_out)) return 1;
    }
    CHECK(hipFree(d_out));
    return 0;
}
