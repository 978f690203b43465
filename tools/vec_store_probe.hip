// Microbenchmark: the row-major [n][S] float stores of a one-lane-per-row kernel, as the vector env's step kernel issues them
// (csrc/row_store.hpp: staged through LDS, 16-byte stores) against the plain form (S stores of 4 bytes per lane, stride 4 S).
// Each lane builds its row from one loaded float, so the stores are what the kernel does; shapes of tools/vec_env_probe.py.
//   hipcc -O3 --offload-arch=gfx950 -o vec_store_probe tools/vec_store_probe.hip && ./vec_store_probe
// Prints, per shape and arm, the median (min, max) microseconds per launch of 7 windows of 200 launches between HIP events.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../trajopt-grpo_amd/csrc/row_store.hpp"

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        hipError_t e__ = (x);                                                                     \
        if (e__ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e__)); exit(1); } \
    } while (0)

template <int S, bool kStaged>
__global__ __launch_bounds__(256) void store_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n) {
    extern __shared__ float4 lds4[];
    float* lds_wave = reinterpret_cast<float*>(lds4) + (threadIdx.x >> 6) * 64 * S;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row0 = i - (threadIdx.x & 63);
    const int64_t ic = i < n ? i : n - 1;
    const float x = src[ic];
    float row[S];
#pragma unroll
    for (int k = 0; k < S; ++k) row[k] = x + (float)k;
    if constexpr (kStaged) {
        tg::store_rows_staged<S>(dst, row0, n, row, lds_wave);
    } else {
        if (i < n) {
#pragma unroll
            for (int k = 0; k < S; ++k) dst[i * S + k] = row[k];
        }
    }
}

template <int S, bool kStaged>
static void run(const char* what, int64_t n, int block) {
    float *src, *dst;
    CHECK(hipMalloc(&src, n * sizeof(float)));
    CHECK(hipMalloc(&dst, n * S * sizeof(float)));
    CHECK(hipMemset(src, 0, n * sizeof(float)));
    const dim3 grid((unsigned)((n + block - 1) / block));
    const size_t lds = kStaged ? (size_t)block * S * sizeof(float) : 0;
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    std::vector<float> us;
    const int launches = 200;
    for (int rep = 0; rep < 2 + 7; ++rep) {
        CHECK(hipEventRecord(a, 0));
        for (int l = 0; l < launches; ++l) hipLaunchKernelGGL((store_kernel<S, kStaged>), grid, dim3(block), lds, 0, src, dst, n);
        CHECK(hipEventRecord(b, 0));
        CHECK(hipEventSynchronize(b));
        CHECK(hipGetLastError());
        float ms;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (rep >= 2) us.push_back(ms * 1e3f / launches);
    }
    std::sort(us.begin(), us.end());
    printf("%-28s %-7s median %7.2f us  (min %7.2f, max %7.2f) per launch\n", what, kStaged ? "staged" : "plain", us[us.size() / 2], us.front(),
           us.back());
    CHECK(hipFree(src));
    CHECK(hipFree(dst));
}

int main() {
    // env_grid's geometry: one wave per workgroup up to 2^18 rows
    run<5, true>("CartPole  S=5  n=4096", 4096, 64);
    run<5, false>("CartPole  S=5  n=4096", 4096, 64);
    run<20, true>("QuadPole  S=20 n=65536", 65536, 64);
    run<20, false>("QuadPole  S=20 n=65536", 65536, 64);
    run<20, true>("QuadPole  S=20 n=1048576", 1048576, 256);
    run<20, false>("QuadPole  S=20 n=1048576", 1048576, 256);
    return 0;
}
