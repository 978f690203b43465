// Row-major [n][S] float rows out of a one-lane-per-row kernel (vec_env.hip; tools/vec_store_probe.hip times it against plain stores).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tg {

// the lanes of a wave see each other's LDS writes behind this (a wave's LDS operations complete in order; the fence keeps the
// compiler from moving them across)
__device__ static inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Rows [row0, row0 + 64) of a row-major f32 [n][S] array, one row per lane in registers -> memory.  The wave's rows are one
// contiguous block of 64 S floats that starts 16-byte aligned (row0 is a multiple of 64, the array 16-byte aligned: the host
// checks): the block is staged in the wave's LDS region (lane l writes its row at dword l S: an odd S is conflict-free, S = 10 two-way
// -- free on ds_write_b32 -- S = 20 four-way) and leaves as consecutive 16-byte stores, lane l the chunks l, l + 64, ... -- whole
// 1-KiB lines per instruction instead of S stores of 4 bytes at a stride of 4 S.  The tail wave of the array writes the chunks that
// lie inside its n - row0 rows, and the last 1..3 floats one by one when 4 does not divide their count.  Every lane of the wave must
// call it (lanes beyond n carry any row).
template <int S>
__device__ static inline void store_rows_staged(float* __restrict__ dst, int64_t row0, int64_t n, const float (&row)[S], float* lds_wave) {
    const int lane = threadIdx.x & 63;
    const int64_t left = n - row0;
    const int valid = (int)(left < 64 ? left : 64) * S;                   // floats of this wave's block that exist
#pragma unroll
    for (int k = 0; k < S; ++k) lds_wave[lane * S + k] = row[k];
    wave_lds_sync();
    float* out = dst + row0 * S;
    constexpr int kChunks = 16 * S;                                         // 16-byte chunks of a full block
#pragma unroll
    for (int q = 0; q < (kChunks + 63) / 64; ++q) {
        const int j = q * 64 + lane;
        if (j < kChunks) {
            if (4 * j + 3 < valid) {
                *reinterpret_cast<float4*>(out + 4 * j) = *reinterpret_cast<const float4*>(lds_wave + 4 * j);
            } else {
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (4 * j + e < valid) out[4 * j + e] = lds_wave[4 * j + e];
            }
        }
    }
    wave_lds_sync();                                                        // (the region is free for the next block)
}

}  // namespace tg
