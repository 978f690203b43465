// GRPO's per-time-step group baseline (GRPO(baseline="step"); INTEGRATION.md, "GRPO step baselines"), gfx950.
//
//   tg_grpo_step_advantage   from the returns-to-go R f32 [T][n] and the mask u8 [T][n] (group g = envs [g E, (g + 1) E)), the
//                            advantage A f32 [T][n]: every valid entry minus the mean of the valid entries of ITS group at ITS
//                            time step, divided (mode 1) by one pooled within-step std of the group.  Two launches.
//
// The arithmetic (tests/grpo_baseline_fp64.py restates it, order included).  [T][n] with n = G E is S = T G segments of E
// consecutive floats: segment s = t G + g starts at s E.  With V the entries of a segment whose mask byte is non-zero, c = |V|:
//     s1 = sum_V (double)R      mean = s1 / c (f64; 0 for c = 0)      b = (float)mean
//     d  = R - b  (one rounded f32 subtraction; +0 for an invalid entry)      q = sum_V (double)d * (double)d   (each product exact)
// and per group, over the steps in ascending t (one thread, serial):  Q = sum_t q,  C = sum_t c,  K = #{t: c >= 1},
//     std = sqrt(Q / (C - K)) in f64 (0 when C - K <= 0)      A = d / ((float)std + 1e-8f)  (mode 1)      A = d  (mode 0).
// The order of the two segment sums.  The segment is cut into quads of 4 consecutive entries (the last one may be short); W = the
// smallest power of two >= the number of quads, at most 64, lanes share a segment.  Lane l adds, to a sum that starts at +0, the
// entries of quads l, l + W, l + 2 W, ... in ascending index (an invalid entry adds +0, which changes no bit); then the lanes'
// sums meet in a __shfl_down tree, offsets W / 2, ..., 1 (lane l takes lane l + off); lane 0 holds the result.  No atomics.
//
// Pass 1 (step_segments_kernel): 64 / W segments per wave.  It reads the segment twice -- the second read, right behind the first
// by the same lanes, is a cache hit -- and leaves {c, mean, q} in three f64 planes [G][T] (a group's steps are contiguous);
// mode 0 also writes d, which IS the advantage.  Pass 2 (step_scale_kernel): one workgroup per (group, chunk of time steps);
// three of its threads first add the group's T entries of the q and c planes serially (redundant across the group's workgroups,
// ~T dependent f64 additions: the price of one launch less and of a fixed order), then the workgroup recomputes d = R - b from
// the mean plane -- the same subtraction, the same bits -- and divides.  Mode 0 launches pass 2 for the group sums alone.
// Loads are unconditional from clamped addresses (a load under a branch is waited for where it stands); with E % 4 == 0,
// n % 4 == 0 and 16-B aligned arrays every quad is one 16-B load of R and one 4-B load of the mask.
#include <cmath>

#include "tg_common.hpp"

namespace tg {

constexpr int kSbBlock = 256;
constexpr int kSbScaleEntries = 8192;      // entries of one pass-2 workgroup (whole time steps; one step when E is larger)

// one quad of the segment at `base`: values and validity flags.  kc is a quad index inside the segment (clamped by the caller).
template <bool VEC>
__device__ static inline void sb_load_quad(const float* __restrict__ R, const uint8_t* __restrict__ mask, int64_t base, int64_t kc, int64_t E,
                                           bool quad_ok, float (&v)[4], bool (&ok)[4]) {
    if (VEC) {
        const float4 r = *reinterpret_cast<const float4*>(R + base + 4 * kc);
        const uint32_t m = *reinterpret_cast<const uint32_t*>(mask + base + 4 * kc);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) ok[j] = quad_ok && ((m >> (8 * j)) & 0xFFu) != 0u;
    } else {
        uint8_t m[4];
        bool in[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t e = 4 * kc + j;
            in[j] = quad_ok && e < E;
            const int64_t ec = e < E ? e : E - 1;
            v[j] = R[base + ec];
            m[j] = mask[base + ec];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ok[j] = in[j] && m[j] != 0;
    }
}

template <bool VEC, bool WRITE_D>
__global__ __launch_bounds__(kSbBlock) void step_segments_kernel(const float* __restrict__ R, const uint8_t* __restrict__ mask, int32_t T,
                                                                 int64_t E, int64_t G, int log2_w, double* __restrict__ tab, float* __restrict__ dout) {
    const int W = 1 << log2_w;                                              // lanes per segment
    const int64_t S = (int64_t)T * G;
    const int64_t sg = ((int64_t)blockIdx.x * kSbBlock + threadIdx.x) >> log2_w;
    const int l = threadIdx.x & (W - 1);
    const bool seg_ok = sg < S;
    const int64_t base = (seg_ok ? sg : S - 1) * E;
    const int64_t nq = (E + 3) >> 2;
    const int64_t iters = (nq + W - 1) >> log2_w;
    // ---- the sum and the count of the valid entries ----
    double s1 = 0.0, c = 0.0;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t k = l + it * W;
        const bool quad_ok = k < nq;
        float v[4]; bool ok[4];
        sb_load_quad<VEC>(R, mask, base, quad_ok ? k : nq - 1, E, quad_ok, v, ok);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s1 += ok[j] ? (double)v[j] : 0.0;
            c += ok[j] ? 1.0 : 0.0;
        }
    }
    for (int off = W >> 1; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, W);
        c += __shfl_down(c, off, W);
    }
    s1 = __shfl(s1, 0, W);
    c = __shfl(c, 0, W);
    const double mean = c > 0.0 ? s1 / c : 0.0;
    const float b = (float)mean;
    // ---- the residuals and their squares, in the same order ----
    double q = 0.0;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t k = l + it * W;
        const bool quad_ok = k < nq;
        float v[4]; bool ok[4];
        sb_load_quad<VEC>(R, mask, base, quad_ok ? k : nq - 1, E, quad_ok, v, ok);
        float d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[j] = ok[j] ? rn_sub(v[j], b) : 0.0f;
            q += (double)d[j] * (double)d[j];                              // (exact product; +0 for an invalid entry)
        }
        if (WRITE_D && seg_ok && quad_ok) {
            if (VEC) {
                *reinterpret_cast<float4*>(dout + base + 4 * k) = float4{d[0], d[1], d[2], d[3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * k + j < E) dout[base + 4 * k + j] = d[j];
            }
        }
    }
    for (int off = W >> 1; off > 0; off >>= 1) q += __shfl_down(q, off, W);
    if (seg_ok && l == 0) {
        const int64_t t = sg / G, g = sg - t * G;
        const int64_t plane = G * (int64_t)T, at = g * T + t;
        tab[at] = c;
        tab[plane + at] = mean;
        tab[2 * plane + at] = q;
    }
}

// SCALE: A = (R - b) / ((float)std_g + 1e-8f) for this workgroup's time steps of its group; else only the group's sums.
template <bool VEC, bool SCALE>
__global__ __launch_bounds__(kSbBlock) void step_scale_kernel(const float* __restrict__ R, const uint8_t* __restrict__ mask, int64_t n, int32_t T,
                                                              int64_t E, int64_t G, int32_t t_chunk, int32_t n_chunks,
                                                              const double* __restrict__ tab, float* __restrict__ A, double* __restrict__ group_out) {
    __shared__ double sh[3];                                                // {Q, C, K} of the group
    const int64_t g = blockIdx.x / n_chunks;
    const int32_t chunk = (int32_t)(blockIdx.x - g * n_chunks);
    const int64_t plane = G * (int64_t)T;
    if (threadIdx.x < 3) {
        // thread 0: Q from the q plane; thread 1: C from the c plane; thread 2: K, the steps of the c plane with c >= 1 -- ascending t
        const int j = threadIdx.x;
        const double* p = tab + (j == 0 ? 2 * plane : 0) + g * T;
        double acc = 0.0;
        int32_t t = 0;
        for (; t + 8 <= T; t += 8) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p[t + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc += j == 2 ? (v[k] >= 1.0 ? 1.0 : 0.0) : v[k];
        }
        for (; t < T; ++t) {
            const double v = p[t];
            acc += j == 2 ? (v >= 1.0 ? 1.0 : 0.0) : v;
        }
        sh[j] = acc;
        if (chunk == 0) group_out[g * 3 + j] = acc;
    }
    if (!SCALE) return;
    __syncthreads();
    const double dof = sh[1] - sh[2];
    const double std_g = dof > 0.0 ? sqrt(sh[0] / dof) : 0.0;
    const float denom = rn_add((float)std_g, 1e-8f);
    const int32_t t0 = chunk * t_chunk;
    const int32_t tc = (T - t0) < t_chunk ? (T - t0) : t_chunk;
    constexpr int U = VEC ? 4 : 1;
    const int64_t total = (int64_t)tc * E;                                  // (tc > 1 only when E <= kSbScaleEntries / 2)
    const int64_t iters = (total + (int64_t)kSbBlock * U - 1) / ((int64_t)kSbBlock * U);
    const double* mean_g = tab + plane + g * T;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t j = (it * kSbBlock + threadIdx.x) * U;
        const bool ok = j < total;
        const int64_t jc = ok ? j : total - U;
        int32_t row = 0;
        int64_t e = jc;
        if (tc > 1) {
            row = (int32_t)((uint32_t)jc / (uint32_t)E);
            e = jc - (int64_t)row * E;
        }
        const int64_t flat = (int64_t)(t0 + row) * n + g * E + e;
        const float b = (float)mean_g[t0 + row];
        if (VEC) {
            const float4 r = *reinterpret_cast<const float4*>(R + flat);
            const uint32_t m = *reinterpret_cast<const uint32_t*>(mask + flat);
            float4 o;
            o.x = (m & 0x000000FFu) ? rn_div(rn_sub(r.x, b), denom) : 0.0f;
            o.y = (m & 0x0000FF00u) ? rn_div(rn_sub(r.y, b), denom) : 0.0f;
            o.z = (m & 0x00FF0000u) ? rn_div(rn_sub(r.z, b), denom) : 0.0f;
            o.w = (m & 0xFF000000u) ? rn_div(rn_sub(r.w, b), denom) : 0.0f;
            if (ok) *reinterpret_cast<float4*>(A + flat) = o;
        } else {
            const float r = R[flat];
            const uint8_t m = mask[flat];
            const float o = m ? rn_div(rn_sub(r, b), denom) : 0.0f;
            if (ok) A[flat] = o;
        }
    }
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_grpo_step_advantage(const float* d_rtg, const uint8_t* d_mask, int64_t n, int32_t T, int64_t group_size, int mode, double* d_work,
                           float* d_adv, double* d_group, void* stream) {
    TG_REQUIRE(d_rtg && d_mask && d_work && d_adv && d_group, "tg_grpo_step_advantage: null pointer");
    TG_REQUIRE(group_size >= 1, "tg_grpo_step_advantage: group_size %lld (>= 1)", (long long)group_size);
    TG_REQUIRE(n >= 0 && n % group_size == 0, "tg_grpo_step_advantage: n=%lld must be a multiple of group_size=%lld", (long long)n,
               (long long)group_size);
    TG_REQUIRE(T >= 1, "tg_grpo_step_advantage: horizon %d (>= 1)", T);
    TG_REQUIRE(mode == 0 || mode == 1, "tg_grpo_step_advantage: mode %d (0: residuals, 1: / (pooled std + 1e-8))", mode);
    if (n == 0) return TG_OK;
    const int64_t E = group_size, G = n / E, S = (int64_t)T * G;
    const int64_t nq = (E + 3) / 4;
    int log2_w = 0;
    while (log2_w < 6 && ((int64_t)1 << log2_w) < nq) ++log2_w;
    const int W = 1 << log2_w;
    const int32_t t_chunk = (int32_t)(E >= kSbScaleEntries ? 1 : (kSbScaleEntries / E < T ? kSbScaleEntries / E : T));
    const int32_t n_chunks = (int32_t)ceil_div(T, t_chunk);
    const int64_t blocks1 = ceil_div(S, kSbBlock / W), blocks2 = mode == 1 ? G * n_chunks : G;
    TG_REQUIRE(blocks1 <= 0x7FFFFFFF && blocks2 <= 0x7FFFFFFF, "tg_grpo_step_advantage: %lld x %d segments of %lld need more workgroups than a launch has",
               (long long)G, T, (long long)E);
    const bool vec = E % 4 == 0 && n % 4 == 0 && (((uintptr_t)d_rtg | (uintptr_t)d_adv) & 15) == 0 && ((uintptr_t)d_mask & 3) == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g1((unsigned)blocks1), g2((unsigned)blocks2), blk(kSbBlock);
#define TG_SB_SEGMENTS(V, D) hipLaunchKernelGGL((step_segments_kernel<V, D>), g1, blk, 0, st, d_rtg, d_mask, T, E, G, log2_w, d_work, d_adv)
    if (vec) { if (mode == 0) TG_SB_SEGMENTS(true, true); else TG_SB_SEGMENTS(true, false); }
    else     { if (mode == 0) TG_SB_SEGMENTS(false, true); else TG_SB_SEGMENTS(false, false); }
#undef TG_SB_SEGMENTS
    TG_LAUNCH_CHECK("tg_grpo_step_advantage(segments)");
    if (mode == 0)
        hipLaunchKernelGGL((step_scale_kernel<false, false>), g2, dim3(64), 0, st, d_rtg, d_mask, n, T, E, G, T, 1, d_work, d_adv, d_group);
    else if (vec)
        hipLaunchKernelGGL((step_scale_kernel<true, true>), g2, blk, 0, st, d_rtg, d_mask, n, T, E, G, t_chunk, n_chunks, d_work, d_adv, d_group);
    else
        hipLaunchKernelGGL((step_scale_kernel<false, true>), g2, blk, 0, st, d_rtg, d_mask, n, T, E, G, t_chunk, n_chunks, d_work, d_adv, d_group);
    TG_LAUNCH_CHECK("tg_grpo_step_advantage(scale)");
    return TG_OK;
}

}  // extern "C"
