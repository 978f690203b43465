// Policy evaluation on the device (include/trajopt_grpo_hip.h, "Deterministic evaluation and parameter sweeps"): the parameter grid
// as a source of the per-env table, the initial states of cell 0 copied to every cell, and per-cell episode statistics in a fixed
// summation order.  One lane per environment everywhere: env is the fastest index of every trajectory array, so a wavefront's
// access is one coalesced 256-B (f32) / 512-B (f64) line per row.  No floating-point atomics, no scratch; the only LDS is the
// cell reduction's.  tests/evaluation_fp64.py restates the grid decode and the statistics bit for bit.
#include "tg_common.hpp"

#include <string.h>

namespace tg {

// ---------------------------------------------------------------------------
// tg_env_param_grid
// ---------------------------------------------------------------------------
// The swept parameters sorted by their p[] index (the host sorts: the decode does not depend on the order they were listed in);
// first[k] = where parameter k's factor list starts in d_values.
struct GridSorted {
    double  nominal[12];
    int32_t count;
    int32_t index[12];
    int32_t levels[12];
    int32_t first[12];
};

__global__ __launch_bounds__(256) void env_param_grid_kernel(GridSorted g, const double* __restrict__ values, double* __restrict__ ptab,
                                                             int64_t n, int64_t env_offset, int64_t episodes_per_cell) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t rem = (env_offset + i) / episodes_per_cell;                     // the cell, row-major: the LAST swept parameter runs fastest
    double factor[12];
#pragma unroll
    for (int k = 11; k >= 0; --k) {
        factor[k] = 1.0;
        if (k < g.count) {                                                  // (uniform)
            const int64_t lv = rem % g.levels[k];
            rem /= g.levels[k];
            factor[k] = values[g.first[k] + lv];
        }
    }
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        double v = g.nominal[r];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < g.count && g.index[k] == r) v = g.nominal[r] * factor[k];
        ptab[r * n + i] = v;
    }
}

// ---------------------------------------------------------------------------
// tg_eval_tile_states
// ---------------------------------------------------------------------------
// obs[k][0][i] = obs[k][0][i % E] for E <= i < n: the reads touch slots < E only, the writes slots >= E only.
template <typename R>
__global__ __launch_bounds__(256) void eval_tile_states_kernel(R* __restrict__ obs, int64_t n, int64_t T1, int64_t E) {
    const int64_t i = E + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t row = (int64_t)blockIdx.y * T1 * n;                       // feature k = blockIdx.y, time slot 0
    obs[row + i] = obs[row + i % E];
}

// ---------------------------------------------------------------------------
// tg_eval_cells
// ---------------------------------------------------------------------------
// First launch: lane i sums its episode's rewards in f64, t ascending.  A slot without a finished episode gets 0.
template <typename R>
__global__ __launch_bounds__(256) void eval_returns_kernel(const R* __restrict__ rew, const int32_t* __restrict__ len, int64_t n, int32_t T,
                                                           double* __restrict__ returns) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t L = len[i];
    double acc = 0.0;
    if (L >= 1 && L <= T) {
        // eight rows in flight per lane; a row at or beyond L adds +0.0, which leaves every bit of the sum as it is (the sum starts
        // at +0.0, so it is never -0.0)
        for (int32_t t0 = 0; t0 < L; t0 += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = t0 + u < L ? (double)rew[(int64_t)(t0 + u) * n + i] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
    }
    returns[i] = acc;
}

// Second launch: one workgroup of 256 threads per cell.  Thread j folds the counted episodes e = j, j + 256, j + 512, ... of the
// cell, in that order, into its own partial; the 256 partials are then added pairwise, partial[j] += partial[j + s] for
// s = 128, 64, ..., 1.  The same order for every column; the integer columns are exact in any order.
constexpr int kCellThreads = 256;
__global__ __launch_bounds__(kCellThreads) void eval_cells_kernel(const double* __restrict__ returns, const int32_t* __restrict__ len,
                                                                  const uint8_t* __restrict__ timeout, int64_t E, int32_t T,
                                                                  double* __restrict__ cells) {
#pragma clang fp contract(off)
    __shared__ double s_sum[kCellThreads], s_sq[kCellThreads], s_min[kCellThreads], s_max[kCellThreads];
    __shared__ unsigned long long s_cnt[kCellThreads], s_len[kCellThreads], s_to[kCellThreads];
    const int j = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * E;
    double sum = 0.0, sq = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    unsigned long long cnt = 0, ln = 0, to = 0;
    for (int64_t e = j; e < E; e += kCellThreads) {
        const int32_t L = len[base + e];
        if (L >= 1 && L <= T) {
            const double r = returns[base + e];
            sum += r;
            sq += r * r;
            mn = r < mn ? r : mn;
            mx = r > mx ? r : mx;
            cnt += 1;
            ln += (unsigned long long)L;
            to += timeout[base + e] != 0;
        }
    }
    s_sum[j] = sum; s_sq[j] = sq; s_min[j] = mn; s_max[j] = mx;
    s_cnt[j] = cnt; s_len[j] = ln; s_to[j] = to;
    __syncthreads();
    for (int s = kCellThreads / 2; s > 0; s >>= 1) {
        if (j < s) {
            s_sum[j] += s_sum[j + s];
            s_sq[j] += s_sq[j + s];
            s_min[j] = s_min[j + s] < s_min[j] ? s_min[j + s] : s_min[j];
            s_max[j] = s_max[j + s] > s_max[j] ? s_max[j + s] : s_max[j];
            s_cnt[j] += s_cnt[j + s];
            s_len[j] += s_len[j + s];
            s_to[j] += s_to[j + s];
        }
        __syncthreads();
    }
    if (j == 0) {
        double* out = cells + (int64_t)blockIdx.x * 8;
        out[0] = (double)s_cnt[0];
        out[1] = s_sum[0];
        out[2] = s_sq[0];
        out[3] = s_min[0];
        out[4] = s_max[0];
        out[5] = (double)s_len[0];
        out[6] = (double)s_to[0];
        out[7] = (double)(s_cnt[0] - s_to[0]);
    }
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_env_param_grid(const tg_env_params* p, const tg_param_grid* g, double* d_ptab, int64_t n, int64_t env_offset, void* stream) {
    TG_REQUIRE(p && g, "tg_env_param_grid: null pointer");
    TG_REQUIRE(d_ptab != nullptr, "tg_env_param_grid: null parameter table");
    TG_REQUIRE(g->count >= 0 && g->count <= 12, "tg_env_param_grid: count=%d outside [0, 12]", g->count);
    TG_REQUIRE(g->count == 0 || g->d_values != nullptr, "tg_env_param_grid: null factor list");
    const int64_t E = g->episodes_per_cell;
    TG_REQUIRE(E >= 1, "tg_env_param_grid: episodes_per_cell=%lld < 1", (long long)E);
    TG_REQUIRE(n >= 0 && env_offset >= 0, "tg_env_param_grid: bad sizes n=%lld env_offset=%lld", (long long)n, (long long)env_offset);
    TG_REQUIRE(n % E == 0, "tg_env_param_grid: n=%lld is not a multiple of episodes_per_cell=%lld", (long long)n, (long long)E);
    int64_t cells = 1;
    int32_t first[12], total = 0;
    for (int k = 0; k < g->count; ++k) {
        TG_REQUIRE(g->index[k] >= 0 && g->index[k] < 12, "tg_env_param_grid: index[%d]=%d outside p[0..11]", k, g->index[k]);
        for (int j = 0; j < k; ++j) TG_REQUIRE(g->index[j] != g->index[k], "tg_env_param_grid: p[%d] listed twice", g->index[k]);
        TG_REQUIRE(g->levels[k] >= 1, "tg_env_param_grid: levels[%d]=%d < 1", k, g->levels[k]);
        TG_REQUIRE(g->levels[k] <= (1 << 20) && cells <= (int64_t)1 << 40, "tg_env_param_grid: the grid is too large");
        cells *= g->levels[k];
        first[k] = total;
        total += g->levels[k];
    }
    TG_REQUIRE((env_offset + n) / E <= cells, "tg_env_param_grid: envs [%lld, %lld) reach beyond the grid's %lld cells of %lld episodes",
               (long long)env_offset, (long long)(env_offset + n), (long long)cells, (long long)E);
    if (n == 0) return TG_OK;
    GridSorted s;
    memset(&s, 0, sizeof(s));
    memcpy(s.nominal, p->p, sizeof(s.nominal));
    s.count = g->count;
    int order[12];
    for (int k = 0; k < g->count; ++k) order[k] = k;
    for (int a = 1; a < g->count; ++a)                                      // insertion sort by p[] index
        for (int b = a; b > 0 && g->index[order[b]] < g->index[order[b - 1]]; --b) {
            const int tmp = order[b]; order[b] = order[b - 1]; order[b - 1] = tmp;
        }
    for (int k = 0; k < g->count; ++k) {
        s.index[k] = g->index[order[k]];
        s.levels[k] = g->levels[order[k]];
        s.first[k] = first[order[k]];
    }
    hipLaunchKernelGGL(env_param_grid_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, s, g->d_values, d_ptab, n,
                       env_offset, E);
    TG_LAUNCH_CHECK("tg_env_param_grid");
    return TG_OK;
}

int tg_eval_tile_states(const tg_traj* tr, int32_t S, int64_t episodes_per_cell, void* stream) {
    TG_REQUIRE(tr && tr->d_obs, "tg_eval_tile_states: null pointer");
    TG_REQUIRE(tr->dtype == TG_F32 || tr->dtype == TG_F64, "tg_eval_tile_states: bad dtype %d", tr->dtype);
    TG_REQUIRE(tr->n > 0 && tr->horizon > 0 && S >= 1 && S <= 65535, "tg_eval_tile_states: bad sizes n=%lld T=%d S=%d", (long long)tr->n,
               tr->horizon, S);
    const int64_t E = episodes_per_cell;
    TG_REQUIRE(E >= 1 && tr->n % E == 0, "tg_eval_tile_states: n=%lld is not a multiple of episodes_per_cell=%lld", (long long)tr->n,
               (long long)E);
    if (tr->n == E) return TG_OK;                                          // one cell: nothing to copy
    const dim3 grid((unsigned)ceil_div(tr->n - E, 256), (unsigned)S);
    const int64_t T1 = (int64_t)tr->horizon + 1;
    if (tr->dtype == TG_F32)
        hipLaunchKernelGGL(eval_tile_states_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (float*)tr->d_obs, tr->n, T1, E);
    else
        hipLaunchKernelGGL(eval_tile_states_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (double*)tr->d_obs, tr->n, T1, E);
    TG_LAUNCH_CHECK("tg_eval_tile_states");
    return TG_OK;
}

int tg_eval_cells(const tg_traj* tr, const uint8_t* d_timeout, int64_t episodes_per_cell, double* d_returns, double* d_cells,
                  void* stream) {
    TG_REQUIRE(tr && tr->d_rew && tr->d_len && d_timeout && d_returns && d_cells, "tg_eval_cells: null pointer");
    TG_REQUIRE(tr->dtype == TG_F32 || tr->dtype == TG_F64, "tg_eval_cells: bad dtype %d", tr->dtype);
    TG_REQUIRE(tr->n > 0 && tr->horizon > 0, "tg_eval_cells: bad sizes n=%lld T=%d", (long long)tr->n, tr->horizon);
    const int64_t E = episodes_per_cell;
    TG_REQUIRE(E >= 1 && tr->n % E == 0, "tg_eval_cells: n=%lld is not a multiple of episodes_per_cell=%lld", (long long)tr->n, (long long)E);
    const int64_t C = tr->n / E;
    TG_REQUIRE(C <= 0x7FFFFFFF, "tg_eval_cells: %lld cells", (long long)C);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(tr->n, 256));
    if (tr->dtype == TG_F32)
        hipLaunchKernelGGL(eval_returns_kernel<float>, grid, dim3(256), 0, st, (const float*)tr->d_rew, tr->d_len, tr->n, tr->horizon, d_returns);
    else
        hipLaunchKernelGGL(eval_returns_kernel<double>, grid, dim3(256), 0, st, (const double*)tr->d_rew, tr->d_len, tr->n, tr->horizon, d_returns);
    TG_LAUNCH_CHECK("tg_eval_cells(returns)");
    hipLaunchKernelGGL(eval_cells_kernel, dim3((unsigned)C), dim3(kCellThreads), 0, st, (const double*)d_returns, tr->d_len, d_timeout, E,
                       tr->horizon, d_cells);
    TG_LAUNCH_CHECK("tg_eval_cells");
    return TG_OK;
}

}  // extern "C"
