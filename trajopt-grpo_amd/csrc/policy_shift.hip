// How far a learn() moved the policy, and the learning rate that follows from it (rsl_rl's schedule="adaptive").
//
// tg_policy_shift: one lane per row.  lp = the Gaussian log-probability of the row's action under the CURRENT means (float32, the row
// arithmetic of loss_row.hpp::gaussian_logp), d = (double)lp - (double)logp_old (exact), k3 = expm1(d) - d (Schulman's k3 estimator
// of KL(old || new), >= 0), clipped = d outside [log1p(-eps), log1p(eps)].  Each workgroup leaves ONE float64 [4] partial
// {rows, sum k3, clipped rows, sum d}: lanes -> wave (fixed shuffle tree) -> the four waves in wave order, no floating-point atomics.
// Workgroup b covers rows [b * 4096, (b + 1) * 4096) (grid-stride beyond 1024 workgroups): which rows a thread adds, and the order of
// every addition after that, depend on `rows` alone.
// tg_policy_shift_finish: one workgroup adds all partials in index order.  tg_lr_adapt: one thread, the rule in float64.
// tg_kl_control: the same thread's work for a check BETWEEN the updates of a learn(): the rule on the rate held in a device control
// block, and target_kl's latch, which the optimizer launches that follow read (optim_kernels.hip: adam_ctl_kernel).
#include "loss_row.hpp"

namespace tg {

constexpr int kShiftThreads = 256, kShiftPerThread = 16, kShiftChunk = kShiftThreads * kShiftPerThread, kShiftMaxBlocks = 1024;

static inline int64_t shift_blocks(int64_t rows) {
    return rows <= 0 ? 0 : (ceil_div(rows, kShiftChunk) < kShiftMaxBlocks ? ceil_div(rows, kShiftChunk) : kShiftMaxBlocks);
}

struct ShiftK {
    const float* mean; int64_t mean_rs;
    const float* act; int64_t act_rs, act_cs;
    const float* logp_old;
    Var8 v;
    const float* log_std;       // kStd only: device log_std [A]
    double log_lo, log_hi;
    int64_t rows;
    double* partial;            // this launch's first slot: f64 [gridDim.x][4]
};

// kStd: inv_var / logp_const are formed here from the device's log_std, as the training heads form them.
// kVec (A a multiple of 4, 16-B aligned unit-stride rows): the means and the actions of a row arrive as float4 loads.
template <int A, bool kStd, bool kVec>
__global__ __launch_bounds__(kShiftThreads) void policy_shift_kernel(ShiftK p) {
    static_assert(!kStd || A <= 4, "a learned log-std has at most four columns");
    static_assert(!kVec || A % 4 == 0, "float4 loads need whole groups of four columns");
    // (a host variance is read from the kernel arguments where it lies: a private copy of Var8, indexed at run time by
    // gaussian_logp()'s partly unrolled loop when A > 4, would be placed in LDS)
    [[maybe_unused]] Var8 v_std = {};
    if constexpr (kStd) {
        const Gauss4 G = gauss4_from_log_std([&](int k) { return p.log_std[k]; }, A, Gauss4{});
#pragma unroll
        for (int k = 0; k < A; ++k) v_std.inv_var[k] = G.inv_var[k];
        v_std.logp_const = G.logp_const;
    }
    const Var8& v = [&]() -> const Var8& {
        if constexpr (kStd) return v_std;
        else return p.v;
    }();
    double s_cnt = 0, s_k3 = 0, s_clip = 0, s_d = 0;
    for (int64_t base = (int64_t)blockIdx.x * kShiftChunk; base < p.rows; base += (int64_t)gridDim.x * kShiftChunk) {
#pragma unroll 4
        for (int k16 = 0; k16 < kShiftPerThread; ++k16) {       // (consecutive lanes, consecutive rows)
            const int64_t i = base + k16 * kShiftThreads + threadIdx.x;
            if (i >= p.rows) continue;
            float mu[A], a[A];
            if constexpr (kVec) {
#pragma unroll
                for (int q = 0; q < A / 4; ++q) {
                    const float4 m4 = *reinterpret_cast<const float4*>(p.mean + i * p.mean_rs + 4 * q);
                    const float4 a4 = *reinterpret_cast<const float4*>(p.act + i * p.act_rs + 4 * q);
                    mu[4 * q] = m4.x; mu[4 * q + 1] = m4.y; mu[4 * q + 2] = m4.z; mu[4 * q + 3] = m4.w;
                    a[4 * q] = a4.x; a[4 * q + 1] = a4.y; a[4 * q + 2] = a4.z; a[4 * q + 3] = a4.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < A; ++k) { mu[k] = p.mean[i * p.mean_rs + k]; a[k] = p.act[i * p.act_rs + k * p.act_cs]; }
            }
            const float lp = gaussian_logp(mu, a, v, A);
            const double d = (double)lp - (double)p.logp_old[i];
            s_cnt += 1.0;
            s_k3 += expm1(d) - d;
            s_clip += (d < p.log_lo || d > p.log_hi) ? 1.0 : 0.0;
            s_d += d;
        }
    }
    double acc[4] = {s_cnt, s_k3, s_clip, s_d};
    const double t = block_sum4_f64(acc);
    if (threadIdx.x < 4) p.partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = t;
}

// all chunks' partials, column j by thread j, in index order
__global__ __launch_bounds__(64) void policy_shift_finish_kernel(const double* __restrict__ partial, int32_t n_partials, double* __restrict__ sums) {
    const int j = threadIdx.x;
    if (j >= 4) return;
    double t = 0.0;
    for (int32_t b = 0; b < n_partials; ++b) t += partial[(int64_t)b * 4 + j];
    sums[j] = t;
}

// out4 = {kl, clip_fraction, lr_in, lr_out}.  Every comparison with a NaN is false: the rate stays.
__global__ __launch_bounds__(64) void lr_adapt_kernel(const double* __restrict__ sums, double desired_kl, double factor, double lr_min,
                                                      double lr_max, double lr, double* __restrict__ out4) {
    if (threadIdx.x != 0) return;
    const double rows = sums[0];
    const double kl = sums[1] / rows, clip_fraction = sums[2] / rows;
    double lr_out = lr;
    if (desired_kl > 0.0 && rows > 0.0) {
        if (kl > 2.0 * desired_kl) lr_out = fmax(lr / factor, lr_min);
        else if (kl < 0.5 * desired_kl) lr_out = fmin(lr * factor, lr_max);
    }
    out4[0] = kl; out4[1] = clip_fraction; out4[2] = lr; out4[3] = lr_out;
}

// ctl f64 [8] = {stopped, lr, stop_update, kl_at_stop, last_kl, last_clip_fraction, checks, 0}.  A latched block is left as it is,
// byte for byte; else tg_lr_adapt's rule on ctl[1] (the check that latches applies it too), then the latch.  A NaN kl or rows == 0
// neither adapts nor stops: every comparison is false.
__global__ __launch_bounds__(64) void kl_control_kernel(const double* __restrict__ sums, double target_kl, double stop_factor,
                                                        double desired_kl, double factor, double lr_min, double lr_max, double update,
                                                        double* __restrict__ ctl) {
    if (threadIdx.x != 0) return;
    if (ctl[0] != 0.0) return;
    const double rows = sums[0];
    const double kl = sums[1] / rows, clip_fraction = sums[2] / rows;
    const double lr = ctl[1];
    double lr_out = lr;
    if (desired_kl > 0.0 && rows > 0.0) {
        if (kl > 2.0 * desired_kl) lr_out = fmax(lr / factor, lr_min);
        else if (kl < 0.5 * desired_kl) lr_out = fmin(lr * factor, lr_max);
    }
    ctl[1] = lr_out; ctl[4] = kl; ctl[5] = clip_fraction; ctl[6] = ctl[6] + 1.0; ctl[7] = 0.0;
    if (target_kl > 0.0 && rows > 0.0 && kl > stop_factor * target_kl) { ctl[0] = 1.0; ctl[2] = update; ctl[3] = kl; }
}

template <int A, bool kStd>
static void launch_shift_std(const ShiftK& k, unsigned grid, bool vec, hipStream_t st) {
    if constexpr (A % 4 == 0) {
        if (vec) {
            hipLaunchKernelGGL((policy_shift_kernel<A, kStd, true>), dim3(grid), dim3(kShiftThreads), 0, st, k);
            return;
        }
    }
    hipLaunchKernelGGL((policy_shift_kernel<A, kStd, false>), dim3(grid), dim3(kShiftThreads), 0, st, k);
}

template <int A>
static void launch_shift(const ShiftK& k, unsigned grid, bool vec, hipStream_t st) {
    if constexpr (A <= 4) {
        if (k.log_std != nullptr) {
            launch_shift_std<A, true>(k, grid, vec, st);
            return;
        }
    }
    launch_shift_std<A, false>(k, grid, vec, st);
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_policy_shift_blocks(int64_t rows) { return (int)shift_blocks(rows); }

int tg_policy_shift(const float* d_mean, int64_t mean_row_stride, const float* d_act, int64_t act_row_stride, int64_t act_col_stride,
                    const float* d_logp_old, const float* var, const float* d_log_std, int act_dim, double log_lo, double log_hi,
                    int64_t rows, double* d_partials, int64_t slot, void* stream) {
    TG_REQUIRE(rows >= 0 && slot >= 0, "tg_policy_shift: bad sizes (rows %lld, slot %lld)", (long long)rows, (long long)slot);
    TG_REQUIRE((var != nullptr) != (d_log_std != nullptr), "tg_policy_shift: exactly one of var (host) and d_log_std (device) must be given");
    TG_REQUIRE(log_lo <= 0.0 && log_hi >= 0.0, "tg_policy_shift: the clip range [%g, %g] of the log-ratio must contain 0", log_lo, log_hi);
    ShiftK k;
    if (d_log_std != nullptr) {
        TG_REQUIRE(act_dim >= 1 && act_dim <= 4, "tg_policy_shift: a device log_std needs 1..4 action dimensions, got %d", act_dim);
        k.v = Var8{};                               // (formed on the device from log_std)
    } else {
        int rc = make_var(var, act_dim, k.v, "tg_policy_shift");
        if (rc != TG_OK) return rc;
    }
    if (rows == 0) return TG_OK;                    // (no partial: tg_policy_shift_blocks(0) == 0)
    TG_REQUIRE(d_mean && d_act && d_logp_old && d_partials, "tg_policy_shift: null pointer");
    TG_REQUIRE(mean_row_stride >= act_dim, "tg_policy_shift: mean_row_stride %lld < act_dim %d", (long long)mean_row_stride, act_dim);
    TG_REQUIRE(((uintptr_t)d_partials & 7) == 0, "tg_policy_shift: the partials are not 8-B aligned");
    k.mean = d_mean; k.mean_rs = mean_row_stride;
    k.act = d_act; k.act_rs = act_row_stride; k.act_cs = act_col_stride;
    k.logp_old = d_logp_old; k.log_std = d_log_std;
    k.log_lo = log_lo; k.log_hi = log_hi; k.rows = rows;
    k.partial = d_partials + slot * 4;
    const bool vec = act_dim % 4 == 0 && ((uintptr_t)d_mean & 15) == 0 && mean_row_stride % 4 == 0 && ((uintptr_t)d_act & 15) == 0 &&
                     act_col_stride == 1 && act_row_stride % 4 == 0 && act_row_stride >= act_dim;
    const unsigned grid = (unsigned)shift_blocks(rows);
    hipStream_t st = (hipStream_t)stream;
#define L(AA)                                   \
    case AA:                                    \
        launch_shift<AA>(k, grid, vec, st);     \
        break;
    switch (act_dim) { L(1) L(2) L(3) L(4) L(5) L(6) L(7) L(8) }
#undef L
    TG_LAUNCH_CHECK("tg_policy_shift");
    return TG_OK;
}

int tg_policy_shift_finish(const double* d_partials, int32_t n_partials, double* d_sums, void* stream) {
    TG_REQUIRE(n_partials >= 0 && d_sums && (n_partials == 0 || d_partials), "tg_policy_shift_finish: bad arguments");
    hipLaunchKernelGGL(policy_shift_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_partials, n_partials, d_sums);
    TG_LAUNCH_CHECK("tg_policy_shift_finish");
    return TG_OK;
}

int tg_lr_adapt(const double* d_sums, double desired_kl, double factor, double lr_min, double lr_max, double lr, double* d_out4, void* stream) {
    TG_REQUIRE(d_sums && d_out4, "tg_lr_adapt: null pointer");
    // (desired_kl <= 0: measure only, the bounds and the factor are not looked at)
    TG_REQUIRE(!(desired_kl > 0.0) || (factor > 1.0 && lr_min <= lr_max), "tg_lr_adapt: factor = %g must be > 1 and lr_min = %g <= lr_max = %g",
               factor, lr_min, lr_max);
    hipLaunchKernelGGL(lr_adapt_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_sums, desired_kl, factor, lr_min, lr_max, lr, d_out4);
    TG_LAUNCH_CHECK("tg_lr_adapt");
    return TG_OK;
}

int tg_kl_control(const double* d_sums, double target_kl, double stop_factor, double desired_kl, double factor, double lr_min,
                  double lr_max, int64_t update, double* d_ctl, void* stream) {
    TG_REQUIRE(d_sums && d_ctl, "tg_kl_control: null pointer");
    TG_REQUIRE(((uintptr_t)d_sums & 7) == 0 && ((uintptr_t)d_ctl & 7) == 0, "tg_kl_control: the sums / the control block are not 8-B aligned");
    // (target_kl <= 0: never stops, stop_factor is not looked at; desired_kl <= 0: the rate stays, the bounds and the factor are not)
    TG_REQUIRE(!(target_kl > 0.0) || (__builtin_isfinite(target_kl) && __builtin_isfinite(stop_factor) && stop_factor > 0.0),
               "tg_kl_control: target_kl = %g must be finite and stop_factor = %g finite and > 0", target_kl, stop_factor);
    TG_REQUIRE(!(desired_kl > 0.0) || (factor > 1.0 && lr_min <= lr_max), "tg_kl_control: factor = %g must be > 1 and lr_min = %g <= lr_max = %g",
               factor, lr_min, lr_max);
    TG_REQUIRE(target_kl == target_kl && desired_kl == desired_kl, "tg_kl_control: target_kl / desired_kl is NaN");
    TG_REQUIRE(update >= 1 && update < ((int64_t)1 << 53), "tg_kl_control: update = %lld must be the 1-based count of optimizer steps", (long long)update);
    hipLaunchKernelGGL(kl_control_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_sums, target_kl, stop_factor, desired_kl, factor, lr_min,
                       lr_max, (double)update, d_ctl);
    TG_LAUNCH_CHECK("tg_kl_control");
    return TG_OK;
}

}  // extern "C"
