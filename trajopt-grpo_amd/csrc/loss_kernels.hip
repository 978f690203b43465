// Gaussian log-prob and the fused clipped-surrogate loss (forward + backward in one pass).
//
// One lane per sample.  The kernel reads the policy mean (GEMM output), the action, the
// old log-prob and the advantage (and value / return for PPO), forms
//   logp, rho = exp(logp - logp_old), min(rho A, clip(rho) A), (V - R)^2, exp(lp_old)(lp_old - lp)
// and writes d(total)/d(mean) (and d/dV) directly, so the whole loss head costs one read of
// its inputs and one write of the gradient instead of ~15 elementwise launches.
// Loss scalars are reduced deterministically: wavefront shuffle -> per-block partial in
// fp64 -> fixed-order final pass (no float atomics).
#include "loss_row.hpp"

namespace tg {

constexpr int kLossBlocks = 1024;   // persistent grid-stride blocks
constexpr int kLossThreads = 256;

// (Var8, gaussian_logp(), make_var() and block_sum4_f64() are loss_row.hpp's: policy_shift.hip compiles them too)

template <int A>
__global__ __launch_bounds__(256) void gaussian_logp_kernel(const float* __restrict__ mean, int64_t mean_rs,
                                                            const float* __restrict__ act, int64_t act_rs, int64_t act_cs,
                                                            Var8 v, float* __restrict__ logp, int64_t M) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        float mu[A], a[A];
#pragma unroll
        for (int k = 0; k < A; ++k) { mu[k] = mean[i * mean_rs + k]; a[k] = act[i * act_rs + k * act_cs]; }
        logp[i] = gaussian_logp(mu, a, v, A);
    }
}

struct LossK {
    const float* mean; int64_t mean_rs;
    const float* act; int64_t act_rs, act_cs;
    const float* logp_old; const float* adv; const float* value; const float* ret;
    const uint8_t* mask; const float* norm; const float* coef;
    Var8 v;
    float epsilon, surr_coef, critic_coef, kl_coef;
    float* grad_mean; float* grad_value; double* work; int64_t M;
    const float* logp_ref; float ref_coef;      // kRef only (tg_ref_penalty)
    const float* log_std; float* std_out;       // kStd only (tg_learned_std): device log_std [A]; out f32 [M][4]
};

// The row arithmetic is loss_row.hpp's; here: the A-templated strided loads, the mask, the stores and the f64 sums.
// kRef: GRPO's KL penalty to a frozen reference policy (tg_surrogate_loss_ref)
// kStd: the policy's learned log-std (tg_surrogate_loss_std): inv_var / logp_const are formed here from the device's log_std, and
// the row's contribution to d total / d log_std goes to std_out[row][4] (zeros for a masked row)
template <int A, bool kRef = false, bool kStd = false>
__global__ __launch_bounds__(256) void surrogate_loss_kernel(LossK p) {
    static_assert(!kStd || A <= 4, "a learned log-std has at most four columns");
    Var8 v = p.v;
    if constexpr (kStd) {
        const Gauss4 G = gauss4_from_log_std([&](int k) { return p.log_std[k]; }, A, Gauss4{});
#pragma unroll
        for (int k = 0; k < A; ++k) v.inv_var[k] = G.inv_var[k];
        v.logp_const = G.logp_const;
    }
    double s_surr = 0, s_crit = 0, s_kl = 0, s_cnt = 0;
    float n_am = 0.f, n_ai = 1.f, n_rm = 0.f, n_ri = 1.f;
    if (p.norm != nullptr) { n_am = p.norm[0]; n_ai = p.norm[1]; n_rm = p.norm[2]; n_ri = p.norm[3]; }
    // (locals: writing into the by-value argument struct would send it to scratch)
    float surr_coef = p.surr_coef, critic_coef = p.critic_coef, kl_coef = p.kl_coef;
    if (p.coef != nullptr) { surr_coef = p.coef[0]; critic_coef = p.coef[1]; kl_coef = p.coef[2]; }
    [[maybe_unused]] const float ref_coef = kRef ? p.ref_coef : 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.M; i += (int64_t)gridDim.x * blockDim.x) {
        const bool valid = p.mask == nullptr || p.mask[i] != 0;
        float g[A];
#pragma unroll
        for (int k = 0; k < A; ++k) g[k] = 0.0f;
        float gv = 0.0f;
        [[maybe_unused]] float gs[4] = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
            float mu[A], a[A];
#pragma unroll
            for (int k = 0; k < A; ++k) { mu[k] = p.mean[i * p.mean_rs + k]; a[k] = p.act[i * p.act_rs + k * p.act_cs]; }
            const float lp = gaussian_logp(mu, a, v, A);
            float lref = 0.f;
            if constexpr (kRef) lref = p.logp_ref[i];
            const ActorTerms t = loss_actor_terms<kRef>(lp, p.logp_old[i], (p.adv[i] - n_am) * n_ai, p.epsilon, surr_coef, kl_coef, lref, ref_coef);
            s_surr += (double)t.c_surr;
            // (the old-policy term and the reference term are added in float first: ref_penalty_check refuses kl_coef != 0 beside a
            // reference penalty, so at most one of the two is ever non-zero and the sum is that term's own value)
            s_kl += (double)t.c_kl;
#pragma unroll
            for (int k = 0; k < A; ++k) g[k] = gauss_mean_grad(t.dlp, a[k] - mu[k], v.inv_var[k]);   // d logp / d mu_k
            if constexpr (kStd) {
#pragma unroll
                for (int k = 0; k < A; ++k) gs[k] = gauss_log_std_grad(t.dlp, a[k] - mu[k], v.inv_var[k]);
            }
            if (p.value != nullptr) {
                const CriticTerms c = loss_critic_terms(p.value[i], p.ret[i], n_rm, n_ri, critic_coef);
                s_crit += (double)c.c_crit;
                gv = c.g0;
            }
            s_cnt += 1.0;
        }
#pragma unroll
        for (int k = 0; k < A; ++k) p.grad_mean[i * A + k] = g[k];
        if (p.grad_value != nullptr) p.grad_value[i] = gv;
        if constexpr (kStd) *reinterpret_cast<float4*>(p.std_out + i * 4) = float4{gs[0], gs[1], gs[2], gs[3]};
    }
    double acc[4] = {s_surr, s_crit, s_kl, s_cnt};
    const double t = block_sum4_f64(acc);
    if (threadIdx.x < 4) p.work[(int64_t)blockIdx.x * 4 + threadIdx.x] = t;
}

__global__ __launch_bounds__(256) void loss_final_kernel(const double* __restrict__ work, int nblocks, double* __restrict__ sums) {
    double acc[4] = {0, 0, 0, 0};
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += work[(int64_t)b * 4 + j];
    }
    const double t = block_sum4_f64(acc);
    if (threadIdx.x < 4) sums[threadIdx.x] = t;
}

// d loss / d log_std: column sums of the heads' [rows][4] side output in f64, fixed order: a grid-stride pass into per-block
// partials, then one block adds the partials in index order and ADDS the result (+ `add`) into the gradient window.
constexpr int kStdBlocks = 256;

__global__ __launch_bounds__(256) void log_std_partial_kernel(const float4* __restrict__ rows4, int64_t rows, double* __restrict__ work) {
    double acc[4] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 r = rows4[i];
        acc[0] += (double)r.x; acc[1] += (double)r.y; acc[2] += (double)r.z; acc[3] += (double)r.w;
    }
    const double t = block_sum4_f64(acc);
    if (threadIdx.x < 4) work[(int64_t)blockIdx.x * 4 + threadIdx.x] = t;
}

__global__ __launch_bounds__(64) void log_std_final_kernel(const double* __restrict__ work, int nblocks, int A, float add, float* __restrict__ grad) {
    const int j = threadIdx.x;
    if (j >= A) return;
    double t = 0.0;
    for (int b = 0; b < nblocks; ++b) t += work[(int64_t)b * 4 + j];
    grad[j] = (float)((double)grad[j] + t + (double)add);
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_loss_work_blocks(void) { return kLossBlocks; }

int tg_gaussian_logp(const float* d_mean, int64_t mean_row_stride, const float* d_act, int64_t act_row_stride,
                     int64_t act_col_stride, const float* var, int act_dim, float* d_logp, int64_t M, void* stream) {
    TG_REQUIRE(d_mean && d_act && var && d_logp, "tg_gaussian_logp: null pointer");
    TG_REQUIRE(M >= 0 && mean_row_stride >= act_dim, "tg_gaussian_logp: bad sizes");
    Var8 v;
    int rc = make_var(var, act_dim, v, "tg_gaussian_logp");
    if (rc != TG_OK) return rc;
    if (M == 0) return TG_OK;
    const unsigned grid = (unsigned)(ceil_div(M, 256) < 4096 ? ceil_div(M, 256) : 4096);
    hipStream_t st = (hipStream_t)stream;
#define L(AA)                                                                                                          \
    case AA:                                                                                                           \
        hipLaunchKernelGGL(gaussian_logp_kernel<AA>, dim3(grid), dim3(256), 0, st, d_mean, mean_row_stride, d_act,      \
                           act_row_stride, act_col_stride, v, d_logp, M);                                              \
        break;
    switch (act_dim) { L(1) L(2) L(3) L(4) L(5) L(6) L(7) L(8) }
#undef L
    TG_LAUNCH_CHECK("tg_gaussian_logp");
    return TG_OK;
}

static int surrogate_loss(const tg_loss_args* a, const tg_ref_penalty* ref, void* stream, const tg_learned_std* std = nullptr) {
    TG_REQUIRE(a != nullptr, "tg_surrogate_loss: null args");
    const int use_ref = ref_penalty_check(ref, a->d_value != nullptr, a->kl_coef, "tg_surrogate_loss_ref");
    if (use_ref < 0) return use_ref;
    // (PPO's per-layer path scores actor and critic in one launch: a learned log-std is refused only for a head without actions)
    const int use_std = learned_std_check(std, a->d_act == nullptr, a->act_dim, "tg_surrogate_loss_std");
    if (use_std < 0) return use_std;
    TG_REQUIRE(a->d_mean && a->d_act && a->d_logp_old && a->d_adv && a->d_grad_mean && a->d_sums && a->d_work,
               "tg_surrogate_loss: null pointer");
    TG_REQUIRE((a->d_value == nullptr) == (a->d_ret == nullptr), "tg_surrogate_loss: value and ret go together");
    TG_REQUIRE(a->d_value == nullptr || a->d_grad_value != nullptr, "tg_surrogate_loss: grad_value missing");
    TG_REQUIRE(a->M >= 0 && a->mean_row_stride >= a->act_dim, "tg_surrogate_loss: bad sizes");
    LossK k;
    if (use_std) {
        k.v = Var8{};                               // (formed on the device from log_std)
    } else {
        int rc = make_var(a->var, a->act_dim, k.v, "tg_surrogate_loss");
        if (rc != TG_OK) return rc;
    }
    k.log_std = use_std ? std->d_log_std : nullptr; k.std_out = use_std ? std->d_out : nullptr;
    k.mean = a->d_mean; k.mean_rs = a->mean_row_stride;
    k.act = a->d_act; k.act_rs = a->act_row_stride; k.act_cs = a->act_col_stride;
    k.logp_old = a->d_logp_old; k.adv = a->d_adv; k.value = a->d_value; k.ret = a->d_ret;
    k.mask = a->d_mask; k.norm = a->d_norm; k.coef = a->d_coef;
    k.epsilon = a->epsilon; k.surr_coef = a->surr_coef; k.critic_coef = a->critic_coef; k.kl_coef = a->kl_coef;
    k.grad_mean = a->d_grad_mean; k.grad_value = a->d_grad_value; k.work = a->d_work; k.M = a->M;
    k.logp_ref = use_ref ? ref->d_logp_ref : nullptr; k.ref_coef = use_ref ? ref->coef : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    int64_t nb = ceil_div(a->M > 0 ? a->M : 1, kLossThreads);
    const unsigned grid = (unsigned)(nb < kLossBlocks ? nb : kLossBlocks);
#define L(AA)                                                                                            \
    case AA:                                                                                             \
        if (use_ref) hipLaunchKernelGGL((surrogate_loss_kernel<AA, true>), dim3(grid), dim3(kLossThreads), 0, st, k); \
        else hipLaunchKernelGGL(surrogate_loss_kernel<AA>, dim3(grid), dim3(kLossThreads), 0, st, k);   \
        break;
#define LS(AA)                                                                                           \
    case AA:                                                                                             \
        if (use_ref) hipLaunchKernelGGL((surrogate_loss_kernel<AA, true, true>), dim3(grid), dim3(kLossThreads), 0, st, k); \
        else hipLaunchKernelGGL((surrogate_loss_kernel<AA, false, true>), dim3(grid), dim3(kLossThreads), 0, st, k);   \
        break;
    if (use_std) {
        switch (a->act_dim) { LS(1) LS(2) LS(3) LS(4) }
    } else {
        switch (a->act_dim) { L(1) L(2) L(3) L(4) L(5) L(6) L(7) L(8) }
    }
#undef L
#undef LS
    TG_LAUNCH_CHECK("tg_surrogate_loss");
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, st, a->d_work, (int)grid, a->d_sums);
    TG_LAUNCH_CHECK("tg_surrogate_loss(final)");
    return TG_OK;
}

int tg_surrogate_loss(const tg_loss_args* a, void* stream) { return surrogate_loss(a, nullptr, stream); }

int tg_surrogate_loss_ref(const tg_loss_args* a, const tg_ref_penalty* ref, void* stream) { return surrogate_loss(a, ref, stream); }

int tg_surrogate_loss_std(const tg_loss_args* a, const tg_ref_penalty* ref, const tg_learned_std* std, void* stream) {
    return surrogate_loss(a, ref, stream, std);
}

int tg_log_std_grad_blocks(void) { return kStdBlocks; }

int tg_log_std_grad(const float* d_rows4, int64_t rows, int32_t act_dim, float add, float* d_grad, double* d_work, void* stream) {
    TG_REQUIRE(d_rows4 && d_grad && d_work, "tg_log_std_grad: null pointer");
    TG_REQUIRE(rows >= 0 && act_dim >= 1 && act_dim <= 4, "tg_log_std_grad: bad sizes (rows %lld, act_dim %d)", (long long)rows, act_dim);
    TG_REQUIRE(((uintptr_t)d_rows4 & 15) == 0, "tg_log_std_grad: the rows are not 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = ceil_div(rows > 0 ? rows : 1, (int64_t)256 * 8);
    const unsigned grid = (unsigned)(nb < kStdBlocks ? nb : kStdBlocks);
    hipLaunchKernelGGL(log_std_partial_kernel, dim3(grid), dim3(256), 0, st, (const float4*)d_rows4, rows, d_work);
    TG_LAUNCH_CHECK("tg_log_std_grad");
    hipLaunchKernelGGL(log_std_final_kernel, dim3(1), dim3(64), 0, st, d_work, (int)grid, act_dim, add, d_grad);
    TG_LAUNCH_CHECK("tg_log_std_grad(final)");
    return TG_OK;
}

}  // extern "C"
