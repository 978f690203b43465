// The loss-head arithmetic of ONE row (algorithms/ppo.py:159-179, grpo.py:122-140), defined once for every learner kernel that
// compiles it: loss_kernels.hip::surrogate_loss_kernel (the library-GEMM fallback), the kHead arm of mlp_fwd_chain.hip (the bf16
// chain learner) and f32_loss.hpp::f32_loss_compute (the fp32 chain learners).  The row functions take and return VALUES only: each
// head keeps its own loads, stores and sums.  Around them: the entry-time pick-up of device-resident constants and the host fill of
// the fields the chain heads' argument structs share.
#pragma once
#include "tg_common.hpp"

namespace tg {

// ---- the actor terms: clipped surrogate, KL-ish penalty to the old policy, GRPO's penalty to a frozen reference policy ----
struct ActorTerms { float c_surr, c_kl, dlp; };     // the row's surrogate and KL contributions, d total / d logp

// kRef: x = lp_ref - lp, D = exp(x) - x - 1 (grpo.py:133): D joins the KL contribution and d total / d logp gains ref_coef (exp(x) - 1),
// ref_coef = coef * beta (the term enters J as - beta D).  (ref_penalty_check refuses kl_coef != 0 beside a reference penalty: at
// most one of the two KL terms is ever non-zero.)
template <bool kRef>
__device__ static inline ActorTerms loss_actor_terms(float lp, float lpo, float adv, float epsilon, float surr_coef, float kl_coef,
                                                     float lref, float ref_coef) {
    ActorTerms t;
    const float rho = expf(lp - lpo);
    const float lo = 1.0f - epsilon, hi = 1.0f + epsilon;
    const float surr1 = rho * adv, surr2 = fminf(fmaxf(rho, lo), hi) * adv;
    // torch.min / torch.clamp subgradients: inside the clip range both branches carry A (tie -> half each); outside, only the
    // unclipped branch when it is the smaller one.
    const bool inside = (rho >= lo) && (rho <= hi);
    const float w = inside ? 1.0f : (surr1 < surr2 ? 1.0f : 0.0f);
    t.c_surr = fminf(surr1, surr2);
    t.c_kl = 0.f;
    t.dlp = surr_coef * adv * rho * w;
    if (kl_coef != 0.0f) {
        const float eo = expf(lpo);
        t.c_kl = eo * (lpo - lp);
        t.dlp -= kl_coef * eo;
    }
    if constexpr (kRef) {
        const float x = lref - lp;
        const float em1 = expf(x) - 1.0f;
        t.c_kl += em1 - x;
        t.dlp += ref_coef * em1;
    }
    return t;
}

// ---- the critic term: squared error against the normalised return ----
struct CriticTerms { float c_crit, g0; };           // the row's squared error, d total / d value

__device__ static inline CriticTerms loss_critic_terms(float value, float ret, float n_m, float n_i, float critic_coef) {
    const float d = value - (ret - n_m) * n_i;
    return CriticTerms{d * d, critic_coef * 2.0f * d};
}

// ---- the diagonal Gaussian: one column ... ----
__device__ static inline float gauss_mean_grad(float dlp, float dmu, float inv_var) { return dlp * dmu * inv_var; }                  // d total / d mu_k
__device__ static inline float gauss_log_std_grad(float dlp, float dmu, float inv_var) { return dlp * (dmu * dmu * inv_var - 1.0f); } // d total / d log_std_k

// ---- ... up to eight columns with a host-given variance (tg_gaussian_logp, tg_surrogate_loss, tg_policy_shift) ... ----
struct Var8 { float inv_var[8]; float logp_const; };

__device__ static inline float gaussian_logp(const float* mu, const float* a, const Var8& v, int A) {
    float quad = 0.0f;
#pragma unroll 4
    for (int k = 0; k < A; ++k) {
        const float d = a[k] - mu[k];
        quad += d * d * v.inv_var[k];
    }
    return -0.5f * quad + v.logp_const;
}

// host: Var8 from the caller's variance array
static inline int make_var(const float* var, int A, Var8& v, const char* who) {
    if (A < 1 || A > 8) return set_error(TG_ERR_ARG, "%s: act_dim %d outside 1..8", who, A);
    double logdet = 0;
    for (int k = 0; k < 8; ++k) v.inv_var[k] = 0.f;
    for (int k = 0; k < A; ++k) {
        if (!(var[k] > 0.f)) return set_error(TG_ERR_ARG, "%s: var[%d] must be positive", who, k);
        v.inv_var[k] = 1.0f / var[k];
        logdet += log((double)var[k]);
    }
    v.logp_const = (float)(-0.5 * A * log(2.0 * 3.141592653589793) - 0.5 * logdet);
    return TG_OK;
}

// Four f64 sums of a 256-thread block, deterministic: lanes -> wave (fixed shuffle tree) -> the four waves as ((w0 + w1) + w2) + w3.
// Thread j < 4 returns sum j, the others 0.
__device__ static inline double block_sum4_f64(double (&acc)[4]) {
    __shared__ double sh[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[j] += __shfl_down(acc[j], off, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sh[j][w] = acc[j];
    }
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < 4) {
        const int j = threadIdx.x;
        t = ((sh[j][0] + sh[j][1]) + sh[j][2]) + sh[j][3];
    }
    return t;
}

// ---- ... and the four columns of a chain head (inv_var is 0 beyond the net's outputs) ----
struct Gauss4 { float inv_var[4]; float logp_const; };

// the row's action act(k) (0 for columns >= A; a callable, so that each head's load of column k stays next to its use) and the head's
// means mu(k) -> dmu and the row's log-probability
template <typename Act, typename Mu>
__device__ static inline float gauss4_logp(Act&& act, Mu&& mu, const Gauss4& G, float (&dmu)[4]) {
    float quad = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d = act(k) - mu(k);
        dmu[k] = d;
        quad += d * d * G.inv_var[k];
    }
    return -0.5f * quad + G.logp_const;
}
__device__ static inline void gauss4_mean_grad(float dlp, const float (&dmu)[4], const Gauss4& G, float (&g)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = gauss_mean_grad(dlp, dmu[k], G.inv_var[k]);
}
// kStd: the row's contribution to d total / d log_std (zeros for k >= A)
__device__ static inline float4 gauss4_log_std_grad(float dlp, const float (&dmu)[4], const Gauss4& G, int A) {
    float gs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) gs[k] = k < A ? gauss_log_std_grad(dlp, dmu[k], G.inv_var[k]) : 0.f;
    return float4{gs[0], gs[1], gs[2], gs[3]};
}
// the Gaussian's constants from the policy's log_std(k), a callable asked for the columns k < A only; the others keep G's inv_var
template <typename LogStd>
__device__ static inline Gauss4 gauss4_from_log_std(LogStd&& log_std, int A, Gauss4 G) {
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < A) {
            const float ls = log_std(k);
            G.inv_var[k] = expf(-2.0f * ls);
            sum += ls;
        }
    }
    G.logp_const = -0.5f * (float)A * 1.8378770664093453f - sum;
    return G;
}

// ---- device, at kernel entry (ChainLoss / F32Loss; `L` is the kernel's own copy and its fields stay scalar registers) ----
template <typename Loss>
__device__ static inline Gauss4 loss_gauss4(const Loss& L) {
    return Gauss4{{L.inv_var[0], L.inv_var[1], L.inv_var[2], L.inv_var[3]}, L.logp_const};
}
// The normalisation pair and the coefficients from the device when PPO keeps them there (tg_ppo_norm's output never visits the host).
// kStd: also the Gaussian's constants from the policy's log_std.  Uniform scalar loads, before anything is in flight.
template <bool kStd, typename Loss>
__device__ static inline void loss_from_device(Loss& L) {
    if (L.norm8 != nullptr) {
        const int q = L.kind == 1 ? 2 : 0;
        L.n_m = L.norm8[q]; L.n_i = L.norm8[q + 1];
        L.surr_coef = L.norm8[4]; L.critic_coef = L.norm8[5]; L.kl_coef = L.norm8[6];
    }
    if constexpr (kStd) {
        const Gauss4 G = gauss4_from_log_std([&](int k) { return L.log_std[k]; }, L.A, loss_gauss4(L));
#pragma unroll
        for (int k = 0; k < 4; ++k) L.inv_var[k] = G.inv_var[k];
        L.logp_const = G.logp_const;
    }
}

// ---- host: the fields ChainLoss and F32Loss share, from tg_chain_loss (+ the reference policy's penalty and the learned log-std,
// or null); the caller adds its own outputs ----
template <typename Loss>
static inline void fill_loss_common(Loss& L, const tg_chain_loss* loss, const tg_ref_penalty* ref, const tg_learned_std* std) {
    L.kind = loss->kind; L.A = loss->act_dim;
    L.act = loss->kind == 0 ? loss->d_act : loss->d_ret;
    L.logp_old = loss->d_logp_old; L.adv = loss->d_adv;
    L.n_m = loss->norm_mean; L.n_i = loss->norm_inv; L.norm8 = loss->d_norm8;
    float logdet = 0.f;
    for (int k = 0; k < 4; ++k) {                   // (a learned log-std: formed on the device at kernel entry)
        L.inv_var[k] = (k < loss->act_dim && std == nullptr) ? 1.0f / loss->var[k] : 0.f;
        if (k < loss->act_dim && std == nullptr) logdet += logf(loss->var[k]);
    }
    L.logp_const = -0.5f * (float)loss->act_dim * 1.8378770664093453f - 0.5f * logdet;
    L.epsilon = loss->epsilon; L.surr_coef = loss->surr_coef; L.critic_coef = loss->critic_coef; L.kl_coef = loss->kl_coef;
    L.logp_ref = ref != nullptr ? ref->d_logp_ref : nullptr; L.ref_coef = ref != nullptr ? ref->coef : 0.f;
    L.log_std = std != nullptr ? std->d_log_std : nullptr; L.std_out = std != nullptr ? std->d_out : nullptr;
}

}  // namespace tg
