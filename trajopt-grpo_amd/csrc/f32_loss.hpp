// The loss head of the fp32 chain learners (mlp_f32_chain.hip: H = 64 / 128; mlp_f32_wide.hip: H = 256): the arithmetic of
// loss_kernels.hip::surrogate_loss_kernel (algorithms/ppo.py:159-179, grpo.py:122-140) for ONE row whose head outputs a lane holds.
#pragma once
#include "tg_common.hpp"

namespace tg {

struct F32Loss {            // (as ChainLoss of mlp_fwd_chain.hip)
    int32_t kind, A;        // 0: actor (clipped surrogate + KL-ish penalty), 1: critic (squared error)
    const float* act;       // actor: [rows][A] contiguous; critic: the returns [rows]
    const float* logp_old; const float* adv;
    float* logp_old_out;    // non-null: the old policy is the current one -- the row's log-probability is its old log-probability, written here
    float n_m, n_i;         // normalisation of the advantage (actor) / return (critic): (x - n_m) * n_i
    float inv_var[4]; float logp_const, epsilon, surr_coef, critic_coef, kl_coef;
    const float* norm8;     // non-null: n_m / n_i and the three coefficients come from this device f32 [8] (tg_ppo_norm's output)
    float* dout4;           // out: d loss / d head output, f32 [rows][4] (columns >= A zero)
    double* work;           // out: f64 [grid][4] partial loss sums (surrogate, squared error, KL, count)
    // kRef instantiations only (tg_ref_penalty): log pi_ref of the row [rows] and coef * beta; read, never written, by the device
    const float* logp_ref; float ref_coef;
    // kStd instantiations only (tg_learned_std): the policy's log_std [A] on the device (inv_var / logp_const are formed from it at
    // kernel entry) and the per-row d loss / d log_std side output f32 [rows][4]
    const float* log_std; float* std_out;
};

// host: tg_chain_loss (+ the reference policy's penalty, or null) -> F32Loss
static inline void fill_f32_loss(F32Loss& L, const tg_chain_loss* loss, const tg_ref_penalty* ref = nullptr, const tg_learned_std* std = nullptr) {
    L.kind = loss->kind; L.A = loss->act_dim;
    L.act = loss->kind == 0 ? loss->d_act : loss->d_ret;
    L.logp_old = loss->d_logp_old; L.adv = loss->d_adv; L.logp_old_out = loss->kind == 0 ? loss->d_logp_old_out : nullptr;
    L.n_m = loss->norm_mean; L.n_i = loss->norm_inv; L.norm8 = loss->d_norm8;
    float logdet = 0.f;
    for (int k = 0; k < 4; ++k) {
        L.inv_var[k] = (k < loss->act_dim && std == nullptr) ? 1.0f / loss->var[k] : 0.f;
        if (k < loss->act_dim && std == nullptr) logdet += logf(loss->var[k]);
    }
    L.log_std = std != nullptr ? std->d_log_std : nullptr; L.std_out = std != nullptr ? std->d_out : nullptr;
    L.logp_const = -0.5f * (float)loss->act_dim * 1.8378770664093453f - 0.5f * logdet;
    L.epsilon = loss->epsilon; L.surr_coef = loss->surr_coef; L.critic_coef = loss->critic_coef; L.kl_coef = loss->kl_coef;
    L.dout4 = (float*)loss->d_dout8; L.work = loss->d_work;
    L.logp_ref = ref != nullptr ? ref->d_logp_ref : nullptr; L.ref_coef = ref != nullptr ? ref->coef : 0.f;
}

// device, at kernel entry: the normalisation pair and the coefficients from the device when PPO keeps them there
// kStd: also the Gaussian's constants from the policy's log_std (uniform loads; columns >= A keep inv_var = 0)
template <bool kStd = false>
__device__ static inline void f32_loss_from_device(F32Loss& L) {
    if (L.norm8 != nullptr) {
        const int q = L.kind == 1 ? 2 : 0;
        L.n_m = L.norm8[q]; L.n_i = L.norm8[q + 1];
        L.surr_coef = L.norm8[4]; L.critic_coef = L.norm8[5]; L.kl_coef = L.norm8[6];
    }
    if constexpr (kStd) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < L.A) {
                const float ls = L.log_std[k];
                L.inv_var[k] = expf(-2.0f * ls);
                sum += ls;
            }
        L.logp_const = -0.5f * (float)L.A * 1.8378770664093453f - sum;
    }
}

// The per-row inputs of the loss head, loadable ahead of the row's products (f32_loss_load) ...
struct F32LossIn { float act[4]; float lpo, adv, lref; };

// (every load unconditional within its uniform branch: columns >= A re-read the last action column)
// row = base + r: `base` wave-uniform (it goes into the scalar part of the address), `r` the lane's part
// kRef: also the row's reference log-probability (GRPO's KL penalty to a frozen reference policy)
template <bool kRef = false, typename R>
__device__ static inline F32LossIn f32_loss_load(const F32Loss& L, int64_t base, R r) {
    F32LossIn in;
    in.act[1] = in.act[2] = in.act[3] = 0.f; in.lpo = 0.f; in.adv = 0.f; in.lref = 0.f;
    if (L.kind == 0) {
        const float* act = L.act + base * L.A;
#pragma unroll
        for (int k = 0; k < 4; ++k) in.act[k] = act[r * L.A + (k < L.A ? k : L.A - 1)];
        if (L.logp_old_out == nullptr) in.lpo = (L.logp_old + base)[r];
        in.adv = (L.adv + base)[r];
        if constexpr (kRef) in.lref = (L.logp_ref + base)[r];
    } else {
        in.act[0] = (L.act + base)[r];
    }
    return in;
}
template <bool kRef = false>
__device__ static inline F32LossIn f32_loss_load(const F32Loss& L, int64_t rowc) { return f32_loss_load<kRef>(L, (int64_t)0, rowc); }

// ... and the arithmetic: head outputs o[4] -> d loss / d output g[4] and the row's contributions to the loss sums.  `row` / `valid` /
// `writer` decide what is written (one lane per row writes).  kZeroInvalid: a lane past the last row gets g = 0 (mlp_f32_chain.hip);
// false: it keeps the clamped row's own g -- the 16-row kernels let such lanes recompute and re-store the last row's values
// (identical bytes), so that every store instruction is issued whatever the row count.
// kRef: GRPO's penalty to the reference policy, x = lp_ref - lp, D = exp(x) - x - 1 (grpo.py:133): D joins the KL sum and
// d loss / d lp gains ref_coef (exp(x) - 1), ref_coef = coef * beta (the term enters J as - beta D).
// kStd: the row's contribution to d loss / d log_std, dlp (dmu_k^2 inv_var_k - 1), to std_out[row][4] (valid rows, the writer lane)
template <bool kZeroInvalid = true, bool kRef = false, bool kStd = false>
__device__ static inline void f32_loss_compute(const F32Loss& L, const F32LossIn& in, const float (&o)[4], int64_t row, bool valid, bool writer,
                                               float (&g)[4], float& c_surr, float& c_crit, float& c_kl) {
    g[0] = g[1] = g[2] = g[3] = 0.f;
    c_surr = c_crit = c_kl = 0.f;
    if (L.kind == 0) {
        float quad = 0.f, dmu[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = (k < L.A ? in.act[k] : 0.f) - o[k];
            dmu[k] = d;
            quad += d * d * L.inv_var[k];
        }
        const float lp = -0.5f * quad + L.logp_const;
        float lpo;
        if (L.logp_old_out != nullptr) {
            lpo = lp;
            if (valid && writer) L.logp_old_out[row] = lp;
        } else {
            lpo = in.lpo;
        }
        const float adv = (in.adv - L.n_m) * L.n_i;
        const float rho = expf(lp - lpo);
        const float lo = 1.0f - L.epsilon, hi = 1.0f + L.epsilon;
        const float surr1 = rho * adv, surr2 = fminf(fmaxf(rho, lo), hi) * adv;
        const bool inside = (rho >= lo) && (rho <= hi);
        const float w = inside ? 1.0f : (surr1 < surr2 ? 1.0f : 0.0f);
        c_surr = fminf(surr1, surr2);
        float dlp = L.surr_coef * adv * rho * w;
        if (L.kl_coef != 0.0f) {
            const float eo = expf(lpo);
            c_kl = eo * (lpo - lp);
            dlp -= L.kl_coef * eo;
        }
        if constexpr (kRef) {
            const float x = in.lref - lp;
            const float em1 = expf(x) - 1.0f;
            c_kl += em1 - x;
            dlp += L.ref_coef * em1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = dlp * dmu[k] * L.inv_var[k];
        if constexpr (kStd) {
            if (valid && writer) {
                float gs[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) gs[k] = k < L.A ? dlp * (dmu[k] * dmu[k] * L.inv_var[k] - 1.0f) : 0.f;
                *reinterpret_cast<float4*>(L.std_out + row * 4) = float4{gs[0], gs[1], gs[2], gs[3]};
            }
        }
    } else {
        const float d = o[0] - (in.act[0] - L.n_m) * L.n_i;
        c_crit = d * d;
        g[0] = L.critic_coef * 2.0f * d;
    }
    if constexpr (kZeroInvalid) {
        if (!valid) { g[0] = g[1] = g[2] = g[3] = 0.f; }
    }
}

// One row, inputs loaded on the spot (`rowc` = the row clamped into range).
template <bool kZeroInvalid = true, bool kRef = false, bool kStd = false>
__device__ static inline void f32_loss_row(const F32Loss& L, const float (&o)[4], int64_t row, int64_t rowc, bool valid, bool writer,
                                           float (&g)[4], float& c_surr, float& c_crit, float& c_kl) {
    const F32LossIn in = f32_loss_load<kRef>(L, rowc);
    f32_loss_compute<kZeroInvalid, kRef, kStd>(L, in, o, row, valid, writer, g, c_surr, c_crit, c_kl);
}

}  // namespace tg
