// The loss head of the fp32 chain learners (mlp_f32_chain.hip: H = 64 / 128; mlp_f32_wide.hip: H = 256) for ONE row whose head
// outputs a lane holds: the loads, the stores and the workgroup's loss sums around loss_row.hpp's arithmetic.
#pragma once
#include "loss_row.hpp"

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

// host: tg_chain_loss (+ the reference policy's penalty and the learned log-std, or null) -> F32Loss
static inline void fill_f32_loss(F32Loss& L, const tg_chain_loss* loss, const tg_ref_penalty* ref = nullptr, const tg_learned_std* std = nullptr) {
    fill_loss_common(L, loss, ref, std);
    L.logp_old_out = loss->kind == 0 ? loss->d_logp_old_out : nullptr;
    L.dout4 = (float*)loss->d_dout8; L.work = loss->d_work;
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
// kRef: GRPO's penalty to the reference policy joins c_kl and g.
// kStd: the row's contribution to d loss / d log_std goes to std_out[row][4] (valid rows, the writer lane)
template <bool kZeroInvalid = true, bool kRef = false, bool kStd = false>
__device__ static inline void f32_loss_compute(const F32Loss& L, const F32LossIn& in, const float (&o)[4], int64_t row, bool valid, bool writer,
                                               float (&g)[4], float& c_surr, float& c_crit, float& c_kl) {
    g[0] = g[1] = g[2] = g[3] = 0.f;
    c_surr = c_crit = c_kl = 0.f;
    if (L.kind == 0) {
        const Gauss4 G = loss_gauss4(L);
        float dmu[4];
        const float lp = gauss4_logp([&](int k) { return k < L.A ? in.act[k] : 0.f; }, [&](int k) { return o[k]; }, G, dmu);
        float lpo;
        if (L.logp_old_out != nullptr) {
            lpo = lp;
            if (valid && writer) L.logp_old_out[row] = lp;
        } else {
            lpo = in.lpo;
        }
        const ActorTerms t = loss_actor_terms<kRef>(lp, lpo, (in.adv - L.n_m) * L.n_i, L.epsilon, L.surr_coef, L.kl_coef, in.lref, L.ref_coef);
        c_surr = t.c_surr; c_kl = t.c_kl;
        gauss4_mean_grad(t.dlp, dmu, G, g);
        if constexpr (kStd) {
            if (valid && writer) *reinterpret_cast<float4*>(L.std_out + row * 4) = gauss4_log_std_grad(t.dlp, dmu, G, L.A);
        }
    } else {
        const CriticTerms t = loss_critic_terms(o[0], in.act[0], L.n_m, L.n_i, L.critic_coef);
        c_crit = t.c_crit;
        g[0] = t.g0;
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

// The workgroup's four f64 loss sums: lanes -> wave (fixed shuffle tree) -> workgroup (waves in index order): deterministic.
// `red_s`: kWaves x 4 doubles of LDS; `work`: the grid's f64 [grid][4]; every thread of the workgroup calls.
template <int kWaves>
__device__ static inline void f32_loss_sums_store(double (&v)[4], double* red_s, double* work) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red_s[wave * 4 + k] = v[k];
    }
    __syncthreads();
    if (tid < 4) {
        double t = 0.0;
        for (int w = 0; w < kWaves; ++w) t += red_s[w * 4 + tid];
        work[(int64_t)blockIdx.x * 4 + tid] = t;
    }
}

}  // namespace tg
