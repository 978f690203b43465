// Fused GPU-resident rollout for float32 policies: the whole T-step loop in ONE persistent launch, every product in
// fp32 (v_mfma_f32_32x32x2_f32) -- the reference's own precision (rollout/rollout_worker.py:19-84 with the fp32
// policies of policies/actor_critic.py:107-138).
//
// The bf16 kernel (fused_rollout.hip) is built for throughput at 10^4..10^5 envs; this one is built for LATENCY at the
// reference's net sizes (128 x 3, 128 x 4, 64-wide nets) and a few thousand envs, where the per-step launch path
// spends its time between kernels (~20 us per time step for 4,096 CartPole envs):
//   * a workgroup owns 32 envs for the whole rollout (many small workgroups: 4,096 envs = 128 CUs busy);
//   * wave w of its H/32 waves owns the 32-feature output tile w of EVERY layer, and its rows of every weight matrix
//     stay in REGISTERS for the whole rollout (H/2 registers per H x H layer): no weight traffic at all after the
//     prologue, neither HBM nor LDS;
//   * transposed form Y^T = W . X^T: the 32 columns of a tile are the 32 envs.  A layer's output tile goes to LDS in
//     groups of 4 consecutive features ([H/4][32 envs][4]), one raw s_barrier, and every wave reads the whole
//     activation vector back as its B operands (lane (env, kh) takes group 2q + kh: ds_read_b128, conflict-free).
//     The k order this implies (step 4q + j multiplies feature 8q + 4kh + j) is folded into the weight registers;
//   * the head (A <= 4 outputs) is a 16-term fp32 dot product per lane on the last accumulators, summed over the
//     2 H/32 partials through LDS in a fixed order;
//   * every wave steps the workgroup's 32 envs redundantly (same instructions, same inputs: same bits), so the env
//     state never has to be broadcast; wave 0 records the trajectory.  Sampling (Philox keyed by global env index
//     and t), dynamics, recording and termination are the code of rollout_step_kernel.
// HBM traffic per env-step is the trajectory record only.
#include "env_dynamics.hpp"
#include "act_f32.hpp"

#include <string.h>

namespace tg {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct SigmaF32 { float v[8]; };

// accumulator start values: rows (r&3) + 8(r>>2) + 4h of a 32-row tile, `b` = tile base + 4h
__device__ static inline f32x16 bias_rows_f32(const float* __restrict__ b) {
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 b4 = *reinterpret_cast<const float4*>(b + 8 * q);
        acc[4 * q] = b4.x; acc[4 * q + 1] = b4.y; acc[4 * q + 2] = b4.z; acc[4 * q + 3] = b4.w;
    }
    return acc;
}

__device__ static inline float4 f32r_lds_f4(const float* __restrict__ p) { return *reinterpret_cast<const float4*>(p); }

__device__ static inline void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // not __syncthreads(): that would also wait for the trajectory stores
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// H = hidden width (64 / 128), NHH = number of H x H layers (hidden layers - 1), kAct = hidden activation (act_f32.hpp).
// Env = PerEnv<...> (the `_dr` entry points; c_arg is then the parameter table): every lane builds the constants of its own env at
// entry and keeps them in registers for the whole rollout (the waves step the workgroup's envs redundantly: the same bits in each).
// Tables: `wstream` f32 [H/32 waves][K1/2 + NHH*H/2 registers][64 lanes]; `tab` f32 [(NHH+1)*H biases][4*H head
// weights, rows >= A zero][4 head biases].
template <typename Env, int H, int NHH, int kAct>
__global__ __launch_bounds__(64 * (H / 32)) __attribute__((amdgpu_waves_per_eu(lag_min_waves<kLagFamF32, Env, float, H, NHH, kAct>())))
void fused_rollout_f32_kernel(
    typename Env::C c_arg, float* __restrict__ obs, float* __restrict__ act, float* __restrict__ rew, uint8_t* __restrict__ mask,
    int32_t* __restrict__ len, int64_t n, int32_t T, int32_t t0, int32_t t1, const float* __restrict__ wstream,
    const float* __restrict__ tab, SigmaF32 sigma, const uint64_t* __restrict__ rng, int64_t env_offset, int32_t agents) {
    constexpr int S = Env::S, A = Env::A, WPW = H / 32;
    constexpr int K1 = (S + 7) / 8 * 8, R1 = K1 / 2, RH = H / 2, RW = R1 + NHH * RH;
    constexpr int NB = (NHH + 1) * H, NTAB = NB + 4 * H + 4;
    static_assert(S <= 32 && A <= 4, "state <= 32 features, <= 4 actions");
    extern __shared__ float lds_f[];
    float* tab_s = lds_f;                                   // NTAB floats
    float* actb = tab_s + NTAB;                             // 2 buffers x [H/4 groups][32 envs][4]
    float* red = actb + 2 * H * 32;                         // 2 buffers x [A][2 WPW partials][32 envs]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int64_t i = (int64_t)blockIdx.x * 32 + col;       // lanes 32..63 shadow lanes 0..31 (they carry the upper k-halves)
    const bool in_range = (i < n) && (h == 0) && (wave == 0);
    const int64_t ic = (i < n) ? i : n - 1;
    const int64_t T1 = (int64_t)T + 1;
    constexpr bool kPerEnv = EnvTraits<Env>::kPerEnv;
    constexpr bool kObsNorm = EnvTraits<Env>::kObsNorm;
    const auto& e_arg = env_arg(c_arg);
    typename EnvTraits<Env>::Consts own;                    // kPerEnv: this lane's vehicle, for the whole rollout
    if constexpr (kPerEnv) own = env_constants<Env>(e_arg, n, ic);
    const auto& c = pick_constants(e_arg, own);
    ObsNormRegs<kObsNorm ? S : 1> on;                       // kObsNorm: the per-feature table, read once per launch
    if constexpr (kObsNorm) on.load(c_arg.on);

    for (int q = threadIdx.x; q < NTAB; q += 64 * WPW) tab_s[q] = tab[q];
    float w1[R1], wh[NHH > 0 ? NHH : 1][RH];
    {
        const float* my = wstream + (int64_t)wave * RW * 64 + lane;
#pragma unroll
        for (int r = 0; r < R1; ++r) w1[r] = my[r * 64];
#pragma unroll
        for (int l = 0; l < NHH; ++l)
#pragma unroll
            for (int r = 0; r < RH; ++r) wh[l][r] = my[(R1 + l * RH + r) * 64];
    }
    float s[S];
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] = obs[(k * T1 + t0) * n + ic];
    const int32_t len0 = len[ic];
    bool alive = (i < n) && (Env::kBalanceTerminates ? len0 <= 0 : len0 == 0);
    int balanced_steps = Env::kBalanceTerminates ? -len0 : 0;
    constexpr bool kLag = EnvTraits<Env>::kLag;              // kLag: the motor state from slot t0 (split launches compose), in registers
    float m[A], alpha = 0.0f;
    if constexpr (kLag) {
        alpha = lag_alpha_of<Env>(c_arg, n, ic);
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const float v = lag_of(c_arg).motor[(k * T1 + t0) * n + ic];
            m[k] = alive ? v : 0.0f;
        }
    }
    __syncthreads();
    int par = 0, rpar = 0;

    for (int32_t t = t0; t < t1; ++t) {
        if (__ballot(alive) == 0ull) break;                  // the same 32 envs in every wave: a uniform exit
        // ---- layer 1: B operands straight from the state registers (feature 8q + 4kh + j at step 4q + j) ----
        f32x16 acc = bias_rows_f32(tab_s + 32 * wave + 4 * h);
#pragma unroll
        for (int q = 0; q < K1 / 8; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float lo = (8 * q + j < S) ? s[(8 * q + j < S) ? 8 * q + j : 0] : 0.0f;
                float hi = (8 * q + 4 + j < S) ? s[(8 * q + 4 + j < S) ? 8 * q + 4 + j : 0] : 0.0f;
                if constexpr (kObsNorm) {                    // what the policy sees of s (the dynamics keep stepping s itself)
                    if (8 * q + j < S) lo = on.apply(lo, 8 * q + j);
                    if (8 * q + 4 + j < S) hi = on.apply(hi, 8 * q + 4 + j);
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[4 * q + j], h ? hi : lo, acc, 0, 0, 0);
            }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = act_f32<kAct>(acc[r]);
        // ---- H x H layers: exchange the activation vector through LDS, multiply with the register-resident rows ----
#pragma unroll
        for (int l = 0; l < NHH; ++l) {
            float* buf = actb + par * (H * 32);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(buf + ((8 * wave + 2 * g + h) * 32 + col) * 4) =
                    float4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
            lds_barrier();
            acc = bias_rows_f32(tab_s + (l + 1) * H + 32 * wave + 4 * h);
#pragma unroll
            for (int q = 0; q < H / 8; ++q) {
                const float4 x = *reinterpret_cast<const float4*>(buf + ((2 * q + h) * 32 + col) * 4);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wh[l][4 * q], x.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wh[l][4 * q + 1], x.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wh[l][4 * q + 2], x.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wh[l][4 * q + 3], x.w, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = act_f32<kAct>(acc[r]);
            par ^= 1;
        }
        // ---- head: per-lane partial dot products over this lane's 16 features, summed through LDS in a fixed order ----
        float mu[A];
        {
            float* rb = red + rpar * (A * 2 * WPW * 32);
#pragma unroll
            for (int k = 0; k < A; ++k) {
                const float* hw = tab_s + NB + k * H + 32 * wave + 4 * h;
                float p = 0.0f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 w4 = *reinterpret_cast<const float4*>(hw + 8 * g);
                    p = __builtin_fmaf(acc[4 * g], w4.x, p);
                    p = __builtin_fmaf(acc[4 * g + 1], w4.y, p);
                    p = __builtin_fmaf(acc[4 * g + 2], w4.z, p);
                    p = __builtin_fmaf(acc[4 * g + 3], w4.w, p);
                }
                rb[(k * 2 * WPW + 2 * wave + h) * 32 + col] = p;
            }
            lds_barrier();
#pragma unroll
            for (int k = 0; k < A; ++k) {
                float m = tab_s[NB + 4 * H + k];
#pragma unroll
                for (int q = 0; q < 2 * WPW; ++q) m += rb[(k * 2 * WPW + q) * 32 + col];
                mu[k] = m;
            }
            rpar ^= 1;
        }
        // ---- sample, step, record (same arithmetic and RNG keys as rollout_step_kernel) ----
        float a[A];
        {
            uint32_t rnd[4];
            Philox::draw(rng[0], (uint64_t)(env_offset + ic), (uint32_t)t, (uint32_t)rng[1], rnd);
            float eps[4];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                if (2 * hh < A) {
                    const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(Philox::u01(rnd[2 * hh])));
                    const float rev = Philox::u01(rnd[2 * hh + 1]);
                    eps[2 * hh] = rad * __builtin_amdgcn_cosf(rev);
                    eps[2 * hh + 1] = rad * __builtin_amdgcn_sinf(rev);
                }
            }
#pragma unroll
            for (int k = 0; k < A; ++k) a[k] = rn_add(mu[k], rn_mul(sigma.v[k], eps[k]));
        }
        float o[S], r;
        StepOut out;
        if constexpr (kLag) {                                // (the rotor lag in front of every physics step)
            int count;
            out = lagged_substep_loop<Env>(s, a, c, t, substeps_of(c_arg), alive, alpha, m, o, r, count);
        } else if constexpr (EnvTraits<Env>::kSubsteps) {    // (control decimation: up to k calls of Env::step, rewards summed)
            int count;
            out = substep_loop<Env>(s, a, c, t, substeps_of(c_arg), alive, o, r, count);
        } else {
            out = Env::step(s, a, c, t + 1, o, r);
        }
        bool ended = out.truncated;
        if constexpr (Env::kBalanceTerminates) {
            balanced_steps = out.balanced ? balanced_steps + 1 : 0;
            ended = ended || (balanced_steps >= c.term_steps);              // terminated, pendulum_env.py:151
        }
        const bool done = any_in_segment(alive && ended, agents) || (t + 1 >= T);
        const bool carry = alive && !done;
        if (in_range) {
#pragma unroll
            for (int k = 0; k < A; ++k) act[((int64_t)k * T + t) * n + i] = alive ? a[k] : 0.0f;
            rew[(int64_t)t * n + i] = alive ? r : 0.0f;
            mask[(int64_t)t * n + i] = alive ? 1 : 0;
#pragma unroll
            for (int k = 0; k < S; ++k) obs[(k * T1 + t + 1) * n + i] = carry ? o[k] : 0.0f;
            if constexpr (kLag) {
#pragma unroll
                for (int k = 0; k < A; ++k) lag_of(c_arg).motor[(k * T1 + t + 1) * n + i] = carry ? m[k] : 0.0f;
            }
            if (alive && done) len[i] = t + 1;
        }
#pragma unroll
        for (int k = 0; k < S; ++k) s[k] = carry ? o[k] : 0.0f;
        if constexpr (kLag) {
#pragma unroll
            for (int k = 0; k < A; ++k) m[k] = carry ? m[k] : 0.0f;
        }
        alive = carry;
    }
    if (Env::kBalanceTerminates && in_range && alive) len[i] = -balanced_steps;   // a later segment [t1, ..) picks the count up
}

// The same rollout with SIXTEEN envs per workgroup on v_mfma_f32_16x16x4_f32, for env counts that leave CUs without a workgroup at 32
// envs each (BASELINE configs[1]: 4,096 CartPole envs = 128 workgroups on 256 CUs).  A time step is a chain of dependent products
// -- 2 H^2 x envs flop per H x H layer on the workgroup's one CU -- so halving the envs per workgroup halves the step's latency and
// fills the other half of the chip.  Wave w still owns features [32 w, 32 w + 32) of every layer, as TWO 16-feature tiles (two
// independent accumulator chains, alternating: a dependent 16x16x4 product issues every 40 cycles, an independent one every 32);
// lane (j, g) = (env j, k sub-index g); the activation vector crosses the waves as [H / 4 groups][16 envs][4] and a lane reads
// group 4 q + g for the four steps 4 q .. 4 q + 3 (features 16 q + 4 g + e at step 4 q + e: folded into the weight registers).
// Weight stream: f32 [H/32 waves][K1/2 + NHH*H/2 registers][64 lanes], register tt * (k / 4) + s of lane (i, g) of wave w =
// W[32 w + 16 tt + i][first layer: 4 s + g | H x H: 16 (s >> 2) + 4 g + (s & 3)].  Everything after the head (sampling, dynamics,
// recording, termination) is the code above; lanes 16..63 shadow lanes 0..15.
typedef float f32x4r __attribute__((ext_vector_type(4)));

template <typename Env, int H, int NHH, int kAct>
__global__ __launch_bounds__(64 * (H / 32)) __attribute__((amdgpu_waves_per_eu(lag_min_waves<kLagFamF32x16, Env, float, H, NHH, kAct>())))
void fused_rollout_f32x16_kernel(
    typename Env::C c_arg, float* __restrict__ obs, float* __restrict__ act, float* __restrict__ rew, uint8_t* __restrict__ mask,
    int32_t* __restrict__ len, int64_t n, int32_t T, int32_t t0, int32_t t1, const float* __restrict__ wstream,
    const float* __restrict__ tab, SigmaF32 sigma, const uint64_t* __restrict__ rng, int64_t env_offset, int32_t agents) {
    constexpr int S = Env::S, A = Env::A, WPW = H / 32, E = 16;
    constexpr int K1 = (S + 7) / 8 * 8, R1 = K1 / 2, RH = H / 2, RW = R1 + NHH * RH, S1 = K1 / 4, SH = H / 4;
    constexpr int NB = (NHH + 1) * H, NTAB = NB + 4 * H + 4;
    static_assert(S <= 32 && A <= 4, "state <= 32 features, <= 4 actions");
    extern __shared__ float lds_f[];
    float* tab_s = lds_f;                                   // NTAB floats
    float* actb = tab_s + NTAB;                             // 2 buffers x [H/4 groups][16 envs][4]
    float* red = actb + 2 * H * E;                          // 2 buffers x [A][4 WPW partials][16 envs]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, col = lane & 15;
    const int64_t i = (int64_t)blockIdx.x * E + col;
    const bool in_range = (i < n) && (g == 0) && (wave == 0);
    const int64_t ic = (i < n) ? i : n - 1;
    const int64_t T1 = (int64_t)T + 1;
    constexpr bool kPerEnv = EnvTraits<Env>::kPerEnv;
    constexpr bool kObsNorm = EnvTraits<Env>::kObsNorm;
    const auto& e_arg = env_arg(c_arg);
    typename EnvTraits<Env>::Consts own;                    // kPerEnv: this lane's vehicle, for the whole rollout
    if constexpr (kPerEnv) own = env_constants<Env>(e_arg, n, ic);
    const auto& c = pick_constants(e_arg, own);
    ObsNormRegs<kObsNorm ? S : 1> on;                       // kObsNorm: the per-feature table, read once per launch
    if constexpr (kObsNorm) on.load(c_arg.on);

    for (int q = threadIdx.x; q < NTAB; q += 64 * WPW) tab_s[q] = tab[q];
    float w1[2][S1], wh[NHH > 0 ? NHH : 1][2][SH];
    {
        const float* my = wstream + (int64_t)wave * RW * 64 + lane;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < S1; ++r) w1[tt][r] = my[(tt * S1 + r) * 64];
#pragma unroll
        for (int l = 0; l < NHH; ++l)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < SH; ++r) wh[l][tt][r] = my[(R1 + l * RH + tt * SH + r) * 64];
    }
    float s[S];
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] = obs[(k * T1 + t0) * n + ic];
    const int32_t len0 = len[ic];
    bool alive = (i < n) && (Env::kBalanceTerminates ? len0 <= 0 : len0 == 0);
    int balanced_steps = Env::kBalanceTerminates ? -len0 : 0;
    constexpr bool kLag = EnvTraits<Env>::kLag;              // kLag: the motor state from slot t0 (split launches compose), in registers
    float m[A], alpha = 0.0f;
    if constexpr (kLag) {
        alpha = lag_alpha_of<Env>(c_arg, n, ic);
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const float v = lag_of(c_arg).motor[(k * T1 + t0) * n + ic];
            m[k] = alive ? v : 0.0f;
        }
    }
    __syncthreads();
    int par = 0, rpar = 0;
    auto bias4 = [&](const float* b) { const float4 v = *reinterpret_cast<const float4*>(b); return f32x4r{v.x, v.y, v.z, v.w}; };

    for (int32_t t = t0; t < t1; ++t) {
        if (__ballot(alive) == 0ull) break;                  // the same 16 envs in every wave: a uniform exit
        // ---- the step's noise first: it depends on (env, t) only, and its ~100 vector instructions fill the products' latencies ----
        float eps[4];
        {
            uint32_t rnd[4];
            Philox::draw(rng[0], (uint64_t)(env_offset + ic), (uint32_t)t, (uint32_t)rng[1], rnd);
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                if (2 * hh < A) {
                    const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(Philox::u01(rnd[2 * hh])));
                    const float rev = Philox::u01(rnd[2 * hh + 1]);
                    eps[2 * hh] = rad * __builtin_amdgcn_cosf(rev);
                    eps[2 * hh + 1] = rad * __builtin_amdgcn_sinf(rev);
                }
            }
        }
        // ---- layer 1: B operands straight from the state registers (feature 4 s + g at step s) ----
        f32x4r acc[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) acc[tt] = bias4(tab_s + 32 * wave + 16 * tt + 4 * g);
#pragma unroll
        for (int r = 0; r < S1; ++r) {
            float x = 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * r + e < S) x = (g == e) ? s[(4 * r + e < S) ? 4 * r + e : 0] : x;
            if constexpr (kObsNorm) {
                // what the policy sees of s: the lane's own feature 4 r + g is selected first (x above, its mean and rstd here), then
                // normalised once; a padding feature stays 0 ((0 - 0) * 1)
                float xm = 0.0f, xr = 1.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * r + e < S) {
                        xm = (g == e) ? on.mean[(4 * r + e < S) ? 4 * r + e : 0] : xm;
                        xr = (g == e) ? on.rstd[(4 * r + e < S) ? 4 * r + e : 0] : xr;
                    }
                x = obs_normalize(x, xm, xr, on.clip);
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[tt][r], x, acc[tt], 0, 0, 0);
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[tt][r] = act_f32<kAct>(acc[tt][r]);
        // ---- H x H layers: exchange the activation vector through LDS, multiply with the register-resident rows ----
#pragma unroll
        for (int l = 0; l < NHH; ++l) {
            float* buf = actb + par * (H * E);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
                *reinterpret_cast<float4*>(buf + ((8 * wave + 4 * tt + g) * E + col) * 4) = float4{acc[tt][0], acc[tt][1], acc[tt][2], acc[tt][3]};
            lds_barrier();
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) acc[tt] = bias4(tab_s + (l + 1) * H + 32 * wave + 16 * tt + 4 * g);
            // (the next group's operands are requested before this group's eight products: hipcc otherwise reads each group into the
            //  same registers right in front of its products -- eight exposed LDS latencies per layer and step)
            float4 x = f32r_lds_f4(buf + (g * E + col) * 4);
#pragma unroll
            for (int q = 0; q < H / 16; ++q) {
                float4 xn = x;
                if (q + 1 < H / 16) xn = f32r_lds_f4(buf + ((4 * (q + 1) + g) * E + col) * 4);
                const float xe[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    __builtin_amdgcn_sched_barrier(0);               // (the two chains stay interleaved, the read stays in front of the group)
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wh[l][0][4 * q + e], xe[e], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wh[l][1][4 * q + e], xe[e], acc[1], 0, 0, 0);
                }
                x = xn;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[tt][r] = act_f32<kAct>(acc[tt][r]);
            par ^= 1;
        }
        // ---- head: per-lane partial dot products over this lane's 8 features, summed through LDS in a fixed order ----
        float mu[A];
        {
            float* rb = red + rpar * (A * 4 * WPW * E);
#pragma unroll
            for (int k = 0; k < A; ++k) {
                const float* hw = tab_s + NB + k * H + 32 * wave + 4 * g;
                float p = 0.0f;
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const float4 w4 = *reinterpret_cast<const float4*>(hw + 16 * tt);
                    p = __builtin_fmaf(acc[tt][0], w4.x, p);
                    p = __builtin_fmaf(acc[tt][1], w4.y, p);
                    p = __builtin_fmaf(acc[tt][2], w4.z, p);
                    p = __builtin_fmaf(acc[tt][3], w4.w, p);
                }
                rb[(k * 4 * WPW + 4 * wave + g) * E + col] = p;
            }
            lds_barrier();
#pragma unroll
            for (int k = 0; k < A; ++k) {
                float m = tab_s[NB + 4 * H + k];
#pragma unroll
                for (int q = 0; q < 4 * WPW; ++q) m += rb[(k * 4 * WPW + q) * E + col];
                mu[k] = m;
            }
            rpar ^= 1;
        }
        // ---- sample, step, record (same arithmetic and RNG keys as rollout_step_kernel) ----
        float a[A];
#pragma unroll
        for (int k = 0; k < A; ++k) a[k] = rn_add(mu[k], rn_mul(sigma.v[k], eps[k]));
        float o[S], r;
        StepOut out;
        if constexpr (kLag) {                                // (the rotor lag in front of every physics step)
            int count;
            out = lagged_substep_loop<Env>(s, a, c, t, substeps_of(c_arg), alive, alpha, m, o, r, count);
        } else if constexpr (EnvTraits<Env>::kSubsteps) {    // (control decimation: up to k calls of Env::step, rewards summed)
            int count;
            out = substep_loop<Env>(s, a, c, t, substeps_of(c_arg), alive, o, r, count);
        } else {
            out = Env::step(s, a, c, t + 1, o, r);
        }
        bool ended = out.truncated;
        if constexpr (Env::kBalanceTerminates) {
            balanced_steps = out.balanced ? balanced_steps + 1 : 0;
            ended = ended || (balanced_steps >= c.term_steps);              // terminated, pendulum_env.py:151
        }
        const bool done = any_in_segment(alive && ended, agents) || (t + 1 >= T);
        const bool carry = alive && !done;
        if (in_range) {
#pragma unroll
            for (int k = 0; k < A; ++k) act[((int64_t)k * T + t) * n + i] = alive ? a[k] : 0.0f;
            rew[(int64_t)t * n + i] = alive ? r : 0.0f;
            mask[(int64_t)t * n + i] = alive ? 1 : 0;
#pragma unroll
            for (int k = 0; k < S; ++k) obs[(k * T1 + t + 1) * n + i] = carry ? o[k] : 0.0f;
            if constexpr (kLag) {
#pragma unroll
                for (int k = 0; k < A; ++k) lag_of(c_arg).motor[(k * T1 + t + 1) * n + i] = carry ? m[k] : 0.0f;
            }
            if (alive && done) len[i] = t + 1;
        }
#pragma unroll
        for (int k = 0; k < S; ++k) s[k] = carry ? o[k] : 0.0f;
        if constexpr (kLag) {
#pragma unroll
            for (int k = 0; k < A; ++k) m[k] = carry ? m[k] : 0.0f;
        }
        alive = carry;
    }
    if (Env::kBalanceTerminates && in_range && alive) len[i] = -balanced_steps;   // a later segment [t1, ..) picks the count up
}

// The kernel instantiation that the variant names (with_env_variant, env_dynamics.hpp), at 16 or 32 envs per workgroup.
// `who`: the name in the launch check and the refusals (the plain entry's, or tg_fused_rollout_f32_sub's).
template <template <typename> class EnvT, int H, int NHH, int kAct>
static int fused_f32_launch(const char* who, const EnvVariant& v, const tg_traj* tr, const float* wstream, const float* tab, const float* sigma,
                            const uint64_t* rng, int64_t env_offset, int t0, int t1, int block_envs, hipStream_t st) {
    using Env = EnvT<float>;
    constexpr int WPW = H / 32, A = Env::A;
    SigmaF32 sg;
    memset(&sg, 0, sizeof(sg));
    for (int k = 0; k < A; ++k) sg.v[k] = sigma[k];
    static_assert(sizeof(float) * ((NHH + 1) * H + 4 * H + 4 + 2 * H * 32 + 2 * 4 * 2 * WPW * 32) <= 64 * 1024, "LDS budget");
    return with_env_variant<Env, true>(v, [&](auto tag, const auto& arg) -> int {
        using EnvK = typename decltype(tag)::type;
        auto launch = [&](auto kernel, int envs) {
            const size_t shmem = sizeof(float) * ((size_t)(NHH + 1) * H + 4 * H + 4 + 2 * H * envs + 2 * A * (64 / envs) * WPW * envs);
            hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(tr->n, envs)), dim3(64 * WPW), shmem, st, arg, (float*)tr->d_obs, tr->d_act,
                               (float*)tr->d_rew, tr->d_mask, tr->d_len, tr->n, tr->horizon, t0, t1, wstream, tab, sg, rng, env_offset,
                               v.p->agents);
        };
        if (block_envs == 16) launch(fused_rollout_f32x16_kernel<EnvK, H, NHH, kAct>, 16);
        else launch(fused_rollout_f32_kernel<EnvK, H, NHH, kAct>, 32);
        TG_LAUNCH_CHECK(who);
        return TG_OK;
    });
}

template <template <typename> class EnvT, int kAct>
static int fused_f32_dispatch(const char* who, int hidden, int n_hh, const EnvVariant& v, const tg_traj* tr, const float* wstream,
                              const float* tab, const float* sigma, const uint64_t* rng, int64_t env_offset, int t0, int t1, int block_envs,
                              hipStream_t st) {
#define TG_F32_CASE(HH, NN) \
    case HH * 10 + NN: return fused_f32_launch<EnvT, HH, NN, kAct>(who, v, tr, wstream, tab, sigma, rng, env_offset, t0, t1, block_envs, st);
    switch (hidden * 10 + n_hh) {
        TG_F32_CASE(64, 0) TG_F32_CASE(64, 1) TG_F32_CASE(64, 2) TG_F32_CASE(64, 3)
        TG_F32_CASE(128, 0) TG_F32_CASE(128, 1) TG_F32_CASE(128, 2) TG_F32_CASE(128, 3)
        default: break;
    }
#undef TG_F32_CASE
    return set_error(TG_ERR_UNSUPPORTED, "%s: hidden width %d with %d hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)",
                     who, hidden, n_hh + 1);
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_fused_rollout_f32_supported(int32_t hidden, int32_t n_hidden_layers) {
    return (hidden == 64 || hidden == 128) && n_hidden_layers >= 1 && n_hidden_layers <= 4;
}

int tg_fused_rollout_f32_block_envs(int64_t n, int32_t agents) {
    // 16 envs per workgroup while that leaves no CU with two workgroups (and a swarm env's bodies fit a 16-lane group), else 32
    return (n <= (int64_t)16 * device_cus() && agents <= 16) ? 16 : 32;
}

// `who`: the name in every message (tg_fused_rollout_f32 through the plain, `_act`, `_dr` and `_on` entries, the entry's own through
// `_sub`).  Through `_sub`, `v.p` describes the physics clock (substeps_check).
static int fused_rollout_f32(const char* who, const EnvVariant& v, const tg_traj* tr, const float* d_wstream, const float* d_tab, int32_t hidden,
                             int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng, int64_t env_offset,
                             int32_t t_begin, int32_t t_end, int32_t activation, void* stream) {
    const tg_env_params* p = v.p;
    TG_REQUIRE(activation == TG_ACT_RELU || activation == TG_ACT_TANH, "%s: unknown activation %d", v.sub ? who : "tg_fused_rollout_f32_act",
               activation);
    TG_REQUIRE(p && tr && d_wstream && d_tab && sigma && d_rng, "%s: null pointer", who);
    TG_REQUIRE(tr->d_obs && tr->d_act && tr->d_rew && tr->d_mask && tr->d_len, "%s: null trajectory pointer", who);
    if (v.sub)
        if (int rc = substeps_check(who, p, tr, v.substeps)) return rc;
    TG_REQUIRE(v.d_obs_norm == nullptr || v.clip > 0.0f, "%s: clip %g (a number > 0; +inf: no clamp)", who, (double)v.clip);
    TG_REQUIRE(tr->dtype == TG_F32, "%s: float32 trajectories only", who);
    if (!v.sub) TG_REQUIRE(tr->n > 0 && tr->horizon == p->max_steps, "%s: horizon %d != env.max_steps %d", who, tr->horizon, p->max_steps);
    TG_REQUIRE(tr->n > 0 && 0 <= t_begin && t_begin <= t_end && t_end <= tr->horizon, "%s: bad step range [%d, %d)", who, t_begin, t_end);
    TG_REQUIRE(block_envs == 16 || block_envs == 32, "%s: %d envs per workgroup (16 or 32: the layout of d_wstream)", who, block_envs);
    TG_REQUIRE(p->agents <= 1 || (p->agents <= block_envs && (p->agents & (p->agents - 1)) == 0 && tr->n % p->agents == 0),
               "%s: agents=%d must be a power of two <= %d dividing n", who, p->agents, block_envs);
    if (t_begin == t_end) return TG_OK;
    const int n_hh = n_hidden_layers - 1;
    hipStream_t st = (hipStream_t)stream;
    switch (activation * 16 + p->env_id) {
#define TG_F32_ENV(ACT, ID, ENV)                                                                                                      \
    case ACT * 16 + ID:                                                                                                               \
        return fused_f32_dispatch<ENV, ACT>(who, hidden, n_hh, v, tr, d_wstream, d_tab, sigma, d_rng, env_offset, t_begin, t_end, block_envs, st);
        TG_F32_ENV(TG_ACT_RELU, TG_ENV_CARTPOLE, CartPoleEnv) TG_F32_ENV(TG_ACT_RELU, TG_ENV_QUADPOLE2D, QuadPole2DEnv)
        TG_F32_ENV(TG_ACT_RELU, TG_ENV_QUADPOLE, QuadPoleEnv) TG_F32_ENV(TG_ACT_RELU, TG_ENV_PENDULUM, PendulumEnv)
        TG_F32_ENV(TG_ACT_TANH, TG_ENV_CARTPOLE, CartPoleEnv) TG_F32_ENV(TG_ACT_TANH, TG_ENV_QUADPOLE2D, QuadPole2DEnv)
        TG_F32_ENV(TG_ACT_TANH, TG_ENV_QUADPOLE, QuadPoleEnv) TG_F32_ENV(TG_ACT_TANH, TG_ENV_PENDULUM, PendulumEnv)
#undef TG_F32_ENV
        default: return set_error(TG_ERR_UNSUPPORTED, "%s: env %d is not instantiated", who, p->env_id);
    }
}

static EnvVariant f32_variant(const tg_env_params* p, const double* d_ptab, const float* d_obs_norm, float clip) {
    return EnvVariant{p, d_ptab, d_obs_norm, clip, 1, false};
}

int tg_fused_rollout_f32(const tg_env_params* p, const tg_traj* tr, const float* d_wstream, const float* d_tab, int32_t hidden,
                         int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng, int64_t env_offset,
                         int32_t t_begin, int32_t t_end, void* stream) {
    return fused_rollout_f32("tg_fused_rollout_f32", f32_variant(p, nullptr, nullptr, 0.0f), tr, d_wstream, d_tab, hidden, n_hidden_layers, block_envs,
                             sigma, d_rng, env_offset, t_begin, t_end, TG_ACT_RELU, stream);
}

int tg_fused_rollout_f32_act(const tg_env_params* p, const tg_traj* tr, const float* d_wstream, const float* d_tab, int32_t hidden,
                             int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng, int64_t env_offset,
                             int32_t t_begin, int32_t t_end, int32_t activation, void* stream) {
    return fused_rollout_f32("tg_fused_rollout_f32", f32_variant(p, nullptr, nullptr, 0.0f), tr, d_wstream, d_tab, hidden, n_hidden_layers, block_envs,
                             sigma, d_rng, env_offset, t_begin, t_end, activation, stream);
}

int tg_fused_rollout_f32_dr(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                            int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                            int64_t env_offset, int32_t t_begin, int32_t t_end, void* stream) {
    TG_REQUIRE(d_ptab != nullptr, "tg_fused_rollout_f32_dr: null parameter table");
    return fused_rollout_f32("tg_fused_rollout_f32", f32_variant(p, d_ptab, nullptr, 0.0f), tr, d_wstream, d_tab, hidden, n_hidden_layers, block_envs,
                             sigma, d_rng, env_offset, t_begin, t_end, TG_ACT_RELU, stream);
}

int tg_fused_rollout_f32_act_dr(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                                int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                                int64_t env_offset, int32_t t_begin, int32_t t_end, int32_t activation, void* stream) {
    TG_REQUIRE(d_ptab != nullptr, "tg_fused_rollout_f32_act_dr: null parameter table");
    return fused_rollout_f32("tg_fused_rollout_f32", f32_variant(p, d_ptab, nullptr, 0.0f), tr, d_wstream, d_tab, hidden, n_hidden_layers, block_envs,
                             sigma, d_rng, env_offset, t_begin, t_end, activation, stream);
}

int tg_fused_rollout_f32_on(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                            int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                            int64_t env_offset, int32_t t_begin, int32_t t_end, int32_t activation, const float* d_obs_norm, float clip,
                            void* stream) {
    TG_REQUIRE(d_obs_norm != nullptr, "tg_fused_rollout_f32_on: null observation-normalisation table");
    TG_REQUIRE(clip > 0.0f, "tg_fused_rollout_f32_on: clip %g (a number > 0; +inf: no clamp)", (double)clip);
    return fused_rollout_f32("tg_fused_rollout_f32", f32_variant(p, d_ptab, d_obs_norm, clip), tr, d_wstream, d_tab, hidden, n_hidden_layers, block_envs,
                             sigma, d_rng, env_offset, t_begin, t_end, activation, stream);
}

int tg_fused_rollout_f32_sub(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                             int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                             int64_t env_offset, int32_t t_begin, int32_t t_end, int32_t activation, const float* d_obs_norm, float clip,
                             int32_t substeps, void* stream) {
    return fused_rollout_f32("tg_fused_rollout_f32_sub", EnvVariant{p, d_ptab, d_obs_norm, clip, substeps, true}, tr, d_wstream, d_tab, hidden,
                             n_hidden_layers, block_envs, sigma, d_rng, env_offset, t_begin, t_end, activation, stream);
}

// The `_sub` entry plus the motor record (lag_check first: a refused lag launches nothing).
int tg_fused_rollout_f32_lag(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                             int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                             int64_t env_offset, int32_t t_begin, int32_t t_end, int32_t activation, const float* d_obs_norm, float clip,
                             int32_t substeps, float* d_motor, void* stream) {
    TG_REQUIRE(p != nullptr, "tg_fused_rollout_f32_lag: null pointer");
    if (int rc = lag_check("tg_fused_rollout_f32_lag", p, d_ptab, d_motor)) return rc;
    return fused_rollout_f32("tg_fused_rollout_f32_lag", EnvVariant{p, d_ptab, d_obs_norm, clip, substeps, true, d_motor}, tr, d_wstream, d_tab,
                             hidden, n_hidden_layers, block_envs, sigma, d_rng, env_offset, t_begin, t_end, activation, stream);
}

}  // extern "C"
