// Vector env for gfx950 (tg_vec_env_step, tg_vec_env_reset_all): n auto-resetting env slots, one lane per slot, one launch per step.
// The slots sit at different positions of their episodes: the step count `t` is per lane, read from device memory, and a slot whose
// episode ends is reset in the same launch (gymnasium's SAME_STEP mode).  No step arithmetic lives here: the kernel calls the env's
// own step / failed / time_rule / reset and the substep loops of env_dynamics.hpp as rollout_step_kernel does for a running episode,
// so episode k of slot i is, bit for bit, what the rollout kernels make of the same initial state and actions.
#include "env_dynamics.hpp"
#include "row_store.hpp"

#include <stdint.h>

namespace tg {

// what persists per slot between steps (struct of arrays, env fastest) and what is fixed per object
struct VecSlots {
    void* state;             // R [S][n]
    int32_t* steps;          // control steps taken in the current episode
    int32_t* balanced;       // Pendulum: consecutive balanced steps
    double* ep_return;
    uint32_t* episode;       // ordinal of the current episode = stream id of its reset draw
    int64_t n, env_offset;
    uint64_t seed;
    int32_t T;               // control-step horizon
    int32_t variant;         // Pendulum: swingup start (reset_kernel's argument)
};

struct VecOut {
    float* obs;              // [n][S]
    float* reward;
    uint8_t* terminated;
    uint8_t* truncated;
    float* final_obs;        // [n][S]
    float* final_return;
    int32_t* final_length;
};

constexpr int kVecBlockMax = 256;

// row i of a row-major f32 [n][A] array in one load of 4 A bytes
template <int A> __device__ static inline void load_action_row(const float* __restrict__ act, int64_t i, float (&a)[A]) {
    if constexpr (A == 4) {
        const float4 v = *reinterpret_cast<const float4*>(act + i * 4);
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    } else if constexpr (A == 2) {
        const float2 v = *reinterpret_cast<const float2*>(act + i * 2);
        a[0] = v.x; a[1] = v.y;
    } else {
#pragma unroll
        for (int k = 0; k < A; ++k) a[k] = act[i * A + k];
    }
}

// The state tg_env_reset draws for global env `key` in stream `stream_id` (reset_kernel's body).  Env::reset, unlike Env::step, is
// compiled with floating-point contraction allowed, so its bits depend on which multiplies the compiler fuses.  reset_kernel, the
// yardstick, gets scalar code: one multiply and three FMAs for QuadPole's quaternion norm.  Inlined here the SLP vectoriser packed
// that sum into v_pk_mul_f32 and plain adds (1 ulp apart), so this translation unit is built with -fno-slp-vectorize (csrc/Makefile):
// the draw then compiles as it does in reset_kernel, and tests/test_vec_env_gpu.py holds every initial state to tg_env_reset's bits.
// (The step functions have contraction off: vectorised or not, their bits are the same.)
template <typename Env, typename R>
__device__ static inline void reset_draw(uint64_t seed, uint64_t key, uint32_t stream_id, int variant, R (&o)[Env::S]) {
    uint32_t rnd[4];
    Philox::draw(seed, key, 0xFFFFFFFFu /* sub = reset */, stream_id, rnd);
    if constexpr (Env::kBalanceTerminates) Env::reset(rnd, o, variant);
    else Env::reset(rnd, o);
}

template <typename Env, typename R>
__global__ __launch_bounds__(kVecBlockMax) void vec_step_kernel(typename Env::C c_arg, VecSlots v, const float* __restrict__ actions,
                                                                 VecOut out) {
#pragma clang fp contract(off)
    constexpr int S = Env::S, A = Env::A;
    extern __shared__ float4 vec_lds[];                                    // blockDim.x rows of S floats: 64 S per wave
    float* lds_wave = reinterpret_cast<float*>(vec_lds) + (threadIdx.x >> 6) * 64 * S;
    const int64_t n = v.n;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row0 = i - (threadIdx.x & 63);                          // the wave's first slot (a wave wholly beyond n stores nothing)
    const bool in_range = i < n;
    const int64_t ic = in_range ? i : n - 1;                               // clamp: every lane's addresses are valid, every lane stays
    R* __restrict__ state = (R*)v.state;

    constexpr bool kPerEnv = EnvTraits<Env>::kPerEnv;
    typename EnvTraits<Env>::Consts own;
    if constexpr (kPerEnv) own = env_constants<Env>(env_arg(c_arg), n, ic);
    const auto& c = pick_constants(env_arg(c_arg), own);
    constexpr bool kLag = EnvTraits<Env>::kLag;
    float m[A], alpha = 0.0f;
    if constexpr (kLag) {
        alpha = lag_alpha_of<Env>(c_arg, n, ic);
#pragma unroll
        for (int k = 0; k < A; ++k) m[k] = lag_of(c_arg).motor[k * n + ic];
    }
    const int32_t t = v.steps[ic];
    const uint32_t episode = v.episode[ic];
    const double ret_in = v.ep_return[ic];
    int32_t balanced_in = 0;
    if constexpr (Env::kBalanceTerminates) balanced_in = v.balanced[ic];
    R s[S], o[S];
    float a[A];
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] = state[k * n + ic];
    load_action_row<A>(actions, ic, a);

    R r;
    StepOut so;
    int count = t + 1;                                                      // the clock the time rule reads: physics steps under kSubsteps
    if constexpr (kLag) {
        so = lagged_substep_loop<Env>(s, a, c, t, substeps_of(c_arg), true, alpha, m, o, r, count);
    } else if constexpr (EnvTraits<Env>::kSubsteps) {
        so = substep_loop<Env>(s, a, c, t, substeps_of(c_arg), true, o, r, count);
    } else {
        so = Env::step(s, a, c, t + 1, o, r);
    }
    bool ended = so.truncated;
    int32_t balanced_steps = 0;
    if constexpr (Env::kBalanceTerminates) {
        balanced_steps = so.balanced ? balanced_in + 1 : 0;
        ended = ended || (balanced_steps >= c.term_steps);
    }
    ended = ended || (t + 1 >= v.T);                                        // the worker's stop at t == max_steps
    const bool timeout = !Env::failed(o, c) && (Env::time_rule(count, c) || t + 1 == v.T);
    const double ret = ret_in + (double)r;

    float row[S];
    const bool any_ended = __ballot(ended && in_range) != 0ull;            // (wave-uniform)
    if (any_ended) {
#pragma unroll
        for (int k = 0; k < S; ++k) row[k] = (float)o[k];
        store_rows_staged<S>(out.final_obs, row0, n, row, lds_wave);
        R fresh[S];
        reset_draw<Env, R>(v.seed, (uint64_t)(v.env_offset + ic), episode + 1u, v.variant, fresh);
#pragma unroll
        for (int k = 0; k < S; ++k) o[k] = ended ? fresh[k] : o[k];
    }
#pragma unroll
    for (int k = 0; k < S; ++k) row[k] = (float)o[k];
    store_rows_staged<S>(out.obs, row0, n, row, lds_wave);

    if (in_range) {
#pragma unroll
        for (int k = 0; k < S; ++k) state[k * n + i] = o[k];
        v.steps[i] = ended ? 0 : t + 1;
        v.ep_return[i] = ended ? 0.0 : ret;
        if constexpr (Env::kBalanceTerminates) v.balanced[i] = ended ? 0 : balanced_steps;
        if constexpr (kLag) {
#pragma unroll
            for (int k = 0; k < A; ++k) lag_of(c_arg).motor[k * n + i] = ended ? 0.0f : m[k];
        }
        out.reward[i] = (float)r;
        out.terminated[i] = (ended && !timeout) ? 1 : 0;
        out.truncated[i] = (ended && timeout) ? 1 : 0;
        if (ended) {
            v.episode[i] = episode + 1u;
            out.final_return[i] = (float)ret;
            out.final_length[i] = t + 1;
        }
    }
}

template <typename Env, typename R>
__global__ __launch_bounds__(kVecBlockMax) void vec_reset_kernel(VecSlots v, float* __restrict__ motor, int32_t restart,
                                                                  float* __restrict__ obs) {
    constexpr int S = Env::S, A = Env::A;
    extern __shared__ float4 vec_lds[];                                    // blockDim.x rows of S floats: 64 S per wave
    float* lds_wave = reinterpret_cast<float*>(vec_lds) + (threadIdx.x >> 6) * 64 * S;
    const int64_t n = v.n;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row0 = i - (threadIdx.x & 63);
    const bool in_range = i < n;
    const int64_t ic = in_range ? i : n - 1;
    const uint32_t episode = restart ? 0u : v.episode[ic] + 1u;
    R o[S];
    reset_draw<Env, R>(v.seed, (uint64_t)(v.env_offset + ic), episode, v.variant, o);
    float row[S];
#pragma unroll
    for (int k = 0; k < S; ++k) row[k] = (float)o[k];
    store_rows_staged<S>(obs, row0, n, row, lds_wave);
    if (in_range) {
        R* __restrict__ state = (R*)v.state;
#pragma unroll
        for (int k = 0; k < S; ++k) state[k * n + i] = o[k];
        v.steps[i] = 0;
        v.balanced[i] = 0;
        v.ep_return[i] = 0.0;
        v.episode[i] = episode;
        if (motor != nullptr) {
#pragma unroll
            for (int k = 0; k < A; ++k) motor[k * n + i] = 0.0f;
        }
    }
}

template <typename Env> static inline size_t vec_lds_bytes(int block) { return (size_t)block * Env::S * sizeof(float); }

static VecSlots vec_slots(const tg_env_params* p, const tg_vec_env* v) {
    return VecSlots{v->d_state, v->d_steps, v->d_balanced, v->d_ep_return, v->d_episode, v->n, v->env_offset, v->seed, v->horizon,
                    (int32_t)(p->p[3] != 0.0)};
}

template <template <typename> class EnvT, typename R>
static int vec_step_dispatch(const EnvVariant& ev, const tg_vec_env* v, const float* actions, const VecOut& out, hipStream_t st) {
    int block;
    dim3 grid = env_grid(v->n, block);
    const VecSlots slots = vec_slots(ev.p, v);
    return with_env_variant<EnvT<R>, /*kMayObsNorm=*/false>(ev, [&](auto tag, const auto& arg) -> int {
        using EnvK = typename decltype(tag)::type;
        hipLaunchKernelGGL((vec_step_kernel<EnvK, R>), grid, dim3(block), vec_lds_bytes<EnvT<R>>(block), st, arg, slots, actions, out);
        TG_LAUNCH_CHECK("tg_vec_env_step");
        return TG_OK;
    });
}

template <template <typename> class EnvT, typename R>
static int vec_reset_dispatch(const tg_env_params* p, const tg_vec_env* v, float* motor, int32_t restart, float* obs, hipStream_t st) {
    int block;
    dim3 grid = env_grid(v->n, block);
    hipLaunchKernelGGL((vec_reset_kernel<EnvT<R>, R>), grid, dim3(block), vec_lds_bytes<EnvT<R>>(block), st, vec_slots(p, v), motor, restart, obs);
    TG_LAUNCH_CHECK("tg_vec_env_reset_all");
    return TG_OK;
}

// what both entries refuse about the object itself
static int vec_env_check(const char* who, const tg_env_params* p, const tg_vec_env* v) {
    TG_REQUIRE(p && v && v->d_state && v->d_steps && v->d_balanced && v->d_ep_return && v->d_episode, "%s: null pointer", who);
    TG_REQUIRE(v->n > 0 && v->horizon > 0 && v->env_offset >= 0, "%s: bad sizes n=%lld horizon=%d env_offset=%lld", who,
               (long long)v->n, v->horizon, (long long)v->env_offset);
    if (p->agents > 1)
        return set_error(TG_ERR_UNSUPPORTED, "%s: swarm envs (agents=%d) are not supported: the bodies of an env would have to end "
                         "and reset together", who, p->agents);
    if (p->env_id != TG_ENV_CARTPOLE && p->env_id != TG_ENV_QUADPOLE2D && p->env_id != TG_ENV_QUADPOLE && p->env_id != TG_ENV_PENDULUM)
        return set_error(TG_ERR_UNSUPPORTED, "%s: unsupported env_id %d", who, p->env_id);
    if (v->dtype != TG_F32 && v->dtype != TG_F64) return set_error(TG_ERR_UNSUPPORTED, "%s: unsupported dtype %d", who, v->dtype);
    return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_vec_env_step(const tg_env_params* p, const double* d_ptab, int32_t substeps, float* d_motor, const tg_vec_env* v,
                    const float* d_actions, float* d_obs, float* d_reward, uint8_t* d_terminated, uint8_t* d_truncated,
                    float* d_final_obs, float* d_final_return, int32_t* d_final_length, void* stream) {
    const char* who = "tg_vec_env_step";
    TG_REQUIRE(d_actions && d_obs && d_reward && d_terminated && d_truncated && d_final_obs && d_final_return && d_final_length,
               "%s: null pointer", who);
    if (int rc = vec_env_check(who, p, v)) return rc;
    TG_REQUIRE(substeps >= 1 && substeps <= 64, "%s: substeps=%d outside [1, 64]", who, substeps);
    if (substeps != 1 && p->env_id == TG_ENV_PENDULUM)
        return set_error(TG_ERR_UNSUPPORTED, "%s: Pendulum takes substeps = 1 only: its balance terminal counts single steps", who);
    if (d_motor != nullptr)
        if (int rc = lag_check(who, p, d_ptab, d_motor)) return rc;
    TG_REQUIRE((int64_t)v->horizon * substeps == (int64_t)p->max_steps,
               "%s: horizon %d x substeps %d != env.max_steps %d (the params describe the physics clock)", who, v->horizon, substeps,
               p->max_steps);
    TG_REQUIRE((((uintptr_t)d_obs | (uintptr_t)d_final_obs) & 15) == 0, "%s: d_obs and d_final_obs must be 16-byte aligned", who);
    int S, A;
    tg_env_dims(p->env_id, &S, &A);
    TG_REQUIRE(((uintptr_t)d_actions & (uintptr_t)(4 * A - 1)) == 0, "%s: d_actions must be aligned to a row (%d bytes)", who, 4 * A);
    // Substepped<> only when asked for: with everything off the launch is the plain instantiation
    const EnvVariant ev{p, d_ptab, nullptr, 0.0f, substeps, substeps != 1 || d_motor != nullptr, d_motor};
    const VecOut out{d_obs, d_reward, d_terminated, d_truncated, d_final_obs, d_final_return, d_final_length};
#define CALL(E, R) vec_step_dispatch<E, R>(ev, v, d_actions, out, (hipStream_t)stream)
    TG_ENV_SWITCH(p->env_id, v->dtype, CALL)
#undef CALL
}

int tg_vec_env_reset_all(const tg_env_params* p, float* d_motor, const tg_vec_env* v, int32_t restart, float* d_obs, void* stream) {
    const char* who = "tg_vec_env_reset_all";
    TG_REQUIRE(d_obs != nullptr, "%s: null pointer", who);
    if (int rc = vec_env_check(who, p, v)) return rc;
    if (d_motor != nullptr && p->env_id != TG_ENV_QUADPOLE2D && p->env_id != TG_ENV_QUADPOLE)
        return set_error(TG_ERR_UNSUPPORTED, "%s: env %d has no rotors to lag (QuadPole2D and QuadPole only)", who, p->env_id);
    TG_REQUIRE(((uintptr_t)d_obs & 15) == 0, "%s: d_obs must be 16-byte aligned", who);
#define CALL(E, R) vec_reset_dispatch<E, R>(p, v, d_motor, restart, d_obs, (hipStream_t)stream)
    TG_ENV_SWITCH(p->env_id, v->dtype, CALL)
#undef CALL
}

}  // extern "C"
