// Per-environment single-step maps as device functions, templated on the arithmetic type
// R (float for production, double for exactness checks against the fp64 reference).
//
// The reference computes the *wrapped control* in float32 (NumPy keeps
// `hover + hover*np.clip(action,-1,1)` in the float32 dtype of the policy's action) and the
// rest in float64.  That float32 control path is reproduced with individually rounded
// rn_mul/rn_add so the double build agrees with the reference to rounding noise.
//
// Citations: environments/cartpole_env.py, environments/quadrotor_env.py of the reference.
#pragma once
#include "tg_common.hpp"

#include <type_traits>

namespace tg {

// div_/inv_sqrt_/norm2_: the double build keeps the reference's exact operation order (division, sqrt then
// square); the float build uses the 1-ulp hardware reciprocal / rsqrt (v_rcp_f32, v_rsq_f32): a few fp32 ulp
// per step, far inside the fp32-vs-fp64 trajectory noise, and ~half the VALU work of the kernel.
template <typename R> struct Math;
template <> struct Math<float> {
    static constexpr bool kFast = true;
    __device__ static inline float div_(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
    __device__ static inline float inv_sqrt_(float x) { return __builtin_amdgcn_rsqf(x); }
    __device__ static inline float sqrt_(float x) { return sqrtf(x); }
    __device__ static inline float atan2_(float y, float x) { return atan2f(y, x); }
    __device__ static inline void sincos_(float x, float* s, float* c) { sincosf(x, s, c); }
    __device__ static inline float abs_(float x) { return fabsf(x); }
    __device__ static inline float tan_(float x) { return tanf(x); }
};
template <> struct Math<double> {
    static constexpr bool kFast = false;
    __device__ static inline double div_(double a, double b) { return a / b; }
    __device__ static inline double inv_sqrt_(double x) { return 1.0 / sqrt(x); }
    __device__ static inline double sqrt_(double x) { return sqrt(x); }
    __device__ static inline double atan2_(double y, double x) { return atan2(y, x); }
    __device__ static inline void sincos_(double x, double* s, double* c) { sincos(x, s, c); }
    __device__ static inline double abs_(double x) { return fabs(x); }
    __device__ static inline double tan_(double x) { return tan(x); }
};

__device__ static inline float clip1(float a) { return fminf(fmaxf(a, -1.0f), 1.0f); }

struct StepOut {
    bool truncated;   // env-level `truncated`
    bool balanced;    // bonus condition held on the new state (drives info['time_balanced'])
};
// `terminated` is always False except for Pendulum, whose episode ends once it has been balanced for more than 5 s
// (pendulum_env.py:151).  Such an env sets kBalanceTerminates and carries `term_steps` in its constants: the number
// of CONSECUTIVE balanced steps after which the fp64-accumulated `_time_balanced` first exceeds the limit.  The
// rollout kernels keep the running count (as -len[env] while the episode runs).

// Time-limit bootstrapping (tg_rollout_final_state) needs to know WHY an episode ended: every env states the two clauses of its
// `truncated` separately as well -- failed(o, c): the failure test on the new state; time_rule(steps_after, c): the clock test.
// The same comparisons as in step(), which does not call them (its code is what it was).

// Per-env domain randomisation (tg_env_randomize and the `_dr` entry points).  Every env's constants C are a function of the twelve
// p[] values of tg_env_params plus timestep / max_steps / time_trunc_step: `C::build`, __host__ __device__, plain IEEE double
// operations with contraction off, so the host (`C::make`, one vehicle for the whole launch, passed by value in the kernel
// arguments) and a lane that builds the C of its own env slot from its column of the parameter table produce the same bits.
// PerEnvTable is what a `_dr` kernel takes in place of the by-value C: the table f64 [12][n] (env fastest) and the fields that
// are not randomised.
struct PerEnvTable {
    const double* ptab;
    double timestep;
    int32_t max_steps, time_trunc_step;
};
// PerEnv<Env> is Env with the table in place of the by-value constants: a kernel template instantiated with it IS the kPerEnv = true
// kernel, while its instantiation with the plain Env stays the very kernel it was (the flag rides on the Env type because a
// further template parameter would change the mangled name of every existing instantiation).  step / failed / time_rule / reset
// are inherited untouched and keep taking the env's own C.
template <typename Env> struct PerEnv : Env {
    using C = PerEnvTable;
};
template <typename Env> struct EnvTraits {
    static constexpr bool kPerEnv = false;
    static constexpr bool kObsNorm = false;
    static constexpr bool kSubsteps = false;
    static constexpr bool kLag = false;
    using Consts = typename Env::C;
};
template <typename Env> struct EnvTraits<PerEnv<Env>> {
    static constexpr bool kPerEnv = true;
    static constexpr bool kObsNorm = false;
    static constexpr bool kSubsteps = false;
    static constexpr bool kLag = false;
    using Consts = typename Env::C;
};
// Control decimation (the `_sub` entry points): `k` physics steps per policy step.  Substepped<Env> -- Env a plain env or PerEnv<...>,
// and ObsNormed<> goes AROUND it -- rides on the Env type for PerEnv's reason: the kernel's argument becomes {Env's own argument, k},
// its instantiation IS the kSubsteps = true kernel (the step call site runs substep_loop below in place of one Env::step), and every
// existing instantiation keeps name and code.  The constants describe the PHYSICS clock (max_steps = horizon * k, dt = the physics
// step); the kernel's t, T, the Philox key and len count control steps.
template <typename BaseC> struct SubstepArg {
    BaseC base;
    int32_t k;
};
template <typename Env> struct Substepped : Env {
    using C = SubstepArg<typename Env::C>;
};
template <typename Env> struct EnvTraits<Substepped<Env>> {
    static constexpr bool kPerEnv = EnvTraits<Env>::kPerEnv;
    static constexpr bool kObsNorm = false;
    static constexpr bool kSubsteps = true;
    static constexpr bool kLag = false;
    using Consts = typename EnvTraits<Env>::Consts;
};
// Actuator lag (the `_lag` entry points): a first-order rotor lag in front of every physics step.  Lagged<Env> -- Env ALWAYS a
// Substepped<...> (also at k = 1: the lag lives in the substep loop, so it adds one instantiation per substepped one, not two), and
// ObsNormed<> goes around it -- rides on the Env type for PerEnv's reason.  The kernel's argument becomes {Substepped's argument, the
// motor record f32 [A][T+1][n] (env fastest; slot t = the motor state at the start of control step t), alpha}: `alpha` is the
// filter gain of the one vehicle of a launch without a parameter table, lag_alpha(p[10], timestep) built on the host; with a table
// the lane builds its own from row 10 (lag_alpha_of), where it builds its own constants.
template <typename BaseC> struct LagArg {
    BaseC base;
    float* motor;
    float alpha;
};
template <typename Env> struct Lagged : Env {
    using C = LagArg<typename Env::C>;
};
template <typename Env> struct EnvTraits<Lagged<Env>> {
    static constexpr bool kPerEnv = EnvTraits<Env>::kPerEnv;
    static constexpr bool kObsNorm = false;
    static constexpr bool kSubsteps = true;
    static constexpr bool kLag = true;
    using Consts = typename EnvTraits<Env>::Consts;
};
constexpr int kLagSlot = 10;                                // the p[] slot (and parameter-table row) that holds the time constant
// alpha = dt / (tau + dt), the backward-Euler gain of dm/dt = (c - m) / tau: one IEEE double add and divide, rounded to float once
// -- the same bits on the host and in a lane (C::build relies on the same).
__host__ __device__ static inline float lag_alpha(double tau, double dt) {
#pragma clang fp contract(off)
    return (float)(dt / (tau + dt));
}
// Running observation normalisation (the `_on` entry points of the fused rollouts).  ObsNormed<Env> -- Env a plain env or PerEnv<...>
// -- rides on the Env type for PerEnv's reason: the kernel's argument becomes {Env's own argument, the f32 table [2][S] = {mean,
// rstd}, the clamp}, its instantiation IS the kObsNorm = true kernel, and every existing instantiation keeps name and code.
struct ObsNormTable {
    const float* tab;
    float clip;                                  // +inf: no clamp
};
template <typename BaseC> struct ObsNormArg {
    BaseC base;
    ObsNormTable on;
};
template <typename Env> struct ObsNormed : Env {
    using C = ObsNormArg<typename Env::C>;
};
template <typename Env> struct EnvTraits<ObsNormed<Env>> {
    static constexpr bool kPerEnv = EnvTraits<Env>::kPerEnv;
    static constexpr bool kObsNorm = true;
    static constexpr bool kSubsteps = EnvTraits<Env>::kSubsteps;
    static constexpr bool kLag = EnvTraits<Env>::kLag;
    using Consts = typename EnvTraits<Env>::Consts;
};
// the env's own kernel argument (by-value constants or the parameter table) inside whatever the kernel was handed
template <typename C> __device__ static inline const C& env_arg(const C& c) { return c; }
template <typename B> __device__ static inline const B& env_arg(const SubstepArg<B>& c) { return c.base; }
template <typename B> __device__ static inline const auto& env_arg(const LagArg<B>& c) { return env_arg(c.base); }
template <typename B> __device__ static inline const auto& env_arg(const ObsNormArg<B>& c) { return env_arg(c.base); }
// the physics steps per control step of a kSubsteps kernel, from the same argument
template <typename B> __device__ static inline int substeps_of(const SubstepArg<B>& c) { return c.k; }
template <typename B> __device__ static inline int substeps_of(const LagArg<B>& c) { return substeps_of(c.base); }
template <typename B> __device__ static inline int substeps_of(const ObsNormArg<B>& c) { return substeps_of(c.base); }
// the motor record and the uniform gain of a kLag kernel, from the same argument
template <typename B> __device__ static inline const LagArg<B>& lag_of(const LagArg<B>& c) { return c; }
template <typename B> __device__ static inline const auto& lag_of(const ObsNormArg<B>& c) { return lag_of(c.base); }
// The policy's view of a state: the table's 2 S floats, read once per launch (uniform addresses: scalar loads), and the one
// definition of the normalised observation (obs_normalize, tg_common.hpp) applied to the register-resident state where it becomes
// the first layer's operand.  The table is per FEATURE, not per env: a compaction that moves envs between lanes moves nothing here.
template <int S> struct ObsNormRegs {
    float mean[S], rstd[S], clip;
    __device__ inline void load(const ObsNormTable& t) {
#pragma unroll
        for (int k = 0; k < S; ++k) { mean[k] = t.tab[k]; rstd[k] = t.tab[S + k]; }
        clip = t.clip;
    }
    __device__ inline float apply(float x, int k) const { return obs_normalize(x, mean[k], rstd[k], clip); }
};
// the constants of env slot i, built by the lane that owns it from column i of the table
template <typename Env>
__device__ static inline typename EnvTraits<Env>::Consts env_constants(const PerEnvTable& pe, int64_t n, int64_t i) {
    double q[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) q[k] = pe.ptab[k * n + i];     // (rows an env does not read cost nothing: dead loads)
    return EnvTraits<Env>::Consts::build(q, pe.timestep, pe.max_steps, pe.time_trunc_step);
}
// The constants a kernel steps with: its by-value argument (kPerEnv = false), or the lane's own (kPerEnv = true).
template <typename C> __device__ static inline const C& pick_constants(const C& uniform, const C&) { return uniform; }
template <typename C> __device__ static inline const C& pick_constants(const PerEnvTable&, const C& own) { return own; }
// the filter gain of env slot i of a kLag kernel: the launch's one (no table), or built from column i of row kLagSlot
template <typename Env, typename CArg> __device__ static inline float lag_alpha_of(const CArg& c_arg, int64_t n, int64_t i) {
    if constexpr (EnvTraits<Env>::kPerEnv) {
        const PerEnvTable& pe = env_arg(c_arg);
        return lag_alpha(pe.ptab[kLagSlot * n + i], pe.timestep);
    } else {
        return lag_of(c_arg).alpha;
    }
}
static inline PerEnvTable per_env_table(const tg_env_params* p, const double* d_ptab) {
    return PerEnvTable{d_ptab, p->timestep, p->max_steps, p->time_trunc_step};
}

// The variant of a rollout kernel that an entry point asked for, and the ONE place that turns it into the kernel's Env type and
// by-value first argument.  The wrappers nest in a fixed order -- PerEnv<> innermost, Substepped<> around it, ObsNormed<> around both
// -- and every launch of a kernel templated on the Env type goes through with_env_variant, so no caller spells a nesting out.
struct EnvVariant {
    const tg_env_params* p;
    const double* d_ptab;        // non-null (the `_dr` entries): PerEnv<>, the table in place of the constants
    const float* d_obs_norm;     // non-null (the `_on` entries): ObsNormed<>, with `clip`
    float clip;
    int32_t substeps;
    bool sub;                    // entered through a `_sub` or `_lag` entry: Substepped<>, also at substeps == 1
    float* d_motor = nullptr;    // non-null (the `_lag` entries, which set `sub`): Lagged<> around Substepped<>
};
template <typename EnvK> struct EnvTag { using type = EnvK; };
// Calls f(EnvTag<EnvK>{}, arg) -- arg the `typename EnvK::C` of the variant -- for the one EnvK in {Env, PerEnv<Env>, ObsNormed<..>,
// Substepped<..>, Lagged<Substepped<..>>, ObsNormed<Substepped<..>>, ObsNormed<Lagged<Substepped<..>>>} that `v` names, and returns
// f's status.  kMayObsNorm / kMaySubstep / Env::kMayLag = false prune the wrapper at compile time (a kernel family or an env
// without those instantiations); a variant that asks for a pruned one is refused.
template <typename Env, bool kMayObsNorm, bool kMaySubstep = Env::kMaySubstep, typename F>
static inline int with_env_variant(const EnvVariant& v, F&& f) {
    auto normed = [&](auto tag, const auto& arg) -> int {
        using E = typename decltype(tag)::type;
        if (v.d_obs_norm == nullptr) return f(tag, arg);
        if constexpr (kMayObsNorm) return f(EnvTag<ObsNormed<E>>{}, ObsNormArg<typename E::C>{arg, ObsNormTable{v.d_obs_norm, v.clip}});
        else return set_error(TG_ERR_UNSUPPORTED, "observation normalisation is not instantiated for this kernel");
    };
    auto substepped = [&](auto tag, const auto& arg) -> int {
        using E = typename decltype(tag)::type;
        if (!v.sub) return normed(tag, arg);
        if constexpr (kMaySubstep) {
            const SubstepArg<typename E::C> sub{arg, v.substeps};
            if (v.d_motor == nullptr) return normed(EnvTag<Substepped<E>>{}, sub);
            if constexpr (Env::kMayLag)
                return normed(EnvTag<Lagged<Substepped<E>>>{},
                              LagArg<SubstepArg<typename E::C>>{sub, v.d_motor, lag_alpha(v.p->p[kLagSlot], v.p->timestep)});
            else return set_error(TG_ERR_UNSUPPORTED, "the actuator lag is not instantiated for this env");
        } else {
            return set_error(TG_ERR_UNSUPPORTED, "substeps are not instantiated for this env");
        }
    };
    if (v.d_ptab != nullptr) return substepped(EnvTag<PerEnv<Env>>{}, per_env_table(v.p, v.d_ptab));
    return substepped(EnvTag<Env>{}, Env::C::make(*v.p));
}

// One control step of a kSubsteps kernel: the action `a` applied for up to `k` consecutive calls of the env's own Env::step, call j
// (from 0) of control step t with steps_after = t k + j + 1, stopping after the first call that reports `truncated`.  Returns the
// last executed call's StepOut, with its state in `o`, the left-to-right sum of the executed calls' rewards in `reward` (in R,
// contraction off) and the physics count it stopped at in `count`.  The loop is wave-uniform: a lane that has stopped (or never ran:
// `alive` false) sits the remaining calls out, and the wave leaves when none of its lanes runs.  k = 1 is one Env::step, bit for bit.
template <typename Env, typename R, typename C>
__device__ static inline StepOut substep_loop(const R (&s)[Env::S], const float (&a)[Env::A], const C& c, int t, int k, bool alive,
                                              R (&o)[Env::S], R& reward, int& count) {
#pragma clang fp contract(off)
    constexpr int S = Env::S;
#pragma unroll
    for (int i = 0; i < S; ++i) o[i] = s[i];
    StepOut out;
    out.truncated = false; out.balanced = false;
    R sum = (R)0;
    int cnt = t * k;
    bool running = alive;
#pragma clang loop unroll(disable)
    for (int j = 0; j < k; ++j) {
        if (__ballot(running) == 0ull) break;
        R nx[S], r;
        const StepOut so = Env::step(o, a, c, t * k + j + 1, nx, r);
        if (running) {
            out = so;
            sum = (j == 0) ? r : sum + r;
            cnt = t * k + j + 1;
#pragma unroll
            for (int i = 0; i < S; ++i) o[i] = nx[i];
        }
        running = running && !so.truncated;
    }
    reward = sum;
    count = cnt;
    return out;
}

// One control step of a kLag kernel: substep_loop with the rotor lag in front of every call.  `m` (normalised action units, 0 = hover
// thrust) is the motor state at the start of the control step and, on return, after the executed calls:
//   m[k] <- m[k] + alpha * (clip1(a[k]) - m[k])        (three float32 operations, each rounded on its own)
// then Env::step(o, m, ...), the env's own step (m lies in [-1, 1]: its clip1 is the identity).  A lane that has stopped filters no
// more; with alive == false `m` comes back as it went in.  Everything else is substep_loop's rule, word for word.
template <typename Env, typename R, typename C>
__device__ static inline StepOut lagged_substep_loop(const R (&s)[Env::S], const float (&a)[Env::A], const C& c, int t, int k, bool alive,
                                                     float alpha, float (&m)[Env::A], R (&o)[Env::S], R& reward, int& count) {
#pragma clang fp contract(off)
    constexpr int S = Env::S, A = Env::A;
#pragma unroll
    for (int i = 0; i < S; ++i) o[i] = s[i];
    StepOut out;
    out.truncated = false; out.balanced = false;
    R sum = (R)0;
    int cnt = t * k;
    bool running = alive;
#pragma clang loop unroll(disable)
    for (int j = 0; j < k; ++j) {
        if (__ballot(running) == 0ull) break;
        // (in place, and the clip recomputed from `a`, which the caller keeps anyway: nothing but m and alpha lives across the step)
#pragma unroll
        for (int i = 0; i < A; ++i) m[i] = running ? rn_add(m[i], rn_mul(alpha, rn_sub(clip1(a[i]), m[i]))) : m[i];
        R nx[S], r;
        const StepOut so = Env::step(o, m, c, t * k + j + 1, nx, r);
        if (running) {
            out = so;
            sum = (j == 0) ? r : sum + r;
            cnt = t * k + j + 1;
#pragma unroll
            for (int i = 0; i < S; ++i) o[i] = nx[i];
        }
        running = running && !so.truncated;
    }
    reward = sum;
    count = cnt;
    return out;
}

// ---------------------------------------------------------------------------
// CartPole swing-up.  cartpole_env.py:48-49, 51-92, 138-182.
// ---------------------------------------------------------------------------
template <typename R> struct CartPoleEnv {
    static constexpr int S = 5, A = 1;
    static constexpr bool kBalanceTerminates = false;
    static constexpr bool kMaySubstep = true;
    static constexpr bool kMayLag = false;
    struct C {
        R mc, mp, l, g, dt;
        int max_steps, time_trunc_step;
        __host__ __device__ static inline C build(const double (&q)[12], double timestep, int max_steps, int time_trunc_step) {
            C c;
            c.mc = (R)q[0]; c.mp = (R)q[1]; c.l = (R)q[2]; c.g = (R)q[3]; c.dt = (R)timestep;
            c.max_steps = max_steps; c.time_trunc_step = time_trunc_step;
            return c;
        }
        __host__ static C make(const tg_env_params& p) { return build(p.p, p.timestep, p.max_steps, p.time_trunc_step); }
    };

    __device__ static inline StepOut step(const R (&s)[S], const float (&a)[A], const C& c, int steps_after,
                                          R (&o)[S], R& reward) {
#pragma clang fp contract(off)   // every kernel that instantiates this gets the same (unfused) arithmetic: bit-identical states
        using M = Math<R>;
        const float u32 = rn_mul(5.0f, clip1(a[0]));                       // :49
        const R u = (R)u32;                                                   // :60
        const R x = s[0], xd = s[1], sn = s[2], cs = s[3];
        const R thd = fmin(fmax(s[4], (R)-10), (R)10);                        // :58
        const R theta = M::atan2_(sn, cs);                                    // :68
        const R msum = c.mc + c.mp;
        const R alpha = (c.g * sn + cs * ((-u - c.mp * c.l * (thd * thd) * sn) / msum)) /
                        (c.l * ((R)4 / (R)3 - (c.mp * (cs * cs)) / msum));    // :71-73
        const R acc = (u + c.mp * c.l * ((thd * thd) * sn - alpha * cs)) / msum;  // :76
        const R xd_n = xd + acc * c.dt;                                       // :79
        const R x_n = x + xd_n * c.dt;                                        // :80
        const R thd_n = thd + alpha * c.dt;                                   // :82
        const R th_n = theta + thd_n * c.dt;                                  // :83
        R sn_n, cs_n;
        M::sincos_(th_n, &sn_n, &cs_n);
        o[0] = x_n; o[1] = xd_n; o[2] = sn_n; o[3] = cs_n; o[4] = thd_n;     // :85-91

        // reward on the new state; three summands (missing comma at :164-165)
        const R theta_cost = -(cs_n * cs_n * cs_n);
        const R thd_cost = thd_n * thd_n;
        const float energy32 = rn_mul(0.001f, rn_mul(u32, u32));        // float32 in the reference
        const R e1 = (R)-5 * (x_n * x_n);
        const R e2 = (R)-0.5 * (xd_n * xd_n);
        const R e3 = -((R)20 * theta_cost - (R)20) * ((R)1 / ((R)1 + (R)2 * thd_cost)) - (R)energy32;
        R r = c.dt * ((e1 + e2) + e3);                                        // :158-166
        const R ax = M::abs_(x_n);
        StepOut out;
        out.truncated = (ax > (R)1) || (steps_after >= c.time_trunc_step);    // :168
        out.balanced = (ax < (R)0.1) && (cs_n > (R)0.95) && (M::abs_(thd_n) < (R)0.1);  // :173
        if (out.balanced) r += (R)100 * c.dt;                                 // :174
        if (ax > (R)1) r -= (R)50;                                            // :179-180
        reward = r;
        return out;
    }

    __device__ static inline bool failed(const R (&o)[S], const C&) { return Math<R>::abs_(o[0]) > (R)1; }          // :168
    __device__ static inline bool time_rule(int steps_after, const C& c) { return steps_after >= c.time_trunc_step; }

    // reset: theta0 ~ U(-pi, pi); state [0, 0, sin, cos, 0].  :102-119
    __device__ static inline void reset(const uint32_t (&rnd)[4], R (&o)[S]) {
        const double th = -3.141592653589793 + 6.283185307179586 * Philox::u01d(rnd[0], rnd[1]);
        R sn, cs;
        Math<R>::sincos_((R)th, &sn, &cs);
        o[0] = 0; o[1] = 0; o[2] = sn; o[3] = cs; o[4] = 0;
    }
};

// ---------------------------------------------------------------------------
// QuadPole2D: planar quadrotor + rigid pendulum payload.  quadrotor_env.py:928, 1044-1130, 1132-1223.
// ---------------------------------------------------------------------------
template <typename R> struct QuadPole2DEnv {
    static constexpr int S = 10, A = 2;
    static constexpr bool kBalanceTerminates = false;
    static constexpr bool kMaySubstep = true;
    static constexpr bool kMayLag = true;    // (rotor thrust: the one actuator the lag models)
    struct C {
        R mq_Lp, mpLp, M, g, dt, bound, balance_radius;
        float hover32, Lq_over_I32, dt32;
        int max_steps;
        __host__ __device__ static inline C build(const double (&q)[12], double timestep, int max_steps, int) {
#pragma clang fp contract(off)
            C c;
            const double mq = q[0], mp = q[1], I = q[2], Lq = q[3], Lp = q[4], g = q[5];
            c.mq_Lp = (R)(mq * Lp); c.mpLp = (R)(mp * Lp); c.M = (R)(mq + mp); c.g = (R)g;
            c.dt = (R)timestep; c.bound = (R)q[6]; c.balance_radius = (R)q[7];
            c.hover32 = (float)((mq + mp) * g / 2);                           // :895
            c.Lq_over_I32 = (float)(Lq / I);
            c.dt32 = (float)timestep;
            c.max_steps = max_steps;
            return c;
        }
        __host__ static C make(const tg_env_params& p) { return build(p.p, p.timestep, p.max_steps, p.time_trunc_step); }
    };

    __device__ static inline StepOut step(const R (&s)[S], const float (&a)[A], const C& c, int steps_after,
                                          R (&o)[S], R& reward) {
#pragma clang fp contract(off)   // every kernel that instantiates this gets the same (unfused) arithmetic: bit-identical states
        using M = Math<R>;
        const float u1 = rn_add(c.hover32, rn_mul(c.hover32, clip1(a[0])));   // :928 (float32)
        const float u2 = rn_add(c.hover32, rn_mul(c.hover32, clip1(a[1])));
        const R x = s[0], z = s[1], vx = s[2], vz = s[3], sth = s[4], cth = s[5], thd = s[6],
                sph = s[7], cph = s[8], phd = s[9];
        const R F = (R)rn_add(u2, u1);                                     // :1085
        const float ddtheta32 = rn_mul(c.Lq_over_I32, rn_sub(u2, u1));  // :1090 (float32)
        const R ddphi = -F * (sph * cth - sth * cph) / c.mq_Lp;               // :1094
        const R phd2 = phd * phd;
        const R ddx = (-sth * F - c.mpLp * cph * ddphi + c.mpLp * sph * phd2) / c.M;             // :1098
        const R ddz = (cth * F - c.M * c.g - c.mpLp * sph * ddphi - c.mpLp * cph * phd2) / c.M;  // :1101
        const R vx_n = vx + ddx * c.dt;                                       // :1105-1108
        const R vz_n = vz + ddz * c.dt;
        const R thd_n = thd + (R)rn_mul(ddtheta32, c.dt32);
        const R phd_n = phd + ddphi * c.dt;
        const R x_n = x + vx_n * c.dt;                                        // :1111-1112
        const R z_n = z + vz_n * c.dt;
        R sth_n, cth_n, sph_n, cph_n;
        M::sincos_(M::atan2_(sth, cth) + thd * c.dt, &sth_n, &cth_n);         // :1116-1118 (OLD rate)
        M::sincos_(M::atan2_(sph, cph) + phd * c.dt, &sph_n, &cph_n);         // :1122-1124
        o[0] = x_n; o[1] = z_n; o[2] = vx_n; o[3] = vz_n; o[4] = sth_n; o[5] = cth_n; o[6] = thd_n;
        o[7] = sph_n; o[8] = cph_n; o[9] = phd_n;

        const R r2 = x_n * x_n + z_n * z_n;
        const R pos_cost = (M::abs_(x_n) + M::abs_(z_n)) + r2;                // :1186
        const R vel_cost = vx_n * vx_n + vz_n * vz_n;
        const R theta_cost = (R)1 - M::abs_(cth_n);
        const R omega_cost = thd_n * thd_n;
        const R phi_cost = cph_n * cph_n * cph_n;
        const R phid_cost = phd_n * phd_n;
        R acc = -(R)15 * pos_cost;                                            // :1195-1201
        acc = acc + (-(R)0.5 * vel_cost);
        acc = acc + (-(R)5 * theta_cost);
        acc = acc + (-(R)5 * omega_cost);
        acc = acc + (-((R)25 * phi_cost - (R)25) * ((R)1 / ((R)1 + (R)5 * phid_cost)));
        R r = c.dt * acc;
        StepOut out;
        out.balanced = (M::sqrt_(r2) < c.balance_radius) && (cph_n < (R)-0.95) && (M::abs_(phd_n) < (R)0.1);  // :1204
        if (out.balanced) r += (R)100 * c.dt;
        const bool oob = (x_n < -c.bound) || (x_n > c.bound) || (z_n < -c.bound) || (z_n > c.bound);  // :1020-1022
        if (oob) r -= (R)1000 * c.dt;                                         // :1215-1217
        out.truncated = (steps_after >= c.max_steps) || oob;                  // :1220
        reward = r;
        return out;
    }

    __device__ static inline bool failed(const R (&o)[S], const C& c) {                                              // :1020-1022
        return (o[0] < -c.bound) || (o[0] > c.bound) || (o[1] < -c.bound) || (o[1] > c.bound);
    }
    __device__ static inline bool time_rule(int steps_after, const C& c) { return steps_after >= c.max_steps; }

    // reset: phi0 ~ U(-pi, pi); quad [0,0,0,0,0,1,0], pend [sin, cos, 0].  :930-961
    __device__ static inline void reset(const uint32_t (&rnd)[4], R (&o)[S]) {
        const double ph = -3.141592653589793 + 6.283185307179586 * Philox::u01d(rnd[0], rnd[1]);
        R sn, cs;
        Math<R>::sincos_((R)ph, &sn, &cs);
        o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = 1; o[6] = 0; o[7] = sn; o[8] = cs; o[9] = 0;
    }
};

// ---------------------------------------------------------------------------
// QuadPole: 3-D quadrotor (quaternion attitude) + tethered payload (quaternion).
// quadrotor_env.py:190-228 (quaternion helpers), 409-413, 417-528, 625-713.
// ---------------------------------------------------------------------------
template <typename R> __device__ static inline void quat_mult(const R (&q)[4], const R (&r)[4], R (&o)[4]) {
#pragma clang fp contract(off)
    o[0] = q[0] * r[0] - q[1] * r[1] - q[2] * r[2] - q[3] * r[3];             // :196-201
    o[1] = q[0] * r[1] + q[1] * r[0] + q[2] * r[3] - q[3] * r[2];
    o[2] = q[0] * r[2] - q[1] * r[3] + q[2] * r[0] + q[3] * r[1];
    o[3] = q[0] * r[3] + q[1] * r[2] - q[2] * r[1] + q[3] * r[0];
}

template <typename R> struct QuadPoleEnv {
    static constexpr int S = 20, A = 4;
    static constexpr bool kBalanceTerminates = false;
    static constexpr bool kMaySubstep = true;
    static constexpr bool kMayLag = true;
    struct C {
        R m0, m_p, g, L, Ixx, Iyy, Izz, arm, dt, bound, tension_k, m0L, inv_m0, s22, mpL2;
        float hover32, tc32;
        int max_steps;
        __host__ __device__ static inline C build(const double (&q)[12], double timestep, int max_steps, int) {
#pragma clang fp contract(off)
            C c;
            const double m0 = q[0], mp = q[1], g = q[2], L = q[3];
            c.m0 = (R)m0; c.m_p = (R)mp; c.g = (R)g; c.L = (R)L;
            c.Ixx = (R)q[4]; c.Iyy = (R)q[5]; c.Izz = (R)q[6];
            c.tc32 = (float)q[7]; c.arm = (R)q[8]; c.bound = (R)q[9];
            c.dt = (R)timestep;
            c.tension_k = (R)(mp / (m0 + mp)); c.m0L = (R)(m0 * L); c.inv_m0 = (R)(1.0 / m0);
            c.s22 = (R)(1.4142135623730951 / 2.0);
            c.mpL2 = (R)(mp * (L * L));   // divisor of :511 (kept as a divisor below)
            c.hover32 = (float)((m0 + mp) * g / 4);                           // :382
            c.max_steps = max_steps;
            return c;
        }
        __host__ static C make(const tg_env_params& p) { return build(p.p, p.timestep, p.max_steps, p.time_trunc_step); }
    };

    __device__ static inline StepOut step(const R (&s)[S], const float (&a)[A], const C& c, int steps_after,
                                          R (&o)[S], R& reward) {
#pragma clang fp contract(off)   // every kernel that instantiates this gets the same (unfused) arithmetic: bit-identical states
        using M = Math<R>;
        float u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = rn_add(c.hover32, rn_mul(c.hover32, clip1(a[i])));  // :413
        const R u_tot = (R)rn_add(rn_add(rn_add(u[0], u[1]), u[2]), u[3]);                  // :445

        const R q[4] = {s[6], s[7], s[8], s[9]};
        const R om[3] = {s[10], s[11], s[12]};
        const R qp[4] = {s[13], s[14], s[15], s[16]};
        const R omp[3] = {s[17], s[18], s[19]};

        // thrust in the inertial frame = third column of R(q) * u_tot.  :210-219, 466
        const R F[3] = {((R)2 * (q[1] * q[3] + q[0] * q[2])) * u_tot,
                        ((R)2 * (q[2] * q[3] - q[0] * q[1])) * u_tot,
                        ((R)1 - (R)2 * (q[1] * q[1] + q[2] * q[2])) * u_tot};
        // tether direction: rotate [0,0,-1] by q_p.  :221-228, 470
        const R qv[4] = {0, 0, 0, -1};
        const R qpc[4] = {qp[0], -qp[1], -qp[2], -qp[3]};
        R tmp[4], rot[4];
        quat_mult(qp, qv, tmp);
        quat_mult(tmp, qpc, rot);
        const R ut[3] = {rot[1], rot[2], rot[3]};
        const R ud[3] = {omp[1] * ut[2] - omp[2] * ut[1], omp[2] * ut[0] - omp[0] * ut[2],
                         omp[0] * ut[1] - omp[1] * ut[0]};                    // :473
        const R ud2 = ud[0] * ud[0] + ud[1] * ud[1] + ud[2] * ud[2];
        R udn2 = ud2;                                                         // |u_dot|^2
        if constexpr (!M::kFast) { const R udn = M::sqrt_(ud2); udn2 = udn * udn; }   // norm()**2 as written
        const R Fdot = F[0] * ut[0] + F[1] * ut[1] + F[2] * ut[2];
        const R T = c.tension_k * (Fdot - c.m0L * udn2);                      // :476
        const R mg[3] = {0, 0, c.m0 * -c.g};
        R vel_n[3], pos_n[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const R acc = c.inv_m0 * ((mg[i] + F[i]) - T * ut[i]);            // :480
            vel_n[i] = s[3 + i] + acc * c.dt;                                 // :483
            pos_n[i] = s[i] + vel_n[i] * c.dt;                                // :484
        }
        // torques; the gyroscopic term is applied twice in the reference (kept).  :487-500
        const R d_x = (R)rn_sub(rn_sub(rn_add(u[0], u[2]), u[1]), u[3]);
        const R d_y = (R)rn_sub(rn_sub(rn_add(u[2], u[3]), u[0]), u[1]);
        const float d_z32 = rn_sub(rn_sub(rn_add(u[0], u[3]), u[1]), u[2]);
        const R tau_x = c.s22 * d_x * c.arm - (c.Izz - c.Iyy) * om[1] * om[2];
        const R tau_y = c.s22 * d_y * c.arm - (c.Izz - c.Ixx) * om[0] * om[2];
        const R tau_z = (R)rn_mul(c.tc32, d_z32);
        const R Jo[3] = {c.Ixx * om[0], c.Iyy * om[1], c.Izz * om[2]};
        const R cr[3] = {om[1] * Jo[2] - om[2] * Jo[1], om[2] * Jo[0] - om[0] * Jo[2], om[0] * Jo[1] - om[1] * Jo[0]};
        R om_n[3];
        om_n[0] = om[0] + M::div_(tau_x - cr[0], c.Ixx) * c.dt;
        om_n[1] = om[1] + M::div_(tau_y - cr[1], c.Iyy) * c.dt;
        om_n[2] = om[2] + M::div_(tau_z - cr[2], c.Izz) * c.dt;
        // q' = normalise(q + 0.5 (q (x) [0, om']) dt)   (NEW omega).  :504-506
        const R om4[4] = {0, om_n[0], om_n[1], om_n[2]};
        R qd[4], q_n[4];
        quat_mult(q, om4, qd);
        R nn = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { q_n[i] = q[i] + ((R)0.5 * qd[i]) * c.dt; nn += q_n[i] * q_n[i]; }
        if constexpr (M::kFast) {
            const R inv = M::inv_sqrt_(nn);
#pragma unroll
            for (int i = 0; i < 4; ++i) q_n[i] = q_n[i] * inv;
        } else {
            nn = M::sqrt_(nn);
#pragma unroll
            for (int i = 0; i < 4; ++i) q_n[i] = q_n[i] / nn;
        }
        // payload: omega_p' and q_p' = normalise(q_p + 0.5 ([0, omega_p'] (x) q_p) dt).  :511-517
        const R arm_v[3] = {c.L * ut[0], c.L * ut[1], c.L * ut[2]};
        const R frc[3] = {T * ut[0] + (R)0, T * ut[1] + (R)0, T * ut[2] + (-c.g * c.m_p)};
        const R ompd[3] = {M::div_(arm_v[1] * frc[2] - arm_v[2] * frc[1], c.mpL2),
                           M::div_(arm_v[2] * frc[0] - arm_v[0] * frc[2], c.mpL2),
                           M::div_(arm_v[0] * frc[1] - arm_v[1] * frc[0], c.mpL2)};
        R omp_n[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) omp_n[i] = omp[i] + ompd[i] * c.dt;
        const R omp4[4] = {0, omp_n[0], omp_n[1], omp_n[2]};
        R qpd[4], qp_n[4];
        quat_mult(omp4, qp, qpd);
        R np_ = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { qp_n[i] = qp[i] + ((R)0.5 * qpd[i]) * c.dt; np_ += qp_n[i] * qp_n[i]; }
        if constexpr (M::kFast) {
            const R inv = M::inv_sqrt_(np_);
#pragma unroll
            for (int i = 0; i < 4; ++i) qp_n[i] = qp_n[i] * inv;
        } else {
            np_ = M::sqrt_(np_);
#pragma unroll
            for (int i = 0; i < 4; ++i) qp_n[i] = qp_n[i] / np_;
        }

#pragma unroll
        for (int i = 0; i < 3; ++i) { o[i] = pos_n[i]; o[3 + i] = vel_n[i]; o[10 + i] = om_n[i]; o[17 + i] = omp_n[i]; }
#pragma unroll
        for (int i = 0; i < 4; ++i) { o[6 + i] = q_n[i]; o[13 + i] = qp_n[i]; }

        // reward on the new state.  :669-699
        const R th_q = (R)1 - M::abs_(q_n[0]);
        const R th_p = (R)1 - M::abs_(qp_n[0]);
        const R c_pos = (pos_n[0] * pos_n[0] + pos_n[1] * pos_n[1]) + pos_n[2] * pos_n[2];
        const R c_vel = (vel_n[0] * vel_n[0] + vel_n[1] * vel_n[1]) + vel_n[2] * vel_n[2];
        const R c_rate = (om_n[0] * om_n[0] + om_n[1] * om_n[1]) + om_n[2] * om_n[2];
        const R c_prate = (omp_n[0] * omp_n[0] + omp_n[1] * omp_n[1]) + omp_n[2] * omp_n[2];
        R acc = (R)1;
        acc = acc + M::div_((R)5, (R)1 + (R)10 * c_pos);
        acc = acc + M::div_((R)10, (R)1 + (R)10 * c_vel);
        acc = acc + M::div_((R)0.1, (R)1 + th_q * th_q);
        acc = acc + M::div_((R)5, (R)1 + c_rate);
        acc = acc + M::div_((R)10, (R)1 + (R)10 * (th_p * th_p));
        acc = acc + M::div_((R)1, (R)1 + (R)10 * c_prate);
        R r = c.dt * acc;
        bool oob = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) oob = oob || (pos_n[i] < -c.bound) || (pos_n[i] > c.bound);   // :614-622
        if (oob) r -= (R)10000 * c.dt;                                        // :705-706
        StepOut out;
        out.truncated = (steps_after >= c.max_steps) || oob;                  // :710
        out.balanced = false;                                                 // never updated by QuadPole.step
        reward = r;
        return out;
    }

    __device__ static inline bool failed(const R (&o)[S], const C& c) {                                              // :614-622
        bool oob = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) oob = oob || (o[i] < -c.bound) || (o[i] > c.bound);
        return oob;
    }
    __device__ static inline bool time_rule(int steps_after, const C& c) { return steps_after >= c.max_steps; }

    // reset: alpha, beta ~ U(-1,1); q_p = normalise(q_y (x) q_x); everything else 0 / identity.  :530-576
    __device__ static inline void reset(const uint32_t (&rnd)[4], R (&o)[S]) {
        const double al = -1.0 + 2.0 * Philox::u01d(rnd[0], rnd[1]);
        const double be = -1.0 + 2.0 * Philox::u01d(rnd[2], rnd[3]);
        R sa, ca, sb, cb;
        Math<R>::sincos_((R)(al / 2), &sa, &ca);
        Math<R>::sincos_((R)(be / 2), &sb, &cb);
        const R qx[4] = {ca, sa, 0, 0}, qy[4] = {cb, 0, sb, 0};
        R qp[4];
        quat_mult(qy, qx, qp);
        const R n = Math<R>::sqrt_(qp[0] * qp[0] + qp[1] * qp[1] + qp[2] * qp[2] + qp[3] * qp[3]);
#pragma unroll
        for (int i = 0; i < S; ++i) o[i] = 0;
        o[6] = 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[13 + i] = qp[i] / n;
    }
};

// ---------------------------------------------------------------------------
// Pendulum.  pendulum_env.py:45-46, 48-74, 124-158.
// ---------------------------------------------------------------------------
template <typename R> struct PendulumEnv {
    static constexpr int S = 3, A = 1;
    static constexpr bool kBalanceTerminates = true;
    static constexpr bool kMayLag = false;
    static constexpr bool kMaySubstep = false;   // (substeps_check: the balance count kept in len counts single steps)
    struct C {
        R mgl, inv_ml2, dt;
        int max_steps, time_trunc_step, term_steps, swingup;
        __host__ __device__ static inline C build(const double (&q)[12], double timestep, int max_steps, int time_trunc_step) {
#pragma clang fp contract(off)
            C c;
            const double mass = q[0], length = q[1], gravity = q[2];
            c.mgl = (R)(mass * gravity * length);                             // python-float product, :61
            c.inv_ml2 = (R)(1.0 / (mass * (length * length)));
            c.dt = (R)timestep;
            c.max_steps = max_steps; c.time_trunc_step = time_trunc_step;
            c.swingup = q[3] != 0.0; c.term_steps = (int)q[4];
            return c;
        }
        __host__ static C make(const tg_env_params& p) { return build(p.p, p.timestep, p.max_steps, p.time_trunc_step); }
    };

    __device__ static inline StepOut step(const R (&s)[S], const float (&a)[A], const C& c, int steps_after,
                                          R (&o)[S], R& reward) {
#pragma clang fp contract(off)   // every kernel that instantiates this gets the same (unfused) arithmetic: bit-identical states
        using M = Math<R>;
        const float a32 = clip1(a[0]);                                        // :46 (float32, no scaling)
        const R u = (R)a32;                                                   // promoted by the float64 scalar at :61
        const R thd = fmin(fmax(s[2], (R)-10), (R)10);                        // :57
        const R theta = M::atan2_(s[0], s[1]);                                // :59
        R sn, cs;
        M::sincos_(theta, &sn, &cs);
        const R alpha = c.inv_ml2 * (u - c.mgl * sn);                         // :61
        const R thd_n = thd + alpha * c.dt;                                   // :63
        const R th_n = theta + thd_n * c.dt;                                  // :64
        R sn_n, cs_n;
        M::sincos_(th_n, &sn_n, &cs_n);
        o[0] = sn_n; o[1] = cs_n; o[2] = thd_n;                               // :68-72
        StepOut out;
        out.balanced = cs_n <= (R)-0.99;                                      // :135
        out.truncated = steps_after >= c.time_trunc_step;                     // :150, float-accumulated time
        const float energy32 = rn_mul(-0.001f, rn_mul(a32, a32));           // float32 in the reference, :145
        const R e1 = (R)-10 * M::sqrt_(M::abs_((R)-1 - cs_n));                // :143 (x ** 0.5)
        const R e2 = (R)-0.1 * (thd_n * thd_n);                               // :144
        R r = c.dt * ((e1 + e2) + (R)energy32);                               // :142
        if (out.balanced) r += (R)1;                                          // :148-149 (time_balanced > 0 <=> balanced now)
        reward = r;
        return out;
    }

    // never fails; the balance rule (a real terminal) is neither clause
    __device__ static inline bool failed(const R (&)[S], const C&) { return false; }
    __device__ static inline bool time_rule(int steps_after, const C& c) { return steps_after >= c.time_trunc_step; }

    // reset: theta0 ~ U(pi - 0.05, pi + 0.05), or U(-pi, pi) with swingup; state [sin, cos, 0].  :86-106
    __device__ static inline void reset(const uint32_t (&rnd)[4], R (&o)[S]) { reset(rnd, o, 0); }
    __device__ static inline void reset(const uint32_t (&rnd)[4], R (&o)[S], int swingup) {
        const double u = Philox::u01d(rnd[0], rnd[1]);
        const double th = swingup ? -3.141592653589793 + 6.283185307179586 * u : (3.141592653589793 - 0.05) + 0.1 * u;
        R sn, cs;
        Math<R>::sincos_((R)th, &sn, &cs);
        o[0] = sn; o[1] = cs; o[2] = 0;
    }
};

// ---------------------------------------------------------------------------
// host dispatch shared by the translation units that launch one lane per env slot (env_kernels.hip, vec_env.hip)
// ---------------------------------------------------------------------------
static inline dim3 env_grid(int64_t n, int& block) {
    // small launches are latency-bound: one wave per workgroup spreads them over all CUs
    block = (n <= (int64_t)1 << 18) ? 64 : 256;
    return dim3((unsigned)ceil_div(n, block));
}

// (a Pendulum through a `_sub` entry never gets here: substeps_check refuses it, and Pendulum's kMaySubstep = false instantiates nothing)
#define TG_ENV_SWITCH(env_id, dtype, CALL)                                                     \
    switch ((env_id) * 2 + (dtype)) {                                                          \
        case TG_ENV_CARTPOLE * 2 + TG_F32: return CALL(CartPoleEnv, float);                    \
        case TG_ENV_CARTPOLE * 2 + TG_F64: return CALL(CartPoleEnv, double);                   \
        case TG_ENV_QUADPOLE2D * 2 + TG_F32: return CALL(QuadPole2DEnv, float);                \
        case TG_ENV_QUADPOLE2D * 2 + TG_F64: return CALL(QuadPole2DEnv, double);               \
        case TG_ENV_QUADPOLE * 2 + TG_F32: return CALL(QuadPoleEnv, float);                    \
        case TG_ENV_QUADPOLE * 2 + TG_F64: return CALL(QuadPoleEnv, double);                   \
        case TG_ENV_PENDULUM * 2 + TG_F32: return CALL(PendulumEnv, float);                    \
        case TG_ENV_PENDULUM * 2 + TG_F64: return CALL(PendulumEnv, double);                   \
        default: return set_error(TG_ERR_UNSUPPORTED, "unsupported env_id %d / dtype %d", (int)(env_id), (int)(dtype)); \
    }

}  // namespace tg

#include "lag_occupancy.hpp"
