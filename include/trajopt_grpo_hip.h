/*
 * trajopt_grpo_hip.h -- C ABI of the MI355X (gfx950) rollout / returns / loss kernels.
 *
 * The reference (Dyllon-Preston/trajopt-grpo @ 2025-06-13) is pure Python and has no
 * FFI of its own; its drop-in seam is the duck-typed Python surface of SURVEY.md 8(b).
 * This library is what that surface's GPU implementation binds (ctypes, see
 * INTEGRATION.md): each entry point names the reference code whose arithmetic it
 * replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (hipMalloc / torch CUDA storage);
 *   - `stream` is a hipStream_t passed as void*; all calls only ENQUEUE work on it
 *     (no allocation, no synchronisation: they are hipGraph-capturable);
 *   - return value: 0 = ok, negative = error (TG_ERR_*); tg_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI;
 *   - struct-of-arrays layouts, env index fastest:
 *       state      [S][ld]            component-major, ld >= n
 *       trajectory obs [S][T+1][n], act [A][T][n], rew [T][n], mask [T][n] (u8),
 *       len [n] (i32).  Slot t of obs is the observation BEFORE action t
 *       (rollout/rollout_worker.py:53); slot t+1 is written only while the
 *       episode is still running, so padding stays zero (rollout_worker.py:37-41).
 *   - flat env index n = g*E + e  (buffers/rollout_buffer.py:85-89).
 */
#ifndef TRAJOPT_GRPO_HIP_H
#define TRAJOPT_GRPO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TG_ABI_VERSION 13

enum { TG_OK = 0, TG_ERR_ARG = -1, TG_ERR_HIP = -2, TG_ERR_UNSUPPORTED = -3 };

/* hidden activation of the fp32 policy kernels' `_act` entry points (tg_fused_rollout_f32_act, tg_mlp_f32_forward_act,
 * tg_mlp_f32_forward_backward_act); every hidden layer of a net uses the same one */
#define TG_ACT_RELU 0
#define TG_ACT_TANH 1

/* environments (environments/cartpole_env.py, environments/quadrotor_env.py) */
enum { TG_ENV_CARTPOLE = 0, TG_ENV_QUADPOLE2D = 1, TG_ENV_QUADPOLE = 2, TG_ENV_QUADROTOR12 = 3, TG_ENV_PENDULUM = 4 };
/* arithmetic type of the environment state / trajectory */
enum { TG_F32 = 0, TG_F64 = 1 };

/* Physical parameters.  p[] meaning per env (defaults = the reference constructors):
 *  CARTPOLE   (cartpole_env.py:7-16):  p0 masscart, p1 masspole, p2 length, p3 gravity
 *  QUADPOLE2D (quadrotor_env.py:875-895): p0 mq, p1 mp, p2 I, p3 Lq, p4 Lp, p5 gravity,
 *                                         p6 bound (|x|,|z| <= p6), p7 balance_radius
 *  QUADPOLE   (quadrotor_env.py:362-382): p0 mass, p1 load_mass, p2 gravity, p3 tether,
 *                                         p4 Ixx, p5 Iyy, p6 Izz, p7 torque_constant, p8 arm,
 *                                         p9 bound
 *  QUADROTOR12(quadrotor_env.py:9-16):   p0 mass, p1 arm_length, p2 Ixx, p3 Iyy, p4 Izz,
 *                                         p5 torque_constant, p6 gravity
 *  PENDULUM   (pendulum_env.py:8-16):    p0 mass, p1 length, p2 gravity, p3 swingup (0 / 1); p4 is filled by
 *                                         tg_env_finalize_params: the number of CONSECUTIVE balanced steps after which
 *                                         the float-accumulated `_time_balanced` first exceeds 5 s (:135, :151).
 *                                         Pendulum is the one env whose episodes TERMINATE (balanced for > 5 s); in a
 *                                         rollout the running count lives in d_len as a negative number.
 * agents: rollout kernels only.  With agents = k > 1, every k consecutive env slots form ONE environment of k
 *  bodies that share the policy and terminate together: when any body truncates, all k stop at that step
 *  (segmented wavefront ballot).  The reference's QuadrotorSwarm is an empty subclass (quadrotor_env.py:185-186),
 *  so this semantics is defined by this build and has no oracle beyond k = 1 == the plain env.
 * time_trunc_step: CartPole and Pendulum -- first step count at which the reference's
 *  float-accumulated `_time > max_time` fires (cartpole_env.py:168, pendulum_env.py:150); filled by
 *  tg_env_default_params / tg_env_finalize_params. */
typedef struct tg_env_params {
    int32_t env_id;
    int32_t max_steps;
    int32_t time_trunc_step;
    int32_t agents;          /* swarm: agents per env (power of two <= 64), 0/1 = single-body env */
    double  timestep;
    double  p[12];
} tg_env_params;

/* GPU-resident trajectory of one rollout (this rank's shard). */
typedef struct tg_traj {
    void*     d_obs;      /* real [S][T+1][n] */
    float*    d_act;      /* f32  [A][T][n]   (policies emit float32: actor_critic.py:138) */
    void*     d_rew;      /* real [T][n] */
    uint8_t*  d_mask;     /* u8   [T][n] */
    int32_t*  d_len;      /* i32  [n]; <= 0 while the episode is running (0; Pendulum: -balanced steps), else its length */
    uint64_t* d_counters; /* u64  [4]: [0] env-steps executed (= sum of mask), [1] episodes ended */
    int64_t   n;
    int32_t   horizon;    /* T = env.max_steps */
    int32_t   dtype;      /* TG_F32 | TG_F64 */
} tg_traj;

const char* tg_last_error(void);
int  tg_abi_version(void);
/* Process-wide switch of the depth-specialised bf16 chain kernel: tg_mlp_backward_chain_ex with the first-layer gradient inside
 * (d_x non-NULL), panel order, H = 256 and 5 hidden layers runs an instantiation with the depth as a compile-time constant -- the same
 * arithmetic and memory operations, bit-identical results, fewer instructions.  on = 0: every launch takes the run-time-depth kernel.
 * Default 1.  Returns the previous value. */
int  tg_chain_depth_kernels(int on);
/* Process-wide switch of the block-structured bf16 forward chain: tg_mlp_forward_chain_loss_ex with the plain head, panel order and
 * H = 256 (any depth it takes) runs an instantiation whose first and top H x H layer are peeled off the layer loop and whose ring
 * slots, wait counts and per-layer pointers are no per-block run-time work -- the same arithmetic and memory operations,
 * bit-identical results, fewer instructions.  on = 0: every launch takes the run-time kernel.  Default 1.  Returns the previous value.
 * Independent of tg_chain_depth_kernels. */
int  tg_chain_fwd_kernels(int on);

int  tg_env_dims(int env_id, int* obs_dim, int* act_dim);
int  tg_env_default_params(int env_id, int max_steps, tg_env_params* out);
/* recompute derived fields (time_trunc_step) after the caller edited max_steps/timestep */
int  tg_env_finalize_params(tg_env_params* p);

/* reset(): draw initial states with the reference's distributions
 * (cartpole_env.py:102-119, quadrotor_env.py:530-576, :930-961) from a counter-based
 * Philox4x32-10 stream keyed by (seed, stream_id, (key_offset + i) / key_div): with
 * key_div = E all E episodes of a group share one draw (the `restart=True` semantics of
 * rollout_worker.py:70-71); key_offset = this shard's first global env index, so results
 * do not depend on how envs are sharded over GPUs.  Writes d_state[S][ld], columns 0..n-1. */
int  tg_env_reset(const tg_env_params* p, int dtype, void* d_state, int64_t ld, int64_t n,
                  uint64_t seed, uint64_t stream_id, int64_t key_offset, int64_t key_div,
                  void* stream);

/* step(): one Env.step for n independent envs on SoA state (may be in place:
 * d_next == d_state).  cartpole_env.py:138-182, quadrotor_env.py:625-713, :1132-1223.
 * d_action f32 [A][ld_a]; d_steps i32 [n] in/out (count before -> after);
 * d_time_balanced real [n] in/out or NULL; d_reward real [n]; d_truncated u8 [n]. */
int  tg_env_step(const tg_env_params* p, int dtype, const void* d_state, int64_t ld,
                 const float* d_action, int64_t ld_a, void* d_next, int64_t ld_next,
                 int32_t* d_steps, void* d_time_balanced, void* d_reward,
                 uint8_t* d_truncated, int64_t n, void* stream);

/* Quadrotor._dynamics (quadrotor_env.py:113-169): pure explicit-Euler map, raw control
 * real [4][ld_c]; state real [12][ld]. */
int  tg_quadrotor12_dynamics(const tg_env_params* p, int dtype, const void* d_state, int64_t ld,
                             const void* d_control, int64_t ld_c, void* d_next, int64_t ld_next,
                             int64_t n, void* stream);

/* ---- GPU-resident rollout (replaces RolloutManager.rollout / RolloutWorker.run_episodes,
 *      rollout/rollout_manager.py:85-125, rollout/rollout_worker.py:19-84) ---- */

/* zero the trajectory + counters (padding must be zero: rollout_worker.py:37-41).  Clears ALL of obs, slot 0
 * included: write the initial states (tg_env_reset into slot 0, or a copy) after this call. */
int  tg_rollout_begin(const tg_traj* tr, int obs_dim, int act_dim, void* stream);

/* fused time step t for all n envs:
 *   action source: d_mean != NULL  -> a = mean[i][:] + sigma * eps, eps ~ N(0,I) from
 *                                     Philox keyed (seed, stream_id, env_offset + i, t)
 *                                     (MultivariateNormal(mean, diag(sigma^2)).sample(),
 *                                     actor_critic.py:131-133); action recorded in act[:,t,i];
 *                  d_mean == NULL  -> teacher forcing: act[:,t,i] is read (parity runs);
 *   then Env.step, reward/mask/len recording and episode termination.  A wavefront whose 64
 *   envs have all ended (ballot == 0) exits before touching memory; env-steps are counted
 *   with one atomic per wavefront (popcount of the ballot).
 * d_rng: device u64[2] = {seed, stream_id} (read by the kernel so a captured graph can be
 * replayed with a fresh stream id).  sigma: host float[A] = sqrt(diag(cov)). */
int  tg_rollout_step(const tg_env_params* p, const tg_traj* tr, int32_t t, const float* d_mean,
                     int64_t mean_row_stride, const float* sigma, const uint64_t* d_rng,
                     int64_t env_offset, void* stream);

/* Teacher-forced steps [t_begin, t_end) in ONE launch: tg_rollout_step(d_mean = NULL) for every t of the range, the state kept in
 * registers between steps (a wavefront owns 64 envs for the whole range) -- per env-step the recorded action is read and the next
 * observation, reward and mask byte are written, nothing else.  Bit-identical to the per-step launches. */
int  tg_rollout_forced(const tg_env_params* p, const tg_traj* tr, int32_t t_begin, int32_t t_end, void* stream);

/* Time-limit bootstrapping, first half: the state each episode's LAST step produced (the rollout drops it: slot len of obs holds
 * the padding's zeros) and whether the clock, not a failure, ended the episode.  For env slot i with L = len[i] in [1, T]:
 *   d_s_final f32 [n][S], row i = Env.step(obs[:, L-1, i], act[:, L-1, i]) with step count L -- the step function of tg_env_step,
 *                                 bit for bit (an f64 trajectory's state is rounded to f32 once, on the store);
 *   d_timeout u8  [n],    [i]   = !failed(s_final) && (time_rule(L) || L == T): `failed` is the env's own failure test (CartPole
 *                                 |x| > 1; QuadPole2D / QuadPole out of bounds; Pendulum: never), `time_rule` its own clock test
 *                                 (step count >= time_trunc_step resp. max_steps).  A Pendulum episode ended by the balance rule
 *                                 is neither: a terminal.
 * A slot whose len is outside [1, T] gets zeros and 0.  Reads d_obs, d_act, d_len of the trajectory only; writes nothing into it.
 * Swarm envs (p->agents > 1) are refused with TG_ERR_UNSUPPORTED. */
int  tg_rollout_final_state(const tg_env_params* p, const tg_traj* tr, float* d_s_final, uint8_t* d_timeout, void* stream);

/* counters[0] = sum of episode lengths (= env-steps executed = sum of mask),
 * counters[1] = episodes ended.  rollout/rollout_worker.py:67-68.  A slot with len <= 0 has not ended (Pendulum keeps minus its
 * balanced-step count there while an episode runs): it counts as 0 steps and no episode, the rule of tg_rollout_finish_stats. */
int  tg_rollout_finish(const tg_traj* tr, void* stream);

/* tg_rollout_finish + tg_rng_advance (d_rng may be NULL) + the statistics Rollout_Buffer.sample() reads
 * (buffers/rollout_buffer.py:70: the average episode return), in two launches: d_stats f64 [3] = {sum of all rewards (fixed
 * summation order: deterministic), n, sum of episode lengths}.  d_work: tg_rollout_finish_stats_workspace() bytes. */
int  tg_rollout_finish_stats_workspace(void);
int  tg_rollout_finish_stats(const tg_traj* tr, uint64_t* d_rng, double* d_stats, double* d_work, void* stream);

/* The whole step range [t_begin, t_end) of a rollout in ONE persistent launch: actor MLP on the matrix cores
 * (bf16 weights, fp32 accumulate), sampling, Env.step, recording and termination, with the env state held in
 * registers.  Same results contract as tg_rollout_step in sampling mode (same Philox keys); the means differ
 * from the GEMM path only by bf16/fp32 summation order.  The actor must be Linear(S,H) ReLU [Linear(H,H) ReLU]*
 * Linear(H,A) with H in {128, 256}, S <= 32, A <= 4.
 *   d_wfrag: bf16 weights in MFMA A-fragment order (see mlp.fragment_stream): blocks of H/16 KiB --
 *            first layer (all output tiles), then one block per 32-row output tile of every H x H layer, then the
 *            head padded to 32 rows;  d_bias: f32 [(n_hidden_layers + 1)][H] (head row padded with zeros). */
int  tg_fused_rollout(const tg_env_params* p, const tg_traj* tr, const void* d_wfrag, const float* d_bias,
                      int32_t hidden, int32_t n_hidden_layers, const float* sigma, const uint64_t* d_rng,
                      int64_t env_offset, int32_t t_begin, int32_t t_end, void* stream);

/* The same for float32 policies (the reference's own precision; rollout/rollout_worker.py:19-84): every product in
 * fp32 on the matrix cores (v_mfma_f32_32x32x2_f32), one workgroup per 32 envs, the weights register-resident for the
 * whole rollout -- built for latency at the reference's net sizes and a few thousand envs.  The means differ from the
 * GEMM path only by fp32 summation order.  Actor: Linear(S,H) ReLU [Linear(H,H) ReLU]^(n_hidden_layers-1) Linear(H,A),
 * H in {64, 128}, 1..4 hidden layers, S <= 32, A <= 4 (tg_fused_rollout_f32_supported()).
 *   block_envs: 32, or 16 -- the same rollout with sixteen envs per workgroup on v_mfma_f32_16x16x4_f32, for env counts that leave
 *              CUs without a workgroup at 32 (BASELINE configs[1]: 4,096 envs = 128 workgroups on 256 CUs): a time step is a chain
 *              of dependent products on the workgroup's one CU, so half the envs are half the step's latency.
 *              tg_fused_rollout_f32_block_envs(n, agents) says which one the launch should use; it decides the layout of d_wstream.
 *   d_wstream: f32 [H/32 waves][K1/2 + (n_hidden_layers-1)*H/2 registers][64 lanes], K1 = S rounded up to 8, first layer then
 *              the H x H layers (zero beyond the matrix; trajopt-grpo_amd/mlp.py `RegisterStreamF32`):
 *              block_envs 32: register 4q + j of lane (m, kh) of wave w is W[32w + m][8q + 4kh + j];
 *              block_envs 16: register tt * (k / 4) + s of lane (i, g) of wave w is W[32w + 16 tt + i][first layer: 4 s + g;
 *                             H x H: 16 (s >> 2) + 4 g + (s & 3)]   (k = the layer's padded input width, tt = 0, 1);
 *   d_tab:     f32 [(n_hidden_layers)*H hidden biases][4*H head weights, rows >= A zero][4 head biases]. */
int  tg_fused_rollout_f32_supported(int32_t hidden, int32_t n_hidden_layers);
int  tg_fused_rollout_f32_block_envs(int64_t n, int32_t agents);
int  tg_fused_rollout_f32(const tg_env_params* p, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                          int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                          int64_t env_offset, int32_t t_begin, int32_t t_end, void* stream);
/* The same rollout with the hidden activation as an argument: TG_ACT_RELU launches exactly what tg_fused_rollout_f32 launches,
 * TG_ACT_TANH the same kernels with a = tanhf(z) (the device library's, |error| <= 4 * 2^-24) in place of max(z, 0).
 * An unknown activation is refused. */
int  tg_fused_rollout_f32_act(const tg_env_params* p, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                              int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                              int64_t env_offset, int32_t t_begin, int32_t t_end, int32_t activation, void* stream);

/* d_rng[1] += 1 (enqueued; one thread) */
int  tg_rng_advance(uint64_t* d_rng, void* stream);

/* ---- Per-env domain randomisation of the physical parameters ----
 * Env slot i of a rollout steps its OWN vehicle: the reference env constructed with slot i's parameters, every derived constant
 * (hover thrust, Lq / I, mp / (m0 + mp), ...) following them.  The parameters live in a device table
 *   d_ptab f64 [12][n]   (env fastest): column i = the p[] of tg_env_params for slot i
 * which tg_env_randomize fills and the `_dr` entry points read next to `p` (`p` still supplies env_id, max_steps,
 * time_trunc_step, agents and timestep, and the nominal p[] the table scales).
 *
 * tg_env_randomize, one launch: row r of the table = p->p[r], times -- when r == index[k] for some k < count -- the factor
 *   f_k(i) = lo[k] + (hi[k] - lo[k]) * u01d(w[2 (k & 1)], w[2 (k & 1) + 1])                      (IEEE double, no contraction)
 *   w      = Philox4x32-10(key = seed ^ (spec->seed * 0x9E3779B97F4A7C15), counter = ((key_offset + i) / key_div, 0xFFFFFFFE - k / 2, stream_id))
 *   u01d(a, b) = ((a << 32 | b) >> 11) * 2^-53
 * with the seed, stream_id, key_offset and key_div of the rollout's tg_env_reset: parameters are re-drawn with every rollout, do not
 * depend on how envs are sharded over ranks, and the episodes of a `restart` group (key_div = E) share one vehicle as they share one
 * initial state.  The counter's third word ("sub") counts down from 0xFFFFFFFE, two parameters per draw: the reset uses 0xFFFFFFFF
 * and time step t uses t, so no draw is shared.  Refused (TG_ERR_ARG, nothing launched): a null table, count outside [0, 12], an
 * index outside [0, 12) or listed twice, a factor range that is not finite with 0 < lo <= hi. */
typedef struct tg_randomize_spec {
    int32_t  count;        /* randomised parameters, <= 12 */
    int32_t  index[12];    /* which p[] each of them scales */
    double   lo[12];       /* factor range of each: finite, 0 < lo <= hi */
    double   hi[12];
    uint64_t seed;         /* combined with the rollout seed (above) */
} tg_randomize_spec;
int  tg_env_randomize(const tg_env_params* p, const tg_randomize_spec* spec, double* d_ptab, int64_t n, uint64_t seed,
                      uint64_t stream_id, int64_t key_offset, int64_t key_div, void* stream);

/* The rollout entry points with the table: the same arguments plus d_ptab (f64 [12][tr->n], not NULL), the same kernels except that
 * the lane that owns env slot i builds its constants from column i at kernel entry (the fused and teacher-forced kernels keep them
 * for all their steps) instead of taking one set by value.  A table whose every column is p->p gives the plain entry point's
 * trajectory bit for bit. */
int  tg_rollout_step_dr(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, int32_t t, const float* d_mean,
                        int64_t mean_row_stride, const float* sigma, const uint64_t* d_rng, int64_t env_offset, void* stream);
int  tg_rollout_forced_dr(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, int32_t t_begin, int32_t t_end, void* stream);
int  tg_rollout_final_state_dr(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, float* d_s_final, uint8_t* d_timeout,
                               void* stream);
int  tg_fused_rollout_dr(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const void* d_wfrag, const float* d_bias,
                         int32_t hidden, int32_t n_hidden_layers, const float* sigma, const uint64_t* d_rng, int64_t env_offset,
                         int32_t t_begin, int32_t t_end, void* stream);
int  tg_fused_rollout_f32_dr(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                             int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                             int64_t env_offset, int32_t t_begin, int32_t t_end, void* stream);
int  tg_fused_rollout_f32_act_dr(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                                 int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                                 int64_t env_offset, int32_t t_begin, int32_t t_end, int32_t activation, void* stream);

/* ---- returns / advantages (algorithms/grpo.py:66-74,110-115; algorithms/ppo.py:93-139) ---- */

/* reward-to-go reverse scan, fp32, bit-for-bit the reference recurrence:
 *   R[T-1] = r[T-1] m[T-1];  R[t] = r[t] m[t] + (gamma R[t+1]) m[t+1]      [T][n] layout */
int  tg_rtg_scan(const float* d_rew, const uint8_t* d_mask, float gamma, float* d_rtg,
                 int64_t n, int32_t T, void* stream);

/* GAE branch (ppo.py:112-124): adv and ret = values + adv.
 * The coefficient of A[t+1] is rn_mul(gamma, lam) of the two floats passed in.  The reference's `gamma * lam * adv` rounds the
 * DOUBLE product once to fp32: the same number for most pairs (every shipped one), one ulp apart for e.g. (0.995, 0.97) --
 * 0.96515006 here against 0.96515.  Where the two agree the scan is the reference's bit for bit. */
int  tg_gae_scan(const float* d_rew, const float* d_values, const uint8_t* d_mask, float gamma,
                 float lam, float* d_adv, float* d_ret, int64_t n, int32_t T, void* stream);

/* masked moments per group of `group_size` consecutive envs (all T steps):
 * d_moments f64 [n/group_size][3] = {count, sum, sum of squares}; deterministic
 * (no float atomics).  d_work: f64 [3*n] scratch. */
int  tg_masked_moments(const float* d_x, const uint8_t* d_mask, int64_t n, int32_t T,
                       int64_t group_size, double* d_moments, double* d_work, void* stream);

/* mode 0 (GRPO, grpo.py:115): out = (x - mean_g) / std_g          (unbiased std, eps inside std)
 * mode 1 (PPO,  ppo.py:138-139): out = (x - mean_g) / (std_g + 1e-8)
 * masked-out entries are written as 0. */
int  tg_group_normalize(const float* d_x, const uint8_t* d_mask, const double* d_moments,
                        int mode, float* d_out, int64_t n, int32_t T, int64_t group_size,
                        void* stream);

/* ---- policy log-prob + fused clipped-surrogate loss (forward + backward) ----
 * Gaussian policy with fixed diagonal covariance (actor_critic.py:100-103,159-160):
 *   logp = -1/2 sum_k (a_k - mu_k)^2 / var_k - k/2 ln 2pi - 1/2 sum_k ln var_k
 * rows are samples; mean is row-major [M][A] (row stride given); act element (i,k) is at
 * d_act[i*act_row_stride + k*act_col_stride]. */
int  tg_gaussian_logp(const float* d_mean, int64_t mean_row_stride, const float* d_act,
                      int64_t act_row_stride, int64_t act_col_stride, const float* var,
                      int act_dim, float* d_logp, int64_t M, void* stream);

typedef struct tg_loss_args {
    const float*   d_mean;  int64_t mean_row_stride;            /* [M][A] policy means */
    const float*   d_act;   int64_t act_row_stride, act_col_stride;
    const float*   d_logp_old;                                  /* [M] */
    const float*   d_adv;                                       /* [M] */
    const float*   d_value;                                     /* [M] or NULL (GRPO) */
    const float*   d_ret;                                       /* [M] or NULL (GRPO) */
    const uint8_t* d_mask;                                      /* [M] or NULL = all rows valid */
    const float*   d_norm;   /* NULL, or device f32[4] {adv_mean, adv_inv_std, ret_mean, ret_inv_std}
                                applied on the fly: x <- (x - mean) * inv_std   (ppo.py:138-139) */
    float   var[8];          /* diag(cov) */
    int32_t act_dim;
    float   epsilon;         /* clip range */
    float   surr_coef;       /* d(total)/d(sum_i min(rho A, clip(rho) A)):
                                GRPO +1/G (descent on J as written, grpo.py:137-145);
                                PPO  -1/n_valid (ppo.py:165) */
    float   critic_coef;     /* PPO: c1/n_valid  (ppo.py:169,179); 0 for GRPO */
    float   kl_coef;         /* PPO: kl_coeff/n_valid  (ppo.py:175-176); 0 for GRPO */
    float*  d_grad_mean;     /* [M][A] row-major (row stride A): d total / d mean */
    float*  d_grad_value;    /* [M] or NULL */
    double* d_sums;          /* f64[4]: sum surrogate, sum (V-R)^2, sum exp(lp_old)(lp_old-lp), #valid */
    double* d_work;          /* f64[4*tg_loss_work_blocks()] scratch */
    int64_t M;
    const float* d_coef;     /* NULL, or device f32[3] {surr_coef, critic_coef, kl_coef}: used INSTEAD of the three host fields
                                (tg_ppo_norm's output + 4: PPO's 1 / n_valid stays on the device) */
} tg_loss_args;

int  tg_loss_work_blocks(void);
int  tg_surrogate_loss(const tg_loss_args* a, void* stream);

/* ---- MLP backward glue (models/neural_network.py:67-77 under torch autograd in the reference) ----
 * dZ = dA * (A > 0) in place (A = post-ReLU activations) fused with the bias-gradient column sums:
 * d_partial f32 [tg_relu_bwd_bias_blocks()][cols]; the caller sums it over axis 0.
 * Row-major [rows][cols]; bf16 needs cols % 8 == 0, f32 cols % 4 == 0; cols <= tg_relu_bwd_bias_max_cols(is_bf16)
 * (one workgroup of 256 threads x 16 bytes holds a row: 2048 in bf16, 1024 in f32). */
int  tg_relu_bwd_bias_blocks(void);
int  tg_relu_bwd_bias_max_cols(int32_t is_bf16);
int  tg_relu_bwd_bias(void* d_dA, const void* d_A, int64_t rows, int32_t cols, int32_t is_bf16,
                      float* d_partial, void* stream);

/* The head's backward-data product fused into the top hidden layer's ReLU backward:
 *   dZ[r][c] = (sum_{k<act_dim} dout[r][k] * Whead[k][c]) * (A[r][c] > 0),  d_partial as tg_relu_bwd_bias.
 * d_dout f32 [rows][act_dim] (contiguous), d_whead f32 [act_dim][cols] (the head's master weights),
 * d_act / d_dz [rows][cols] bf16 (is_bf16) or f32; cols % 8 == 0, cols <= tg_head_bwd_relu_bias_max_cols() (2048, both dtypes).
 * d_maskbits (optional, bf16, cols 128 / 256): the layer's ReLU mask bits from tg_mlp_forward_chain (cols / 8 bytes
 * per row) are read instead of d_act (which may then be NULL): 4 B instead of 16 B per thread. */
int  tg_head_bwd_relu_bias_max_cols(void);
int  tg_head_bwd_relu_bias(const float* d_dout, int32_t act_dim, const float* d_whead, const void* d_act,
                           const void* d_maskbits, void* d_dz, int64_t rows, int32_t cols, int32_t is_bf16,
                           float* d_partial, void* stream);

/* Bias gradients: out[v][c] += sum_{b<n_blocks} partial[b][v][c] for n_vec <= 8 gradient vectors of `width` entries in
 * one launch (d_partial = the per-workgroup column sums tg_mlp_backward_chain / tg_dx_relu_bias / tg_relu_bwd_bias /
 * tg_head_prep leave; d_out = HOST array of n_vec device pointers).  Fixed summation order. */
int  tg_colsum_finish(const float* d_partial, int32_t n_blocks, int32_t n_vec, int32_t width, float* const* d_out,
                      void* stream);

/* Head of the backward pass: d_dz[r][k] = dout[r][k] (k < act_dim; compute dtype bf16 / f32), zero for the padding
 * columns up to out_pad (8 or 16), and d_partial f32 [tg_head_prep_blocks()][act_dim] = per-workgroup column sums of
 * dout (the head's bias gradient, finished by tg_colsum_finish with width act_dim). */
int  tg_head_prep_blocks(void);
int  tg_head_prep(const float* d_dout, int64_t rows, int32_t act_dim, int32_t out_pad, int32_t is_bf16, void* d_dz,
                  float* d_partial, void* stream);

/* Weight-gradient epilogue (replaces the reduction, tail GEMM and additions PyTorch would run after a split-K batched
 * GEMM dz^T a; torch autograd's accumulation into Linear.weight.grad):
 *   grad[m][k] += sum_{b<n_batches} partial[b][m][k] + sum_{r<tail} dz_tail[r][m] * a_tail[r][k],  m < m_out, k < k_out
 * d_partial f32 [n_batches][m_dim][k_dim]; d_dz_tail [tail][m_dim], d_a_tail [tail][k_dim] (bf16 if is_bf16 else f32;
 * may be NULL when tail == 0); d_grad f32 with row stride grad_ld.  Fixed summation order: deterministic. */
int  tg_dw_finish(const float* d_partial, int32_t n_batches, int32_t m_dim, int32_t k_dim, const void* d_dz_tail,
                  const void* d_a_tail, int32_t tail, int32_t is_bf16, float* d_grad, int64_t grad_ld, int32_t m_out,
                  int32_t k_out, void* stream);

/* A hidden layer's backward-data product on the matrix cores, fused with the ReLU backward and the bias gradient
 * of the layer below (bf16 operands, fp32 accumulate; replaces `dA = dZ @ W` + tg_relu_bwd_bias):
 *   dZ_below[r][m] = (sum_{k<k_dim} dZ[r][k] * W[k][m]) * (A[r][m] > 0)
 *   d_partial f32 [tg_dx_relu_bias_blocks()][m_dim]: per-workgroup column sums of dZ_below (caller sums axis 0).
 * d_dz_in bf16 [rows][k_dim], d_act / d_dz_out bf16 [rows][m_dim] (row-major, contiguous, distinct buffers),
 * W = Linear.weight bf16 [k_dim = out_features][m_dim = in_features].  d_wfrag is W re-ordered by
 * tg_dx_pack_weights (k_dim*m_dim bf16, MFMA A-fragment order; rebuild it whenever W changes).
 * tg_dx_relu_bias_supported(k_dim, m_dim) != 0 for the shapes that have a kernel (square 64 / 128 / 256).
 * d_maskbits (optional, widths 128 / 256): the ReLU mask bits of A written by tg_mlp_forward_chain (m_dim / 8 bytes per
 * row) are read instead of d_act (which may then be NULL): 1.03 instead of 1.5 KB of traffic per row at 256. */
int  tg_dx_relu_bias_supported(int32_t k_dim, int32_t m_dim);
int  tg_dx_relu_bias_blocks(void);
int  tg_dx_pack_weights(const void* d_w, void* d_wfrag, int32_t k_dim, int32_t m_dim, void* stream);
int  tg_dx_relu_bias(const void* d_dz_in, const void* d_wfrag, const void* d_act, const void* d_maskbits, void* d_dz_out,
                     int64_t rows, int32_t k_dim, int32_t m_dim, float* d_partial, void* stream);

/* ---- MLP forward, all layers in one persistent launch (models/neural_network.py:67-77) ----
 * Linear(in<=32, H) ReLU [Linear(H, H) ReLU]^(n_hidden_layers-1) Linear(H, out<=out_cols), H in {128, 256}, bf16
 * operands, fp32 accumulate / bias / head output.  A row's activations stay on chip between layers and are only
 * written (for the backward pass):
 *   d_x      bf16 [rows][32]   input, features >= in zero-padded
 *   d_wfrag  bf16 weight stream in MFMA fragment order (trajopt-grpo_amd/mlp.py `FragmentStream(layout="chain")`
 *            documents and builds it), d_bias f32 [n_hidden_layers + 1][H] (natural order, head row zero-padded)
 *   d_acts   HOST array of n_hidden_layers device pointers, bf16 [rows][H] each (post-ReLU outputs of the hidden
 *            layers, row-major), or NULL to skip storing them.  d_acts[0] alone may be NULL: the first activation is
 *            then left out (tg_mlp_weight_grad kind HR recomputes it; its mask bits are still written)
 *   d_masks  HOST array of n_hidden_layers device pointers, u32 [rows][H / 32] each, or NULL: the ReLU masks of the
 *            stored activations, 1 bit each (all the backward-data kernels need of them).  Per row: [lane half h = 0, 1]
 *            [H / 64 words]; feature 32 mt + 16 h + r is bit (mt & 1) * 8 + (r >> 1) + 16 * (r & 1) of word mt >> 1
 *   d_out    f32 [rows][out_cols], out_cols in {4, 8, 16} (columns >= out hold the padded head rows: zeros + bias 0; 4 for nets
 *            with <= 4 outputs: a 16-B row, so that tg_rollout_step reads no padding with the policy mean) */
int  tg_mlp_forward_chain(const void* d_x, const void* d_wfrag, const float* d_bias, int32_t hidden,
                          int32_t n_hidden_layers, int64_t rows, void* const* d_acts, void* const* d_masks,
                          float* d_out, int32_t out_cols, void* stream);
/* Layout of the learner's INTERNAL [rows][H] bf16 tensors -- the stored activations and the dZ, whose one reader is
 * tg_mlp_weight_grad.  TG_LAYOUT_ROWS: row-major (what every entry point without a layout argument writes and reads).
 * TG_LAYOUT_PANEL: "panel order", the weight-gradient kernel's own LDS panel image per 32-row tile: the 16-byte chunk c (features
 * 8 c .. 8 c + 7) of row r sits at byte
 *     (r / 32) * 64 H  +  (r % 32 / 4) * (H / 32 * 256)  +  (c / 4) * 256  +  (r % 4) * 64  +  (c % 4) * 16
 * Rows stay time-major; a buffer holds ceil(rows / 32) WHOLE tiles (64 H bytes each) and the producers fill the pad rows of the
 * last tile with copies of the last row (finite; the consumer multiplies them by zeros).  The `_ex` entry points of the three
 * producers take the layout they write; tg_dw_job.layout says which operands of a job are stored so.  Same values, same sums:
 * only addresses differ. */
enum { TG_LAYOUT_ROWS = 0, TG_LAYOUT_PANEL = 1 };
/* tg_mlp_forward_chain with the layout of d_acts as an argument (TG_LAYOUT_PANEL: d_acts non-NULL, n_hidden_layers >= 2) */
int  tg_mlp_forward_chain_ex(const void* d_x, const void* d_wfrag, const float* d_bias, int32_t hidden,
                             int32_t n_hidden_layers, int64_t rows, void* const* d_acts, void* const* d_masks,
                             float* d_out, int32_t out_cols, int32_t layout, void* stream);

/* The training forward pass with the LOSS HEAD and the head's weight gradient inside it.  The clipped-surrogate / squared-error
 * gradient of a row (what tg_surrogate_loss + tg_head_prep produce: algorithms/ppo.py:159-179, grpo.py:122-140) is a function of the
 * head output the kernel holds and of per-row inputs, so d loss / d output is written directly (bf16 [rows][8], the backward
 * chain's input) and contracted on chip with the top hidden activation: that activation is NOT written (d_acts[n - 1] may be
 * NULL, as d_acts[0]) and tg_mlp_weight_grad needs no DH job.
 *   kind 0 (actor): d_act (contiguous [rows][act_dim]), d_logp_old, d_adv, var[act_dim], epsilon, surr_coef, kl_coef
 *   kind 1 (critic): d_ret, critic_coef              act_dim <= 4
 *   norm_mean / norm_inv: the advantage (actor) / return (critic) enters as (x - norm_mean) * norm_inv (0 and 1: as is)
 *   d_head_slabs  f32 [tg_mlp_forward_chain_blocks()][4][16][H] partial head weight gradients (rows 0..act_dim-1 of each [16][H]);
 *                 d_bias_partial f32 [blocks][4]; d_work f64 [blocks][4] partial sums (surrogate, squared error, KL, count):
 *                 the caller adds the first `grid` = min(blocks, ceil(rows / 256)) of each in order. */
typedef struct tg_chain_loss {
    int32_t      kind, act_dim;
    const float* d_act; int64_t act_row_stride, act_col_stride;
    const float* d_logp_old; const float* d_adv; const float* d_ret;
    float        norm_mean, norm_inv;
    float        var[4];
    float        epsilon, surr_coef, critic_coef, kl_coef;
    void*        d_dout8; float* d_head_slabs; double* d_work; float* d_bias_partial;
    /* kind 0 (tg_mlp_forward_chain_loss, tg_mlp_f32_forward_backward; NULL otherwise): the old policy IS the current one (ppo.py:142-143 always; GRPO when
     * nothing has touched either net since `old_policy.load_state_dict(policy.state_dict())`, grpo.py:148): the row's log-probability
     * is written here and used as its own old log-probability (ratio exactly 1, as in the reference, whose two forward passes are
     * the same arithmetic) -- d_logp_old is not read, and the caller needs no no-grad pass of the old policy. */
    float*       d_logp_old_out;
    /* NULL, or device f32[8] as tg_ppo_norm writes it {adv mean, adv 1/(std+eps), ret mean, ret 1/(std+eps), surr_coef, critic_coef,
     * kl_coef, n}: the head then takes its normalisation pair (kind 0: [0], [1]; kind 1: [2], [3]) and its coefficients ([4], [5], [6])
     * from there instead of from norm_mean / norm_inv / *_coef above -- PPO's batch statistics (ppo.py:138-139) and 1 / n_valid
     * (:165-179) never visit the host. */
    const float* d_norm8;
} tg_chain_loss;
int  tg_mlp_forward_chain_blocks(void);
int  tg_mlp_forward_chain_loss(const void* d_x, const void* d_wfrag, const float* d_bias, int32_t hidden, int32_t n_hidden_layers,
                               int64_t rows, void* const* d_acts, void* const* d_masks, const tg_chain_loss* loss, void* stream);

/* ---- GRPO's KL penalty to a frozen reference policy (DeepSeekMath GRPO; grpo.py:127-134) ----
 * The `_ref` variants of the five training heads (tg_surrogate_loss, tg_mlp_forward_chain_loss, tg_mlp_f32_forward_backward,
 * tg_mlp_f32w_forward_backward, tg_mlp_f32r_forward_backward) take the same arguments plus `ref`.  Per valid actor row, with
 * lp = the row's log-probability under the current policy and x = d_logp_ref[row] - lp:
 *   D = exp(x) - x - 1             added to the KL sum (slot 2 of the f64 [4] sums / d_work)
 *   d loss / d lp += coef (exp(x) - 1)
 * i.e. loss = surr_coef * sum min(rho A, clip(rho) A) - coef * sum D, and GRPO passes coef = surr_coef * beta.
 * ref == NULL or coef == 0: the plain entry point's kernel, bit for bit.  Refused: a penalty on a critic (tg_chain_loss.kind != 0,
 * tg_loss_args.d_value != NULL), a NULL d_logp_ref with a nonzero coef, and a nonzero host kl_coef beside it (slot 2 is the
 * penalty's; a device d_norm8 / d_coef kl_coef must be 0 too). */
typedef struct tg_ref_penalty {
    const float* d_logp_ref;  /* [rows] f32: log pi_ref(a | s) of the same rows the head reads (row-indexed as d_logp_old) */
    float        coef;        /* d loss / d (sum D) = -coef */
    int32_t      reserved;    /* 0 */
} tg_ref_penalty;
int  tg_surrogate_loss_ref(const tg_loss_args* a, const tg_ref_penalty* ref, void* stream);
int  tg_mlp_forward_chain_loss_ref(const void* d_x, const void* d_wfrag, const float* d_bias, int32_t hidden, int32_t n_hidden_layers,
                                   int64_t rows, void* const* d_acts, void* const* d_masks, const tg_chain_loss* loss,
                                   const tg_ref_penalty* ref, void* stream);

/* ---- A learned, state-independent log-std of the Gaussian policy (one parameter per action dimension) ----
 * The `_std` variants of the training heads take the same arguments plus a nullable `ref` (GRPO's penalty above) and `std`.  The
 * head then reads log_std[k], k < act_dim, from DEVICE memory at kernel entry -- inv_var[k] = exp(-2 log_std[k]), logp_const =
 * -act_dim / 2 log(2 pi) - sum log_std; tg_loss_args.var / tg_chain_loss.var are not read -- and writes, per valid actor row,
 *   d_out[row][k] = (d loss / d logp) * ((act_k - mean_k)^2 inv_var[k] - 1)      k < act_dim; columns >= act_dim zero
 * the row's contribution to d loss / d log_std[k] (d loss / d logp as the head forms it: surrogate, kl_coef term, reference
 * penalty).  Rows the head skips (tg_loss_args.d_mask) get zeros.  tg_log_std_grad sums the rows of d_out in f64 in a fixed order
 * (no float atomics) and ADDS the sums, plus `add` to every component, into d_grad f32 [act_dim]: the log_std window of the
 * gradient bucket, once per chunk (`add` = -entropy coefficient on one chunk of one rank, 0 elsewhere).  d_work: f64
 * [tg_log_std_grad_blocks()][4] scratch.
 * std == NULL: what the `_ref` entry point launches.  Refused: act_dim > 4, a critic head, a NULL field of `std`. */
typedef struct tg_learned_std {
    const float* d_log_std;   /* [act_dim] f32, read on the device at kernel entry */
    float*       d_out;       /* [rows][4] f32 */
} tg_learned_std;
int  tg_surrogate_loss_std(const tg_loss_args* a, const tg_ref_penalty* ref, const tg_learned_std* std, void* stream);
int  tg_mlp_forward_chain_loss_std(const void* d_x, const void* d_wfrag, const float* d_bias, int32_t hidden, int32_t n_hidden_layers,
                                   int64_t rows, void* const* d_acts, void* const* d_masks, const tg_chain_loss* loss,
                                   const tg_ref_penalty* ref, const tg_learned_std* std, void* stream);
/* tg_mlp_forward_chain_loss_std (ref, std nullable) with the layout of d_acts as an argument; TG_LAYOUT_PANEL is built for the plain
 * head (ref == NULL or coef 0, std == NULL) and refused otherwise. */
int  tg_mlp_forward_chain_loss_ex(const void* d_x, const void* d_wfrag, const float* d_bias, int32_t hidden, int32_t n_hidden_layers,
                                  int64_t rows, void* const* d_acts, void* const* d_masks, const tg_chain_loss* loss,
                                  const tg_ref_penalty* ref, const tg_learned_std* std, int32_t layout, void* stream);
int  tg_log_std_grad_blocks(void);
int  tg_log_std_grad(const float* d_rows4, int64_t rows, int32_t act_dim, float add, float* d_grad, double* d_work, void* stream);
/* (the fp32 chain learners' `_std` entry points are declared beside their plain ones below) */

/* ---- How far the updates of a learn() moved the policy, and the learning rate that follows (rsl_rl's schedule="adaptive") ----
 * tg_policy_shift, one chunk of rows: lp = the Gaussian log-probability of the row's action under d_mean (float32, the row
 * arithmetic of tg_gaussian_logp; strides as there), with either `var` (HOST float [act_dim], act_dim <= 8) or `d_log_std` (DEVICE
 * float [act_dim], act_dim <= 4, read at kernel entry as the `_std` heads read it: no host read of a learned std) -- exactly one of
 * the two is non-NULL.  Per row, in float64: d = lp - logp_old (exact), k3 = expm1(d) - d (>= 0: an estimate of KL(old || new)),
 * clipped = d < log_lo || d > log_hi (the caller forms log_lo = log1p(-epsilon), log_hi = log1p(epsilon) in double).
 * Workgroup b of the launch covers rows [4096 b, 4096 (b + 1)) (at most 1024 workgroups, grid-stride beyond) and leaves ONE partial
 *   d_partials[slot + b][4] = {rows, sum k3, clipped rows, sum d}
 * added in a fixed order (shuffle tree, then the four waves in wave order; no floating-point atomics): which rows a thread adds
 * depends on `rows` alone.  tg_policy_shift_blocks(rows) partials are written (0 for rows == 0: nothing is launched); the caller
 * gives each chunk its own `slot`.
 * tg_policy_shift_finish (one workgroup): d_sums[4] = the n_partials partials added in index order (zeros for n_partials == 0).
 * tg_lr_adapt (one thread, float64): d_out4 = {kl, clip_fraction, lr_in, lr_out} from the (all-reduced) sums,
 *   kl = sums[1] / sums[0], clip_fraction = sums[2] / sums[0], lr_in = lr, and with rows = sums[0]
 *   lr_out = fmax(lr / factor, lr_min)   if desired_kl > 0 && rows > 0 && kl > 2 desired_kl
 *            fmin(lr * factor, lr_max)   if desired_kl > 0 && rows > 0 && kl < desired_kl / 2
 *            lr                          otherwise (a NaN kl included: every comparison is false; desired_kl <= 0: measure only). */
int  tg_policy_shift_blocks(int64_t rows);
int  tg_policy_shift(const float* d_mean, int64_t mean_row_stride, const float* d_act, int64_t act_row_stride, int64_t act_col_stride,
                     const float* d_logp_old, const float* var, const float* d_log_std, int act_dim, double log_lo, double log_hi,
                     int64_t rows, double* d_partials, int64_t slot, void* stream);
int  tg_policy_shift_finish(const double* d_partials, int32_t n_partials, double* d_sums, void* stream);
int  tg_lr_adapt(const double* d_sums, double desired_kl, double factor, double lr_min, double lr_max, double lr, double* d_out4,
                 void* stream);
/* tg_kl_control (one thread, float64): a check BETWEEN the optimizer steps of a learn() acts on a device control block
 *   d_ctl f64 [8] = {stopped, lr, stop_update, kl_at_stop, last_kl, last_clip_fraction, checks, 0}
 * which the `_ctl` optimizer launches read (tg_adam_step_ctl).  The caller initialises it to {0, lr, 0, 0, nan, nan, 0, 0}.  In order:
 *   1. d_ctl[0] != 0 (latched): the block is left as it is, byte for byte;
 *   2. kl and clip_fraction as tg_lr_adapt forms them, into slots 4 and 5; slot 6 += 1;
 *   3. desired_kl > 0: tg_lr_adapt's rule on d_ctl[1] (the check that latches applies it too);
 *   4. target_kl > 0 && rows > 0 && kl > stop_factor * target_kl (strict): d_ctl[0] = 1, d_ctl[2] = update, d_ctl[3] = kl.
 * update: the 1-based count of optimizer steps applied so far.  A NaN kl or rows == 0 neither adapts nor stops. */
int  tg_kl_control(const double* d_sums, double target_kl, double stop_factor, double desired_kl, double factor, double lr_min,
                   double lr_max, int64_t update, double* d_ctl, void* stream);

/* ---- MLP backward-data pass, all hidden layers in one persistent launch ----
 * For Linear(in, H) ReLU [Linear(H, H) ReLU]^(n_hidden_layers-1) Linear(H, out <= 8), H in {128, 256}, 3..6 hidden
 * layers, bf16:
 *   dZ_top   = (dOut . W_head)  * (a_top   > 0)
 *   dZ_below = (dZ   . W_layer) * (a_below > 0)           for every hidden-to-hidden layer, from the top down
 * a row's gradient stays on chip from the head to the first hidden layer; read 16 B + H/8 B of mask bits per layer,
 * write 2 H B per layer (H = 256, 5 layers: 2.7 instead of 4.8 KB per row).
 *   d_dout8   bf16 [rows][8]: d loss / d head output, columns >= out zero
 *   d_wfrag   bf16 stream of the TRANSPOSED weights, head first then the hidden-to-hidden layers top down
 *             (trajopt-grpo_amd/mlp.py `FragmentStream(layout="chain", transposed=True)`)
 *   d_dz      HOST array of n_hidden_layers device pointers, bf16 [rows][H]: outputs, TOP hidden layer first.  d_dz[0] may
 *             be NULL (only with d_partial == NULL): the top layer's dZ is then not written -- it is a function of d_dout8
 *             and the layer's mask bits, and tg_mlp_weight_grad (kind RH) rebuilds it on chip
 *   d_masks   HOST array of the same layers' ReLU mask bits (u32 [rows][H/32], as tg_mlp_forward_chain writes them)
 *   d_partial f32 [tg_mlp_backward_chain_blocks()][n_hidden_layers][H]: per-workgroup column sums of the dZ (bias
 *             gradients; the caller sums axis 0).  Deterministic.  NULL: no column sums (tg_mlp_weight_grad forms the
 *             bias gradients inside its contraction; the kernel is ~10 % shorter without them). */
int  tg_mlp_backward_chain_blocks(void);
int  tg_mlp_backward_chain(const void* d_dout8, const void* d_wfrag, int32_t hidden, int32_t n_hidden_layers, int64_t rows,
                           void* const* d_dz, const void* const* d_masks, float* d_partial, void* stream);
/* The same pass with the FIRST layer's weight gradient formed inside it: dW0 = dZ_bottom^T . x contracts over the rows the kernel
 * already holds, so the bottom layer's dZ is not written (d_dz[n_hidden_layers - 1] may be NULL) and tg_mlp_weight_grad needs no
 * HX job.  d_x = the net input, bf16 [rows][32], zero padded -- with column 31 set to ONE if the caller wants the first layer's
 * bias gradient as column 31 of the result.  d_w0_slabs: f32 [*n_slabs][H][32] partial gradients (2 per workgroup; buffer of at
 * least 2 * tg_mlp_backward_chain_blocks() * H * 32 floats = slab_floats); the caller adds the *n_slabs slabs in order.
 * Replaces: the bottom Linear's weight.grad / bias.grad of `loss.backward()` (algorithms/ppo.py:181-183). */
int  tg_mlp_backward_chain_w0(const void* d_dout8, const void* d_wfrag, int32_t hidden, int32_t n_hidden_layers, int64_t rows,
                              void* const* d_dz, const void* const* d_masks, const void* d_x, float* d_w0_slabs, int64_t slab_floats,
                              int32_t* n_slabs, void* stream);

/* Either of the two with the layout of d_dz as an argument: d_x == NULL (d_w0_slabs, slab_floats, n_slabs ignored):
 * tg_mlp_backward_chain without column sums; otherwise tg_mlp_backward_chain_w0. */
int  tg_mlp_backward_chain_ex(const void* d_dout8, const void* d_wfrag, int32_t hidden, int32_t n_hidden_layers, int64_t rows,
                              void* const* d_dz, const void* const* d_masks, const void* d_x, float* d_w0_slabs, int64_t slab_floats,
                              int32_t* n_slabs, int32_t layout, void* stream);

/* ---- MLP weight gradients, every layer in one persistent launch (what `loss.backward()` leaves in Linear.weight.grad /
 *      .bias.grad: algorithms/ppo.py:181-183, algorithms/grpo.py:143-145) ----
 *   wgrad[m][n] += sum over rows r of P[r][m] * Q[r][n]   (m < m_out, n < n_out)      bgrad[m] += sum over rows of P[r][m]
 * one job per Linear; P = the layer's dZ (tg_mlp_backward_chain), Q = the layer's input.  bf16 operands, fp32 sums, every
 * operand byte read once.  A workgroup keeps one job's whole H x H fp32 gradient in registers for its share of the rows and
 * leaves it as a partial ("slab") in the workspace; a second kernel adds the slabs in a fixed order into the gradient
 * windows (e.g. the learner's flat all-reduce bucket): deterministic.
 *   kind HH: P bf16 [rows][H], Q bf16 [rows][H]          hidden-to-hidden layers
 *        HX: P bf16 [rows][H], Q bf16 [rows][32]         first layer (Q = the zero-padded net input)
 *        DH: P bf16 [rows][8], Q bf16 [rows][H]          head (P = d loss / d head output, zero padded; no bias sums:
 *                                                        tg_head_prep produces them)
 *        HR: P bf16 [rows][H], Q bf16 [rows][32]         second layer WITHOUT its stored input: the first hidden
 *                                                        activation relu(W0 x + b0) is recomputed on chip from the net
 *                                                        input row (d_w0frag = first block of the forward chain's weight
 *                                                        stream, d_b0 = first-layer bias f32 [H]); bit-identical to
 *                                                        what tg_mlp_forward_chain would have stored
 *        RH: P bf16 [rows][8],  Q bf16 [rows][H]         top hidden-to-hidden layer WITHOUT its stored dZ: dZ_top =
 *                                                        (dOut . W_head) * (a_top > 0) is recomputed on chip from P = d loss /
 *                                                        d head output (as DH's P), d_aux = the top hidden layer's ReLU mask
 *                                                        bits (u32 [rows][H/32], tg_mlp_forward_chain) and d_whfrag = the first
 *                                                        block of the backward chain's weight stream (W_head^T);
 *                                                        bit-identical to what tg_mlp_backward_chain would have stored
 * H in {128, 256}.  d_workspace: tg_mlp_weight_grad_workspace(H) bytes. */
enum { TG_DW_HH = 0, TG_DW_HX = 1, TG_DW_DH = 2, TG_DW_HR = 3, TG_DW_RH = 4 };
typedef struct tg_dw_job {
    const void* d_p;
    const void* d_q;
    float*      d_wgrad;      /* f32, row stride wgrad_ld */
    float*      d_bgrad;      /* f32 [m_out] or NULL */
    int64_t     wgrad_ld;
    int32_t     kind;
    int32_t     m_out, n_out;
    int32_t     layout;       /* (in what used to be padding: 0 = both row-major) bit 0: P, bit 1: Q is a [rows][H] operand in panel
                               * order (TG_LAYOUT_PANEL; never the [rows][8] / [rows][32] operands of DH / RH / HX / HR) */
    const void* d_aux;        /* RH: the top hidden layer's ReLU mask bits; otherwise unused */
} tg_dw_job;
int64_t tg_mlp_weight_grad_workspace(int32_t hidden);
/* tg_mlp_weight_grad_ex: the same launch pair, with up to 4 more fixed-order slab reductions riding on the second launch -- the
 * chain kernels' OWN partial gradients (tg_mlp_forward_chain_loss's head slabs and bias partials, tg_mlp_backward_chain_w0's
 * first-layer slabs), which the learner otherwise adds with three torch launches each:
 *   d_grad[m * grad_ld + n] += sum over s < n_slabs of d_slab[s * slab_stride + m * row_pitch + n],  m < m_out, n < n_out
 * -- and, optionally, the forward chain's per-workgroup f64 loss sums: d_loss_sums[k] += sum over r < n_loss_rows of
 * d_loss_work[r * 4 + k] (k < 4), rows in order.  Everything deterministic, no atomics. */
typedef struct tg_slab_sum {
    const float* d_slab; int64_t slab_stride; int32_t n_slabs; int32_t row_pitch;
    float* d_grad; int64_t grad_ld; int32_t m_out, n_out;
} tg_slab_sum;
int  tg_mlp_weight_grad_ex(int32_t hidden, const tg_dw_job* jobs, int32_t n_jobs, int64_t rows, const void* d_w0frag, const float* d_b0,
                           const void* d_whfrag, void* d_workspace, int64_t workspace_bytes, const tg_slab_sum* extra, int32_t n_extra,
                           const double* d_loss_work, int32_t n_loss_rows, double* d_loss_sums, void* stream);
int  tg_mlp_weight_grad(int32_t hidden, const tg_dw_job* jobs, int32_t n_jobs, int64_t rows, const void* d_w0frag,
                        const float* d_b0, const void* d_whfrag, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- The update in the reference's own precision (fp32) at the reference's own net sizes ----
 * Linear(S <= 32, H) ReLU [Linear(H, H) ReLU]{0..3} Linear(H, A <= 4), H in {64, 128}: pipelines/cartpole_pipeline_grpo.py:54-76,
 * cartpole_pipeline_ppo.py:54-79 (models/neural_network.py:67-77); every product is v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains).
 *   d_x       f32 [rows][in_pad], in_pad in {8, 16, 24, 32}, columns >= S zero
 *   d_stream  f32, tg_mlp_f32_stream_floats(H, n_hidden_layers, in_pad) floats (trajopt-grpo_amd/mlp.py `F32ChainStream` documents
 *             and builds it): [first layer in MFMA fragment order: H x in_pad][hidden biases: n x H][head weights: 4 x H, rows >= A
 *             zero][head bias: 4][forward blocks of the H x H layers][backward (transposed) blocks, top layer first]
 * tg_mlp_f32_forward: the no-grad pass (models/neural_network.py:67-77): d_out f32 [rows][4] (columns >= A: zeros + bias 0).
 * tg_mlp_f32_forward_backward: forward pass + loss head + backward-DATA pass of every row in ONE launch (algorithms/ppo.py:159-183,
 *   grpo.py:122-145 up to the weight gradients): `loss` as for tg_mlp_forward_chain_loss, except that d_dout8 receives d loss /
 *   d head output as F32 [rows][4], d_head_slabs / d_bias_partial are not used (the head's gradient is a job of
 *   tg_mlp_f32_weight_grad) and d_work is f64 [tg_mlp_f32_blocks()][4]; the caller adds the first min(blocks, ceil(rows / 256)).
 *   d_acts / d_dz: HOST arrays of n_hidden_layers device pointers, f32 [rows][H] each: the post-ReLU outputs of the hidden layers
 *   and d loss / d their pre-activations (index = layer, 0 = first hidden layer), written for tg_mlp_f32_weight_grad.  With >= 2
 *   hidden layers d_acts[0] and (given d_top_maskbits: u32 [rows][4], the top layer's ReLU mask, 1 bit per feature) d_dz[n - 1]
 *   may be NULL: the weight-gradient job that would read them rebuilds them on chip (tg_f32_dw_job.recompute).  Mask layout:
 *   feature 32 mt + 8 q + 4 hh + low (q < 4, hh < 2, low < 4) is bit low + 4 q + 16 (mt % 2) of word hh * (H / 64) + mt / 2.
 * tg_mlp_f32_weight_grad: every job's wgrad += P^T Q (and bgrad += column sums of P) in one launch + one fixed-order reduction
 *   (deterministic, no float atomics).  kind MM: P f32 [rows][H] (a layer's dZ), Q f32 [rows][n_cols] (its input: n_cols = H, or
 *   the padded net input, n_cols = in_pad), window m_out = H x n_out <= n_cols; kind HEAD: P = d loss / d head output f32
 *   [rows][4], Q = the top activation f32 [rows][H], window m_out = A x n_out = H, bgrad [A]. */
int64_t tg_mlp_f32_stream_floats(int32_t hidden, int32_t n_hidden_layers, int32_t in_pad);
int  tg_mlp_f32_blocks(void);
int  tg_mlp_f32_forward(const float* d_x, int32_t in_pad, const float* d_stream, int32_t hidden, int32_t n_hidden_layers,
                        int64_t rows, float* d_out, void* stream);
int  tg_mlp_f32_forward_backward(const float* d_x, int32_t in_pad, const float* d_stream, int32_t hidden, int32_t n_hidden_layers,
                                 int64_t rows, void* const* d_acts, void* const* d_dz, void* d_top_maskbits,
                                 const tg_chain_loss* loss, void* stream);
int  tg_mlp_f32_forward_backward_ref(const float* d_x, int32_t in_pad, const float* d_stream, int32_t hidden, int32_t n_hidden_layers,
                                     int64_t rows, void* const* d_acts, void* const* d_dz, void* d_top_maskbits,
                                     const tg_chain_loss* loss, const tg_ref_penalty* ref, void* stream);   /* (tg_ref_penalty above) */
/* The two passes with the hidden activation as an argument (and, for the training pass, a nullable `ref`: NULL = the plain head,
 * else GRPO's reference penalty as in the `_ref` entry).  TG_ACT_RELU launches exactly what tg_mlp_f32_forward /
 * tg_mlp_f32_forward_backward[_ref] launch.  TG_ACT_TANH: a = tanhf(z) (the device library's, |error| <= 4 * 2^-24) and
 * dZ = dA * (1 - a^2) from the stored fp32 a (torch's tanh_backward); a mask bit cannot stand for 1 - a^2, so nothing is rebuilt:
 * every d_acts[i] and d_dz[i] must be given and d_top_maskbits must be NULL (the weight-gradient jobs are plain MM / HEAD jobs).
 * Refused before any launch: an unknown activation, Tanh with a mask buffer or a NULL d_acts[i] / d_dz[i], and everything the
 * plain entries refuse. */
int  tg_mlp_f32_forward_act(const float* d_x, int32_t in_pad, const float* d_stream, int32_t hidden, int32_t n_hidden_layers,
                            int64_t rows, float* d_out, int32_t activation, void* stream);
int  tg_mlp_f32_forward_backward_act(const float* d_x, int32_t in_pad, const float* d_stream, int32_t hidden, int32_t n_hidden_layers,
                                     int64_t rows, void* const* d_acts, void* const* d_dz, void* d_top_maskbits,
                                     const tg_chain_loss* loss, const tg_ref_penalty* ref, int32_t activation, void* stream);
int  tg_mlp_f32_forward_backward_act_std(const float* d_x, int32_t in_pad, const float* d_stream, int32_t hidden, int32_t n_hidden_layers,
                                         int64_t rows, void* const* d_acts, void* const* d_dz, void* d_top_maskbits,
                                         const tg_chain_loss* loss, const tg_ref_penalty* ref, const tg_learned_std* std,
                                         int32_t activation, void* stream);   /* (tg_learned_std above) */
/* The same passes at H = 256 (the reference's QuadPole factory at its own precision: pipelines/quadpole_pipeline_ppo.py:54-58,
 * 20-256x5-{4,1} fp32), csrc/mlp_f32_wide.hip: a wave owns 16 rows on v_mfma_f32_16x16x4_f32, two 4-wave workgroups per CU.
 *   d_stream  f32, tg_mlp_f32w_stream_floats(n_hidden_layers) floats, in 16-KiB blocks of 16 pieces x 64 lanes x 16 B, lane = (i = lane & 15,
 *             g = lane >> 4) (trajopt-grpo_amd/mlp.py `F32WideStream`):
 *               first layer, 2 blocks: block b, piece 2 tt + q (tt < 8, q < 2): W0[16 (8 b + tt) + i][8 g + 4 q .. + 3] (zero beyond the inputs)
 *               forward, layer l = 1 .. n_hidden_layers - 1, 16 blocks mo, piece t:  W_l[16 mo + i][16 t + 4 g .. + 3]
 *               backward, layer l = n_hidden_layers - 1 .. 1, 16 blocks ko, piece t: {W_l[16 t + 4 g + r][16 ko + i], r = 0..3}
 *   d_table   f32 [tg_mlp_f32w_table_floats()]: [5][256] hidden biases | [4][256] head weights (rows >= outputs zero) | [4] head bias
 *   d_acts / d_dz as for tg_mlp_f32_forward_backward (d_acts[0] and d_dz[top] may be NULL). */
int64_t tg_mlp_f32w_stream_floats(int32_t n_hidden_layers);
int64_t tg_mlp_f32w_table_floats(void);
int  tg_mlp_f32w_blocks(void);
int  tg_mlp_f32w_forward(const float* d_x, int32_t in_pad, const float* d_stream, const float* d_table, int32_t n_hidden_layers, int64_t rows,
                         float* d_out, void* stream);
int  tg_mlp_f32w_forward_backward(const float* d_x, int32_t in_pad, const float* d_stream, const float* d_table, int32_t n_hidden_layers,
                                  int64_t rows, void* const* d_acts, void* const* d_dz, const tg_chain_loss* loss, void* stream);
int  tg_mlp_f32w_forward_backward_ref(const float* d_x, int32_t in_pad, const float* d_stream, const float* d_table, int32_t n_hidden_layers,
                                      int64_t rows, void* const* d_acts, void* const* d_dz, const tg_chain_loss* loss,
                                      const tg_ref_penalty* ref, void* stream);
int  tg_mlp_f32w_forward_backward_std(const float* d_x, int32_t in_pad, const float* d_stream, const float* d_table, int32_t n_hidden_layers,
                                      int64_t rows, void* const* d_acts, void* const* d_dz, const tg_chain_loss* loss,
                                      const tg_ref_penalty* ref, const tg_learned_std* std, void* stream);
/* The H = 128 net with at most ONE H x H layer (BASELINE configs[1], C2: 5-128-128-1, pipelines/cartpole_pipeline_grpo.py:54-76) on the
 * same 16-row machine with its whole weight stream resident in LDS (csrc/mlp_f32_wide.hip, mlp_f32_res_kernel): 12 waves per CU (16 without gradients), no
 * barrier in the row loop, rows dealt 16 at a time wave-major across the CUs (C2's ~176,000 rows are 10.78 wave-rounds per SIMD: 11
 * here, 6 x 32-row rounds = 12 in tg_mlp_f32_forward_backward).  Same outputs as tg_mlp_f32_forward[_backward] (incl. the top layer's
 * mask bits): interchangeable in front of tg_mlp_f32_weight_grad.
 *   d_stream f32 [tg_mlp_f32r_stream_floats]: forward blocks [8 mo][8 pieces t][64 lanes] x 16 B: W_1[16 mo + i][16 t + 4 g .. + 3], then
 *            backward blocks [8 ko][8 t][64]: {W_1[16 t + 4 g + r][16 ko + i]}   (lane = (i = lane & 15, g = lane >> 4); empty with one hidden layer)
 *   d_w0     f32 [tg_mlp_f32r_w0_floats]: [8 tiles mo][in_pad / 4 steps s][64 lanes]: W0[16 mo + i][4 s + g] (zero beyond the inputs)
 *   d_table  f32 [tg_mlp_f32r_table_floats]: [2][128] hidden biases | [4][128] head weights | [4] head bias | 12 zeros */
int  tg_mlp_f32r_supported(int32_t hidden, int32_t n_hidden_layers, int32_t in_pad);
int64_t tg_mlp_f32r_stream_floats(int32_t hidden, int32_t n_hidden_layers);
int64_t tg_mlp_f32r_w0_floats(int32_t hidden, int32_t in_pad);
int64_t tg_mlp_f32r_table_floats(int32_t hidden);
int  tg_mlp_f32r_grid(int64_t rows);          /* workgroups of a training launch over `rows` rows = rows of f64 [4] partial sums it leaves in d_work */
int  tg_mlp_f32r_forward(const float* d_x, int32_t in_pad, const float* d_stream, const float* d_w0, const float* d_table, int32_t hidden,
                         int32_t n_hidden_layers, int32_t out_dim, int64_t rows, float* d_out /* [rows][4], columns >= out_dim zero */, void* stream);
int  tg_mlp_f32r_forward_backward(const float* d_x, int32_t in_pad, const float* d_stream, const float* d_w0, const float* d_table, int32_t hidden,
                                  int32_t n_hidden_layers, int64_t rows, void* const* d_acts, void* const* d_dz, void* d_top_maskbits,
                                  const tg_chain_loss* loss, void* stream);
int  tg_mlp_f32r_forward_backward_ref(const float* d_x, int32_t in_pad, const float* d_stream, const float* d_w0, const float* d_table,
                                      int32_t hidden, int32_t n_hidden_layers, int64_t rows, void* const* d_acts, void* const* d_dz,
                                      void* d_top_maskbits, const tg_chain_loss* loss, const tg_ref_penalty* ref, void* stream);
int  tg_mlp_f32r_forward_backward_std(const float* d_x, int32_t in_pad, const float* d_stream, const float* d_w0, const float* d_table,
                                      int32_t hidden, int32_t n_hidden_layers, int64_t rows, void* const* d_acts, void* const* d_dz,
                                      void* d_top_maskbits, const tg_chain_loss* loss, const tg_ref_penalty* ref, const tg_learned_std* std,
                                      void* stream);
enum { TG_F32DW_MM = 0, TG_F32DW_HEAD = 1 };
typedef struct tg_f32_dw_job {
    const float* d_p;
    const float* d_q;
    float*       d_wgrad;     /* f32, row stride wgrad_ld */
    float*       d_bgrad;     /* f32 [m_out] or NULL */
    int64_t      wgrad_ld;
    int32_t      kind, n_cols, m_out, n_out;
    /* wide MM job with operands REBUILT on chip instead of read, and the net's two light gradients riding on it (nets with >= 2
     * hidden layers; tg_mlp_f32_forward_backward then need not store the rebuilt matrices, and no MM job for the first layer /
     * HEAD job is given):
     *   bit 0 (the second layer's job): Q = relu(W0 x + b0), d_q = the net input f32 [rows][in_pad]; rider: the FIRST layer's
     *     gradient -- d_dz0 = the bottom dZ f32 [rows][H], d_w0grad f32 H x in_dim (row stride w0grad_ld) += dZ_0^T x, d_b0grad [H];
     *   bit 1 (the top layer's job): P = (g . W_head) * mask, d_p = d loss / d output f32 [rows][4], d_maskbits = the top layer's
     *     mask bits u32 [rows][4] written by tg_mlp_f32_forward_backward; rider: the HEAD's gradient -- d_a_top = the top
     *     activation f32 [rows][H], d_whgrad f32 act_dim x H (row stride whgrad_ld) += g^T A_top, d_bhgrad [act_dim]. */
    int32_t      recompute, in_pad, in_dim, act_dim;
    const float* d_w0;        /* Linear 0 weight f32 [H][in_dim], bias f32 [H] (the master tensors) */
    const float* d_b0;
    const float* d_wh;        /* head weight f32 [act_dim][H] */
    const uint32_t* d_maskbits;
    const float* d_a_top;
    float*       d_whgrad;
    float*       d_bhgrad;
    int64_t      whgrad_ld;
    const float* d_dz0;
    float*       d_w0grad;
    float*       d_b0grad;
    int64_t      w0grad_ld;
} tg_f32_dw_job;
int64_t tg_mlp_f32_weight_grad_workspace(int32_t hidden);
/* d_loss_work / n_loss_rows / d_loss_sums (optional, both pointers or neither): the reduction launch also adds rows [0, n_loss_rows)
 * of d_loss_work (f64 [.][4]: tg_mlp_f32_forward_backward's d_work, n_loss_rows = min(blocks, ceil(rows / 256))) into d_loss_sums
 * (f64 [4]) in a fixed order -- the loss statistics of an update without reduction / accumulation launches of their own. */
int  tg_mlp_f32_weight_grad(int32_t hidden, const tg_f32_dw_job* jobs, int32_t n_jobs, int64_t rows, void* d_workspace,
                            int64_t workspace_bytes, const double* d_loss_work, int32_t n_loss_rows, double* d_loss_sums, void* stream);

/* ---- Optimizer step and derived weight layouts (pipelines: torch.optim.Adam; algorithms/grpo.py:145, ppo.py:183) ----
 * tg_adam_step: torch.optim.Adam's DEFAULT update (foreach path: no amsgrad, weight decay, maximize, capturable) of n_tensors
 *   fp32 tensors in one launch, the same fp32 operation sequence per element as torch's kernels (bit-identical results).
 *   d_table: DEVICE array of n_tensors descriptors (param, grad, exp_avg, exp_avg_sq device pointers; `first` = the running
 *   element offset of the tensor in the launch's index space, ascending; total = the sum of the sizes).  step = the 1-based
 *   step number AFTER the increment (torch's state['step']).  zero_grads != 0: every gradient element is set to 0 once it has
 *   been read -- the NEXT update's optimizer.zero_grad(set_to_none=False) (algorithms/grpo.py:143, ppo.py:181) without a launch.
 * tg_gather_streams: dst[j] = master tensor (code[j] >> 24) element (code[j] & 0xFFFFFF), or 0 where code[j] < 0, converted
 *   to bf16 (is_bf16) or kept f32, for every segment in one launch (d_segments: DEVICE array, `first` as above; the master
 *   tensors are the `p` pointers of d_table).  Rebuilds every derived weight layout after a step. */
typedef struct tg_adam_tensor { float* p; float* g; float* m; float* v; int64_t first; } tg_adam_tensor;
typedef struct tg_gather_segment { void* dst; const int32_t* code; int64_t first; int32_t is_bf16; int32_t pad; } tg_gather_segment;
int  tg_adam_step(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                  int64_t step, int32_t zero_grads, void* stream);
int  tg_gather_streams(const tg_gather_segment* d_segments, int32_t n_segments, int64_t total, const tg_adam_tensor* d_table,
                       void* stream);
/* d_flag[0] |= 1 when, for any tensor of the table, an element of `p` differs bitwise from the same element of `g` (m, v unused). */
int  tg_params_differ(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, int32_t* d_flag, void* stream);
/* tg_adam_step + tg_gather_streams in ONE launch: the thread that updates element e of the launch's index space also writes the new
 * value to every layout position derived from it -- d_inv_start int32 [total + 1] / d_inv_dst: the segments' codes inverted (CSR);
 * a destination is (segment << 26 | element of that segment).  Positions whose code is negative (padding) are not touched: the
 * layouts must have been built once by tg_gather_streams.  Same update, bit for bit. */
int  tg_adam_step_push(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                       int64_t step, int32_t zero_grads, const tg_gather_segment* d_segments, int32_t n_segments,
                       const int32_t* d_inv_start, const int32_t* d_inv_dst, void* stream);
/* Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_(params, max_norm), norm_type 2) with no host round trip.
 * tg_grad_clip_coef: d_out2 = {norm, coef} in float32, norm = ||d_flat[0..n)||_2 and coef = min(1, max_norm / (norm + 1e-6)) formed in
 *   float32 as torch forms it (coef == 1 exactly when nothing is clipped).  The squares are summed in float64 -- no overflow for any
 *   finite float32 input -- as one partial per block in d_work (tg_grad_clip_workspace(n) bytes, 8-byte aligned) and the partials in
 *   a fixed order by a second, one-block launch: no floating-point atomics, the same bytes give the same bits.  n == 0: {0, 1}
 *   (d_flat and d_work may be NULL).  d_out2 may be a row of a larger table that the host reads later.
 * tg_adam_step_clip / tg_adam_step_push_clip: tg_adam_step / tg_adam_step_push on g' = g * *d_coef (one float32 product, rounded
 *   once, as g.mul_(coef) rounds it).  zero_grads == 0: g' is written back, the caller reads clipped gradients; else zeroed as before. */
int64_t tg_grad_clip_workspace(int64_t n);
int  tg_grad_clip_coef(const float* d_flat, int64_t n, double max_norm, float* d_out2, double* d_work, void* stream);
int  tg_adam_step_clip(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                       int64_t step, int32_t zero_grads, const float* d_coef, void* stream);
int  tg_adam_step_push_clip(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2,
                            double eps, int64_t step, int32_t zero_grads, const tg_gather_segment* d_segments, int32_t n_segments,
                            const int32_t* d_inv_start, const int32_t* d_inv_dst, const float* d_coef, void* stream);
/* The four launches above behind tg_kl_control's device control block d_ctl (f64 [8], 8-byte aligned; see tg_kl_control): separate
 * kernels, the same update.  Every thread reads d_ctl[0]; nonzero (a check has latched target_kl's stop): no parameter, moment or
 * derived layout is written, the gradient element is zeroed if zero_grads != 0 and left as it is otherwise (a clip product is not
 * written back).  lr_from_ctl == 1: the step size is (float)((d_ctl[1] / bc1) * -1.0), formed in double on the device, where
 * bc1 = 1 - beta1^step comes from the host by value -- the division tg_adam_step does on the host, so a block that holds `lr` gives
 * tg_adam_step's bits; `lr` itself is then not read.  lr_from_ctl == 0: `lr` by value, as in the plain launch (param groups with
 * rates of their own).  bc1 must lie in (0, 1]. */
int  tg_adam_step_ctl(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                      int64_t step, int32_t zero_grads, const double* d_ctl, int32_t lr_from_ctl, double bc1, void* stream);
int  tg_adam_step_push_ctl(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2,
                           double eps, int64_t step, int32_t zero_grads, const tg_gather_segment* d_segments, int32_t n_segments,
                           const int32_t* d_inv_start, const int32_t* d_inv_dst, const double* d_ctl, int32_t lr_from_ctl, double bc1,
                           void* stream);
int  tg_adam_step_ctl_clip(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2,
                           double eps, int64_t step, int32_t zero_grads, const float* d_coef, const double* d_ctl, int32_t lr_from_ctl,
                           double bc1, void* stream);
int  tg_adam_step_push_ctl_clip(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2,
                                double eps, int64_t step, int32_t zero_grads, const tg_gather_segment* d_segments, int32_t n_segments,
                                const int32_t* d_inv_start, const int32_t* d_inv_dst, const float* d_coef, const double* d_ctl,
                                int32_t lr_from_ctl, double bc1, void* stream);
/* tg_mlp_f32_weight_grad with the optimizer step RIDING on its reduction launch: the thread that completes a gradient element applies
 * tg_adam_step's update to its parameter and (push tables given) tg_adam_step_push's layout writes, then leaves the gradient zeroed
 * (zero_grads) or holding the accumulated value -- what `loss.backward(); optimizer.step()` (algorithms/grpo.py:144-145) leaves, bit
 * for bit, in the launches of the backward pass alone.  h_table: a HOST copy of the optimizer's tensor table; every tensor of it must
 * be exactly one gradient window of `jobs`, whole and contiguous (else an error: a parameter without a window would miss its step).
 * Only where nothing stands between the gradients and the step: one rank (no all-reduce), one chunk of rows per update. */
typedef struct tg_adam_rider {
    const tg_adam_tensor*    h_table;
    int32_t                  n_tensors;
    int32_t                  zero_grads;
    int64_t                  total;
    double                   lr, beta1, beta2, eps;
    int64_t                  step;          /* 1-based, after the increment */
    const tg_gather_segment* d_segments;    /* optional (all three or none): tg_adam_step_push's tables */
    int32_t                  n_segments;
    int32_t                  pad;
    const int32_t*           d_inv_start;
    const int32_t*           d_inv_dst;
} tg_adam_rider;
int  tg_mlp_f32_weight_grad_adam(int32_t hidden, const tg_f32_dw_job* jobs, int32_t n_jobs, int64_t rows, void* d_workspace,
                                 int64_t workspace_bytes, const double* d_loss_work, int32_t n_loss_rows, double* d_loss_sums,
                                 const tg_adam_rider* adam, void* stream);

/* ---- The learner's prologue (algorithms/grpo.py:66-115, algorithms/ppo.py:126-139: returns, group statistics, `x[mask]`) ----
 * tg_returns_moments: tg_rtg_scan + tg_masked_moments of the returns in two launches instead of three, in the form for rollouts of
 *   a few thousand envs (a workgroup stages 64-step strips of 32 envs through LDS; one lane per env runs the recurrence in the
 *   reference's order): d_rtg and d_moments are BIT-identical to tg_rtg_scan / tg_masked_moments.  d_work: f64 [3*n] scratch.
 *   T <= tg_returns_moments_max_horizon() (the strips of a workgroup's 32 envs live in LDS).
 * tg_learn_count: valid entries per 1,024-entry chunk of the flat mask u8 [entries] (time-major [T][n]) and their exclusive prefix
 *   into d_work (tg_learn_count_workspace(entries) bytes); d_total[0] = the number of valid entries, d_total[1] = 1 when
 *   expected_rows >= 0 and differs from it (the host sized its buffers from the rollout's own statistic: a mask edited since then,
 *   or a hand-built trajectory, must not pass silently).
 * tg_learn_compact: for every valid (t, e), in time-major order (the order of `mask.nonzero()`), row r = its rank:
 *     d_idx[r] = t*n + e;   d_xin[r][0..in_pad) = obs[.][t][e] converted to bf16 (xin_bf16) or f32, zero padded, 1 in column
 *     `ones_col` (or -1);   d_act_rows[r][0..A) = act[.][t][e] (optional);   d_dst0[r] = d_src0[t*n + e],  d_dst1[r] = d_src1[..]
 *   (optional [T][n] f32 sources; with d_moments, d_dst0 is tg_group_normalize(mode = norm_mode) of d_src0 evaluated for the valid
 *   entries only -- same arithmetic, bit-identical).  d_offsets = tg_learn_count's d_work.  Rows >= rows_cap are not written.
 *   obs: [S] planes of obs_feat_stride elements (TG_F32 / TG_F64), entry (t, e) at t*n + e; act: f32 [A][T][n]. */
typedef struct tg_compact_args {
    const uint8_t* d_mask; const void* d_offsets;
    int64_t n; int32_t T; int32_t S; int32_t A; int32_t obs_dtype;
    const void* d_obs; int64_t obs_feat_stride; const float* d_act;
    void* d_xin; int32_t in_pad; int32_t xin_bf16; int32_t ones_col; int32_t norm_mode;
    float* d_act_rows; int64_t* d_idx;
    const float* d_src0; float* d_dst0; const float* d_src1; float* d_dst1;
    const double* d_moments; int64_t group_size;
    int64_t rows_cap;
} tg_compact_args;
int  tg_returns_moments_max_horizon(void);
int  tg_returns_moments(const float* d_rew, const uint8_t* d_mask, float gamma, float* d_rtg, int64_t n, int32_t T,
                        int64_t group_size, double* d_moments, double* d_work, void* stream);
int64_t tg_learn_count_workspace(int64_t entries);
int  tg_learn_count(const uint8_t* d_mask, int64_t entries, int64_t expected_rows, void* d_work, int64_t work_bytes, int64_t* d_total,
                    void* stream);
int  tg_learn_compact(const tg_compact_args* args, void* stream);

/* ---- GRPO's per-time-step group baseline (GRPO(baseline="step")) ----
 * tg_grpo_step_advantage: d_rtg f32 [T][n] (tg_rtg_scan / tg_returns_moments) and d_mask u8 [T][n] (any byte pattern; non-zero =
 *   valid) -> d_adv f32 [T][n], two launches, no floating-point atomics, deterministic.  Segment (g, t) = the group_size
 *   consecutive entries at t*n + g*group_size; with V its valid entries and c = |V|:
 *     s1 = sum_V (double)R, mean = s1 / c in f64, b = (float)mean, d = R - b (one rounded f32 subtraction; +0 where invalid),
 *     q = sum_V (double)d * (double)d; a segment with c = 0 contributes nothing.
 *   Per group, in ascending t: Q = sum q, C = sum c, K = the number of steps with c >= 1 (the fitted means);
 *     std = sqrt(Q / (C - K)) in f64, 0 when C - K <= 0.
 *   mode 1: d_adv = d / ((float)std + 1e-8f), both operations rounded f32 (tg_group_normalize's mode 1); mode 0: d_adv = d.
 *   Invalid entries are +0.  No NaN / Inf from finite returns (group_size 1, singleton, empty and constant segments included).
 *   The order of the two segment sums: quads of 4 consecutive entries; W = min(64, the smallest power of two >= the number of
 *   quads) lanes; lane l adds the entries of quads l, l + W, ... in ascending index to a sum that starts at +0; then a
 *   __shfl_down tree with offsets W / 2 .. 1 (lane l += lane l + off), the result in lane 0.
 *   d_work: f64 [3][n / group_size][T] scratch (left holding {c, mean, q} per (group, step)); d_group f64 [n / group_size][3] =
 *   {Q, C, K}.  n == 0: TG_OK, nothing is launched. */
int  tg_grpo_step_advantage(const float* d_rtg, const uint8_t* d_mask, int64_t n, int32_t T, int64_t group_size, int mode,
                            double* d_work, float* d_adv, double* d_group, void* stream);

/* ---- Running observation normalisation (policies: normalize_obs=True) ----
 * The policy owns {count f64 [1], mean f64 [S], m2 f64 [S] = sum of squared deviations} and a derived f32 table [2][S] =
 * {(float)mean, (float)(1 / sqrt(m2 / count + eps))} (count == 0: {0, 1}).  The normalised observation, wherever a policy reads a
 * state, is ONE fp32 expression: xn[k] = clamp((x[k] - table[0][k]) * table[1][k], -clip, +clip) -- subtract, multiply and clamp
 * each rounded on its own, an f64 observation rounded to f32 first, bf16 paths round xn once.  clip = +inf: no clamp.
 * tg_obs_moments: over the valid (t, e) of a trajectory (f32 or f64 planes), per feature s, d_out f64 [S][3] = {count,
 *   sum (x - c[s]), sum (x - c[s])^2} in f64, c = d_center f64 [S] (the running mean: identical on every rank, so the ranks' outputs
 *   add).  Two launches, a fixed summation order: deterministic for a given trajectory shape.  d_work: the workspace-size query's
 *   bytes for (T * n, S).
 * tg_obs_norm_merge: Chan's merge of d_batch f64 [S][3] (tg_obs_moments' output, all-reduced) into d_count / d_mean / d_m2 and the
 *   table rewritten IN PLACE (same allocation: captured graphs and cached arguments stay valid), one small launch, IEEE f64 sqrt
 *   and divide.  d_batch == NULL: only the table is rewritten from the statistics as they stand.
 * tg_obs_normalize_rows: rows x[r][k] at d_x + r * row_stride + k * feat_stride elements (TG_F32 / TG_F64; an SoA slot has
 *   row_stride 1, row-major rows feat_stride 1) -> d_xin[r][0..in_pad): xn in bf16 (xin_bf16) or f32, zero padding, 1 in column
 *   `ones_col` (or -1): tg_learn_compact's row contract.
 * tg_learn_compact_on: tg_learn_compact whose input rows hold xn instead of x; everything else is tg_learn_compact's.
 * tg_fused_rollout_on / tg_fused_rollout_f32_on: the fused rollouts with the three operations applied where the register-resident
 *   state becomes the first layer's operand (separate kernel instantiations; the trajectory records the RAW observation).  d_ptab:
 *   the per-env parameter table of the `_dr` entry points, or NULL; `activation` as in the `_act` entry points. */
int64_t tg_obs_moments_workspace(int64_t entries, int32_t S);
int  tg_obs_moments(const tg_traj* tr, int32_t S, const double* d_center, void* d_work, int64_t work_bytes, double* d_out, void* stream);
int  tg_obs_norm_merge(const double* d_batch, int32_t S, double eps, double* d_count, double* d_mean, double* d_m2, float* d_table,
                       void* stream);
int  tg_obs_normalize_rows(const void* d_x, int32_t x_dtype, int64_t row_stride, int64_t feat_stride, int64_t rows, int32_t S,
                           const float* d_obs_norm, float clip, void* d_xin, int32_t in_pad, int32_t xin_bf16, int32_t ones_col,
                           void* stream);
int  tg_learn_compact_on(const tg_compact_args* args, const float* d_obs_norm, float clip, void* stream);
int  tg_fused_rollout_on(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const void* d_wfrag, const float* d_bias,
                         int32_t hidden, int32_t n_hidden_layers, const float* sigma, const uint64_t* d_rng, int64_t env_offset,
                         int32_t t_begin, int32_t t_end, const float* d_obs_norm, float clip, void* stream);
int  tg_fused_rollout_f32_on(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                             int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                             int64_t env_offset, int32_t t_begin, int32_t t_end, int32_t activation, const float* d_obs_norm, float clip,
                             void* stream);

/* ---- Control decimation: `substeps` physics steps per policy step (additions to ABI 13) ----
 * An env with substeps = k applies each policy action for up to k consecutive calls of the env's own step and stops after the first
 * call that reports `truncated`; call j (from 0) of control step t runs with steps_after = t k + j + 1.  Transition t of the
 * trajectory holds the observation before the first call (slot t), the one sampled action, the state after the last executed call
 * (slot t + 1; zeros when the episode ended), rew[t] = the left-to-right sum of the executed calls' rewards in the trajectory dtype
 * (no contraction), and mask / len in CONTROL steps.  The Philox key stays (env, t) with t the control step: one policy evaluation
 * and one draw per control step.
 * `p` describes the PHYSICS clock: p->timestep is the physics step and p->max_steps = tr->horizon * substeps is required
 * (TG_ERR_ARG otherwise; the entry points without `_sub` refuse such a `p` through their horizon == max_steps check).  Run
 * tg_env_finalize_params on it.  t, t_begin and t_end count control steps.
 * The identity the tests pin: such a rollout with forced actions a[t] is, bit for bit, the plain rollout of the same env with
 * max_steps = k T driven with a[p / k] at physics step p and read at every k-th step.  substeps == 1 gives the bits of the sibling
 * entry point.
 * Each entry takes the arguments of its sibling plus `substeps`; d_ptab (the per-env parameter table of the `_dr` entries) and, for
 * the fused ones, d_obs_norm / clip (tg_fused_rollout_on) may be NULL: one entry per path covers the crossings.
 * tg_rollout_final_state_sub re-runs the last control step -- up to k calls from (obs[:, L-1], act[:, L-1]), starting at physics
 *   count (L-1) k + 1: d_s_final is the state after the last executed call, timeout = !failed(s_final) && (time_rule(the count it
 *   stopped at) || L == T).
 * Limits, refused before any launch: substeps outside [1, 64] (TG_ERR_ARG); swarm envs, agents > 1 (TG_ERR_UNSUPPORTED: the bodies
 * of an env would have to stop at the same physics step); Pendulum (TG_ERR_UNSUPPORTED: its balance terminal and the running count
 * it keeps in len count single steps). */
int  tg_rollout_step_sub(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, int32_t t, const float* d_mean,
                         int64_t mean_row_stride, const float* sigma, const uint64_t* d_rng, int64_t env_offset, int32_t substeps,
                         void* stream);
int  tg_rollout_forced_sub(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, int32_t t_begin, int32_t t_end,
                           int32_t substeps, void* stream);
int  tg_rollout_final_state_sub(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, float* d_s_final, uint8_t* d_timeout,
                                int32_t substeps, void* stream);
int  tg_fused_rollout_sub(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const void* d_wfrag, const float* d_bias,
                          int32_t hidden, int32_t n_hidden_layers, const float* sigma, const uint64_t* d_rng, int64_t env_offset,
                          int32_t t_begin, int32_t t_end, const float* d_obs_norm, float clip, int32_t substeps, void* stream);
int  tg_fused_rollout_f32_sub(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                              int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                              int64_t env_offset, int32_t t_begin, int32_t t_end, int32_t activation, const float* d_obs_norm, float clip,
                              int32_t substeps, void* stream);

/* ---- Actuator lag: a first-order rotor lag in front of every physics step (additions to ABI 13) ----
 * Build-defined, like `_sub` and `_dr`.  p->p[10] = tau, the motor time constant in seconds (slot 10 is read by no env's constants;
 * with a parameter table it is row 10, column i for env slot i).  Every env slot carries a motor state m[A] in float32, in
 * normalised action units (0 = hover thrust), 0 at the reset.  With dt = p->timestep (the physics step),
 *     alpha = (float)(dt / (tau_i + dt))          one IEEE double add and divide, rounded to float once
 * and in front of EVERY call of the env's own step -- each of the up to `substeps` calls of a control step; a lane that has stopped
 * filters no more --
 *     m[k] <- m[k] + alpha * (clip(a[k], -1, 1) - m[k])      three float32 operations, each rounded on its own
 * then step(state, m): the step function is untouched (m lies in [-1, 1], so its clip is the identity).  `act` records the
 * COMMANDED action a; a teacher-forced replay takes commanded actions and filters them again.  mask, len, rewards, the Philox key
 * and termination are those of `_sub`.
 * d_motor: f32 [A][T+1][n], env fastest, obs's conventions: slot t = m at the start of control step t (slot 0: zeros, written by
 * the caller), slot t + 1 = m after step t's executed physics steps while the episode carries on, else 0.
 * The identity the tests pin: a lagged rollout is, bit for bit, tg_rollout_forced on the k T physics steps fed the filtered commands.
 * Each entry takes the arguments of its `_sub` sibling (substeps == 1 included) plus d_motor:
 * tg_rollout_step_lag reads slot t and writes slot t + 1; tg_rollout_forced_lag reads slot t_begin and writes every later slot of
 * its range; the fused entries read slot t_begin, so split launches compose; tg_rollout_final_state_lag reads slot L - 1.
 * With a parameter table the host sees only the nominal p[10]: EVERY entry of the table's row 10 must be finite and >= 0 (the
 * caller's duty; tg_env_randomize and tg_env_param_grid keep it, their factors being finite and > 0).  A negative entry gives a gain
 * above 1 or, at -dt, a division by zero in the lane that reads it.
 * Limits, refused before any launch, beside those of `_sub`: envs other than QUADPOLE2D and QUADPOLE and swarm envs
 * (TG_ERR_UNSUPPORTED); a null d_motor, a non-finite or negative p[10], p[10] == 0 without a table (TG_ERR_ARG: 0 is off). */
int  tg_rollout_step_lag(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, int32_t t, const float* d_mean,
                         int64_t mean_row_stride, const float* sigma, const uint64_t* d_rng, int64_t env_offset, int32_t substeps,
                         float* d_motor, void* stream);
int  tg_rollout_forced_lag(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, int32_t t_begin, int32_t t_end,
                           int32_t substeps, float* d_motor, void* stream);
int  tg_rollout_final_state_lag(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, float* d_s_final, uint8_t* d_timeout,
                                int32_t substeps, const float* d_motor, void* stream);
int  tg_fused_rollout_lag(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const void* d_wfrag, const float* d_bias,
                          int32_t hidden, int32_t n_hidden_layers, const float* sigma, const uint64_t* d_rng, int64_t env_offset,
                          int32_t t_begin, int32_t t_end, const float* d_obs_norm, float clip, int32_t substeps, float* d_motor,
                          void* stream);
int  tg_fused_rollout_f32_lag(const tg_env_params* p, const double* d_ptab, const tg_traj* tr, const float* d_wstream, const float* d_tab,
                              int32_t hidden, int32_t n_hidden_layers, int32_t block_envs, const float* sigma, const uint64_t* d_rng,
                              int64_t env_offset, int32_t t_begin, int32_t t_end, int32_t activation, const float* d_obs_norm, float clip,
                              int32_t substeps, float* d_motor, void* stream);

/* ---- PPO's prologue (algorithms/ppo.py:93-139) without a host round trip ----
 * tg_scatter_rows: d_dst[d_idx[r]] = d_src[r * src_stride] for r < rows -- the critic's values of the valid rows (the no-grad
 *   forward's padded output, column 0) back onto the zeroed [T][n] grid (ppo.py:93 evaluated on the valid rows only).
 * tg_ppo_returns: returns and advantages of every (t, e) and their masked fp64 moments in two launches.  monte_carlo != 0:
 *   R = tg_rtg_scan(rew, mask, gamma), A = R - V (ppo.py:100-111); else tg_gae_scan (ppo.py:112-124: A by GAE(gamma, lam), R = V + A).
 *   d_adv / d_ret f32 [T][n] (distinct); d_moments f64 [2][3] = {count, sum, sum of squares} of the valid advantages, then of the
 *   valid returns; d_work f64 [6 n] scratch.  Bit-identical to tg_rtg_scan / `rtg - V` / tg_gae_scan + tg_masked_moments(group = n).
 * tg_ppo_norm: from d_moments (after the ranks' all-reduce, if any) the f32 [8] the loss heads read through
 *   tg_chain_loss.d_norm8 / tg_loss_args.d_norm + d_coef: {adv mean, 1 / (adv std + 1e-8), ret mean, 1 / (ret std + 1e-8),
 *   -1 / n, c1 / n, kl_coeff / n, n} with the unbiased std clamped at 0, in torch's own order of fp64 / fp32 operations
 *   (ppo.py:138-139, :165-179).
 * tg_gather_rows2: d_dst0[r] = d_src0[d_idx[r]] (and d_dst1 / d_src1 when given): `advantages[mask]`, `returns[mask]`. */
int  tg_scatter_rows(const float* d_src, int64_t src_stride, const int64_t* d_idx, int64_t rows, float* d_dst, void* stream);
int  tg_ppo_returns(const float* d_rew, const float* d_values, const uint8_t* d_mask, float gamma, float lam, int monte_carlo,
                    float* d_adv, float* d_ret, int64_t n, int32_t T, double* d_moments, double* d_work, void* stream);
/* Time-limit bootstrapping, second half: tg_ppo_returns on the rewards with gamma * d_boot[i] added to the reward of env i's last
 * step, t == d_len[i] - 1 -- fp32, r + (gamma * boot), each operation rounded on its own -- without writing d_rew or copying it:
 * bit-identical to tg_ppo_returns on a reward tensor augmented that way.  d_len i32 [n], d_boot f32 [n] (0 = no bootstrap; a
 * d_len[i] outside [1, T] adds nothing).  Same two launches, same d_work / d_moments layout. */
int  tg_ppo_returns_boot(const float* d_rew, const float* d_values, const uint8_t* d_mask, const int32_t* d_len, const float* d_boot,
                         float gamma, float lam, int monte_carlo, float* d_adv, float* d_ret, int64_t n, int32_t T, double* d_moments,
                         double* d_work, void* stream);
int  tg_ppo_norm(const double* d_moments, double c1, double kl_coeff, float* d_norm8, void* stream);
int  tg_gather_rows2(const int64_t* d_idx, int64_t rows, const float* d_src0, float* d_dst0, const float* d_src1, float* d_dst1,
                     void* stream);

/* ---- Running value normalisation (policies: normalize_value=True; PPO) ----
 * The policy owns {count, mean, m2} f64 [1] each (m2 = sum of squared deviations of every return merged so far) and a derived f32
 * table [4] = {(float)mean, (float)sigma, (float)(1 / sigma), 0}, sigma = sqrt(m2 / count + eps) in f64 (count == 0: {0, 1, 1, 0}).
 * The critic predicts (R - mean) / sigma; wherever its output enters a return it is denormalised first, v * table[1] + table[0],
 * in fp32 with the multiply and the add each rounded on its own (no FMA).  The tables are read on the device.
 * tg_scatter_rows_affine: tg_scatter_rows with d_dst[d_idx[r]] = d_src[r * src_stride] * d_table[1] + d_table[0]; entries no row
 *   points at are not written (the zeroed grid stays 0 there).
 * tg_boot_values_affine: the bootstrap rows, d_out[i] = (d_v[i * v_stride] * d_table[1] + d_table[0]) * (float)d_timeout[i] for
 *   i < n in one launch -- the product torch.mul(v, timeout) forms, with the denormalisation in front (d_timeout u8 [n]).
 * tg_value_norm_merge: Chan's merge of d_moments3 f64 [3] = {n_b, sum, sum of squares} of a batch of returns (the second row of
 *   tg_ppo_returns' d_moments, all-reduced; batch variance max(s2 - s1 * (s1 / n_b), 0)) into d_count / d_mean / d_m2, and the
 *   table rewritten IN PLACE; one single-threaded launch, f64 operations rounded one by one, IEEE divide and sqrt.
 *   d_moments3 == NULL (or n_b == 0): the statistics keep their bits, only the table is rewritten.  d_norm8 != NULL: entries 2 and
 *   3 of tg_ppo_norm's f32 [8] become d_table[0] and d_table[2] (the critic's regression target is then (R - mean) / sigma of the
 *   merged statistics); launch it after tg_ppo_norm, and after the last scatter that reads the table, on the same stream. */
int  tg_scatter_rows_affine(const float* d_src, int64_t src_stride, const int64_t* d_idx, int64_t rows, const float* d_table,
                            float* d_dst, void* stream);
int  tg_boot_values_affine(const float* d_v, int64_t v_stride, const uint8_t* d_timeout, int64_t n, const float* d_table, float* d_out,
                           void* stream);
int  tg_value_norm_merge(const double* d_moments3, double eps, double* d_count, double* d_mean, double* d_m2, float* d_table,
                         float* d_norm8, void* stream);
/* PopArt (policies: normalize_value=True, popart=True): tg_value_norm_merge and, in the same launch of one workgroup of 256 threads,
 * the rescale of the critic's last layer d_head_w f32 [hidden], d_head_b f32 [1] that keeps every denormalised prediction where it
 * was while the statistics move from (mean_a, sigma_a) to (mean_n, sigma_n), sigma = sqrt(m2 / count + eps) in f64:
 *   w'[k] = (float)((double)w[k] * r), r = sigma_a / sigma_n;   b' = (float)(((double)b * sigma_a + (mean_a - mean_n)) / sigma_n),
 * every f64 operation rounded on its own.  d_count / d_mean / d_m2 / d_table / d_norm8[2:4] come out bit for bit as
 * tg_value_norm_merge writes them.  The head keeps its bits, and nothing is stored to it, when d_moments3 == NULL, when n_b == 0,
 * when the count before the merge is 0 (a critic never trained against a table has nothing to preserve), or when sigma_a or sigma_n
 * is not a positive finite number.  Refused (TG_ERR_ARG) before any launch: a null statistics, table or head pointer, eps < 0,
 * hidden < 1.  The masters are written by raw pointer: every weight layout derived from the head is stale afterwards. */
int  tg_value_norm_merge_popart(const double* d_moments3, double eps, double* d_count, double* d_mean, double* d_m2, float* d_table,
                                float* d_norm8, float* d_head_w, int32_t hidden, float* d_head_b, void* stream);

/* ---- Privileged critic (policies: privileged_critic={name: (lo, hi)}; PPO) ----
 * The critic of an asymmetric actor-critic reads, behind the observation, the physical parameters its env slot was rolled out with
 * (tg_env_randomize's table), each as a feature on [-1, 1].  tg_privileged_rows forms those input rows from the actor's prepared rows.
 * Row r of d_dst [rows][dst_pad] (bf16 != 0: bf16, else f32; d_src [rows][src_pad] has the same type; both 16-byte aligned):
 *   columns [0, S)      the BITS of d_src[r][0 .. S) -- the actor's prepared row, normalised or not;
 *   column S + k        (float)(((d_ptab[index[k] * n + e] / nominal[k]) - center[k]) * scale[k]), k < count: f64, IEEE divide, every
 *                       operation rounded on its own (no FMA), rounded once to f32 and, on bf16 rows, once more to bf16 (nearest even);
 *                       e = d_idx[r] % n (d_idx: tg_learn_compact's flat t * n + e), or e = r when d_idx == NULL (rows <= n);
 *   the other columns   0, and 1 in ones_col unless it is -1.
 * Every element of every row is written; d_ptab is the f64 [12][n] table.  Refused (TG_ERR_ARG): a null pointer other than d_idx, count
 * outside [1, 12], an index outside [0, 12) or listed twice, S < 1, S > src_pad, S + count > dst_pad, ones_col inside [0, S + count) or
 * >= dst_pad, a pad that is not a multiple of 8 (bf16) / 4 (f32) or above 64, a nominal value that is 0 or not finite, a centre or scale
 * that is not finite, n <= 0, rows < 0.  rows == 0: TG_OK without a launch. */
typedef struct tg_privileged_spec {
    int32_t count;          /* privileged columns, 1..12 */
    int32_t index[12];      /* p[] index of column k */
    double  nominal[12];    /* the env's nominal p[index[k]]: the table holds nominal * factor */
    double  center[12];     /* (lo + hi) / 2 of the factor's range */
    double  scale[12];      /* 2 / (hi - lo), 0 for hi == lo */
} tg_privileged_spec;
int  tg_privileged_rows(const void* d_src, int32_t src_pad, int32_t S, const int64_t* d_idx, int64_t rows, int64_t n,
                        const double* d_ptab, const tg_privileged_spec* spec, void* d_dst, int32_t dst_pad, int32_t bf16,
                        int32_t ones_col, void* stream);

/* ---- Deterministic evaluation and parameter sweeps (Evaluator) ----
 * A mean-action rollout needs no kernel of its own: every sampling site forms a[k] = rn_add(mu[k], rn_mul(sigma[k], eps[k])) with a
 * finite eps (Philox::u01 is in (0, 1]), so the entry points above called with a sigma of exactly 0.0f record a == mu (a mean of -0
 * may come out as +0).  What an evaluation adds is below; `episodes_per_cell` = E, the n env slots of the trajectory are C = n / E
 * cells of E consecutive slots.
 *
 * tg_env_param_grid: a third source of the per-env table d_ptab f64 [12][n] (beside "absent" and tg_env_randomize).  Slot i belongs
 *   to cell c = (env_offset + i) / E.  c is decoded row-major over the swept parameters taken in p[] order (ascending index,
 *   whatever order the struct lists them in): the parameter with the largest index runs fastest, level = c % levels, c /= levels, and
 *   so on down.  Row r of column i = p->p[r], times -- when r is swept -- d_values[first(r) + level(r)], where first(r) is where r's
 *   factor list starts in d_values (the lists are concatenated in the struct's listing order).  Plain IEEE double, no contraction:
 *   a factor of 1.0 reproduces p->p[r] bit for bit, so such a table gives the plain entry point's trajectory bit for bit (above).
 *   Refused (TG_ERR_ARG, nothing launched): a null pointer (d_values may be NULL only with count == 0), count outside [0, 12], an
 *   index outside [0, 12) or listed twice, a level count < 1, episodes_per_cell < 1, n not a multiple of episodes_per_cell,
 *   env_offset < 0, envs that reach beyond the grid's last cell.  The factors themselves live on the device and are not looked at.
 * tg_eval_tile_states: obs[k][0][i] = obs[k][0][i % E] for k < S, E <= i < n, one launch, f32 and f64 trajectories: every cell
 *   starts from the E initial states of cell 0 (drawn there by tg_env_reset).  Nothing else of the trajectory is touched.
 * tg_eval_cells: two launches.
 *   d_returns f64 [n]: [i] = the sum of rew[t][i] over t < len[i], t ascending, each reward converted to f64 and added in f64 (no
 *     contraction); 0 for a slot that is not counted.  A slot is counted when 1 <= len[i] <= T.
 *   d_cells f64 [C][8], row c over the counted slots of cell c = {episodes, sum of returns, sum of squared returns (r * r rounded,
 *     then added), smallest return, largest return, sum of lengths, clock-ended episodes (d_timeout[i] != 0, as
 *     tg_rollout_final_state writes it), episodes ended early (counted and not clock-ended)}.
 *   Summation order of a cell, for both sums: 256 partials, partial j = 0.0 plus the counted slots e = j, j + 256, j + 512, ... of
 *     the cell added in that order; then for s = 128, 64, ..., 1: partial[j] += partial[j + s] for every j < s.  Row value =
 *     partial[0].  No floating-point atomics: the bits depend on the trajectory alone.
 *   A cell without a counted slot reports episodes = 0, sums 0, smallest return +inf and largest return -inf.
 *   Reads d_rew and d_len of the trajectory (not d_mask: len says the same) and d_timeout u8 [n]; writes nothing into it. */
typedef struct tg_param_grid {
    int32_t       count;             /* swept parameters, <= 12 */
    int32_t       index[12];         /* which p[] each of them scales */
    int32_t       levels[12];        /* how many factors each has, >= 1 */
    const double* d_values;          /* DEVICE f64 [sum of levels]: the factor lists, concatenated in listing order */
    int64_t       episodes_per_cell; /* E >= 1 */
} tg_param_grid;
int  tg_env_param_grid(const tg_env_params* p, const tg_param_grid* g, double* d_ptab, int64_t n, int64_t env_offset, void* stream);
int  tg_eval_tile_states(const tg_traj* tr, int32_t S, int64_t episodes_per_cell, void* stream);
int  tg_eval_cells(const tg_traj* tr, const uint8_t* d_timeout, int64_t episodes_per_cell, double* d_returns, double* d_cells,
                   void* stream);

/* ---- Vector env: n auto-resetting env slots behind one launch per step (DeviceVecEnv; additions to ABI 13) ----
 * The gymnasium VectorEnv contract in its SAME_STEP autoreset mode: a step takes actions f32 [n][A] (row-major, as every RL library
 * hands them over), returns observations f32 [n][S], rewards and the terminated / truncated flags, and a slot whose episode ended
 * comes back already reset.  The slots sit at DIFFERENT positions of their episodes; what persists between steps lives in device
 * arrays the caller owns (struct of arrays, env fastest) and nothing a launch takes by value changes from step to step -- a step is
 * one launch: no allocation, no host read, no synchronisation.
 *   d_state     real [S][n]   the current state, in the arithmetic type `dtype`
 *   d_steps     i32  [n]      control steps taken in the slot's current episode
 *   d_balanced  i32  [n]      Pendulum: consecutive balanced steps so far (the other envs neither read nor write it)
 *   d_ep_return f64  [n]      the current episode's rewards, each converted to f64 and added in step order
 *   d_episode   u32  [n]      ordinal of the slot's current episode: the stream id of its reset draw
 * The motor state f32 [A][n] of an actuator lag is the d_motor argument of the two entries (NULL: no lag), not a field.
 * horizon = T, the control steps of an episode (env.max_steps); `p` describes the PHYSICS clock as for the `_sub` entries:
 * p->max_steps = horizon * substeps.  Slot i is global env env_offset + i: shards with consecutive offsets are, bit for bit, the slots
 * of one object (sharding over GPUs).
 *
 * tg_vec_env_step, per slot i with t = d_steps[i]:
 *   1. one control step from d_state[:, i] under d_actions[i][:], exactly as tg_rollout_step's kernel takes it for a running episode:
 *      the env's own step (the plain instantiation when d_ptab == NULL, substeps == 1 and d_motor == NULL), or up to `substeps`
 *      calls of it with steps_after = t substeps + j + 1 (`_sub`), behind the rotor lag with d_motor non-NULL (`_lag`), with the
 *      constants of column i of d_ptab f64 [12][n] when it is non-NULL (`_dr`; the table is the caller's: tg_env_randomize);
 *   2. ended = the step's `truncated` || (Pendulum: the balanced count reached its limit) || t + 1 >= T;
 *      timeout = !failed(new state) && (time_rule(the physics count the step stopped at) || t + 1 == T), tg_rollout_final_state's
 *      rule; d_truncated[i] = ended && timeout (the clock), d_terminated[i] = ended && !timeout (a failure, or Pendulum's balance
 *      terminal); their OR is the reference's "episode over";
 *   3. d_reward[i] = (float)r; d_ep_return[i] += (double)r; where ended: d_final_return[i] = (float)d_ep_return[i],
 *      d_final_length[i] = t + 1 (entries of slots that did not end keep what they held);
 *   4. where ended, in the same launch: d_episode[i] += 1, the new state is tg_env_reset's for (seed, stream_id = d_episode[i],
 *      key_offset = env_offset + i, key_div = 1), and steps, balanced, motor and ep_return go to 0; else steps (and balanced) count on;
 *   5. d_obs f32 [n][S], row i = the next state -- the fresh initial state where the slot was reset -- an f64 state rounded once, on
 *      the store; d_final_obs f32 [n][S], row i = the state the step produced BEFORE the reset.  A wavefront writes its 64 rows of
 *      d_final_obs only when one of its slots ended: rows are defined only where terminated | truncated.
 * tg_vec_env_reset_all: every slot starts a new episode in one launch -- d_episode[i] = 0 when restart != 0, else d_episode[i] + 1;
 *   state and d_obs from that reset draw; steps, balanced, motor (when given) and ep_return zeroed.
 * Refused before any launch: a null pointer other than d_ptab / d_motor, n <= 0, horizon <= 0, env_offset < 0, substeps outside
 * [1, 64], p->max_steps != horizon * substeps, d_obs / d_final_obs not 16-byte aligned, d_actions not aligned to a row of 4 A bytes (TG_ERR_ARG); swarm envs
 * (agents > 1), substeps != 1 on Pendulum, a motor state on an env without rotors, an unknown env or dtype (TG_ERR_UNSUPPORTED);
 * with d_motor, tg_rollout_step_lag's conditions on p->p[10]. */
typedef struct tg_vec_env {
    void*     d_state;
    int32_t*  d_steps;
    int32_t*  d_balanced;
    double*   d_ep_return;
    uint32_t* d_episode;
    int64_t   n;
    int64_t   env_offset;
    uint64_t  seed;
    int32_t   horizon;
    int32_t   dtype;         /* TG_F32 | TG_F64 */
} tg_vec_env;
int  tg_vec_env_step(const tg_env_params* p, const double* d_ptab, int32_t substeps, float* d_motor, const tg_vec_env* v,
                     const float* d_actions, float* d_obs, float* d_reward, uint8_t* d_terminated, uint8_t* d_truncated,
                     float* d_final_obs, float* d_final_return, int32_t* d_final_length, void* stream);
int  tg_vec_env_reset_all(const tg_env_params* p, float* d_motor, const tg_vec_env* v, int32_t restart, float* d_obs, void* stream);

/* ---- Replay buffer: n-step transitions of a vector env for off-policy loops (DeviceReplayBuffer; additions to ABI 13) ----
 * A ring of K = capacity_steps time slots of n env slots each, float32, row-major, row = slot * n + i: one time slot is one
 * contiguous [n][.] block of every array.
 *   d_obs f32 [K n][S], d_act f32 [K n][A], d_next_obs f32 [K n][S], d_rew f32 [K n], d_disc f32 [K n], d_nstep u8 [K n]
 *   d_last_obs f32 [n][S]   the observation each slot's next action is applied to
 *   d_cursor i32 [n]        the time slot the next push writes (equal across slots; a push block reads that of its first slot)
 *   d_filled i32 [n]        time slots written so far, at most K (equal across slots; the sample reads entry 0)
 *   d_open   i32 [n]        stored rows of slot i that the next push still extends, in [0, n_step - 1]
 *   discount[j] = (float)(gamma^j), j = 0 .. n_step.
 * Everything that changes from push to push lives in these device arrays: the arguments of a push are the same every time, so a
 * vector-env step and a push can be captured into one hipGraph.
 *
 * tg_replay_start: d_last_obs = d_obs_in [n][S], d_open = 0; stored rows, d_cursor and d_filled stay.
 * tg_replay_push, one launch; per env slot i with c = d_cursor, o = d_open[i], done = terminated[i] | truncated[i],
 *   nx = done ? d_final_obs[i] : d_obs_in[i]:
 *   row c n + i:                          obs = d_last_obs[i], act = d_actions[i], rew = d_reward[i], next_obs = nx,
 *                                         disc = terminated[i] ? 0 : discount[1], nstep = 1;
 *   rows ((c - j) mod K) n + i, j = 1..o: rew = fadd(rew, fmul(discount[j], d_reward[i])) (two float32 roundings), next_obs = nx,
 *                                         disc = terminated[i] ? 0 : discount[j + 1], nstep = j + 1;
 *   then d_open[i] = done ? 0 : min(o + 1, n_step - 1), d_cursor[i] = (c + 1) mod K, d_filled[i] = min(d_filled[i] + 1, K),
 *   d_last_obs[i] = d_obs_in[i].
 *   Every stored row is therefore at all times a consistent nstep-step transition with the target rew + disc * Q(next_obs): it never
 *   spans an episode boundary, bootstraps through a truncation from final_obs and not at all through a termination.
 * tg_replay_sample, one launch: R = d_filled[0] n; element b takes row d_indices[b], or with d_indices == NULL row
 *   ((uint64)w R) >> 32 for w = word 0 of the Philox draw (seed, idx = b, sub = ordinal >> 32, stream = ordinal & 0xffffffff);
 *   o_obs [B][S], o_act [B][A], o_rew [B], o_next_obs [B][S], o_disc [B] = that row, o_idx i64 [B] = its index.  A row outside
 *   [0, R) is not read: its outputs are NaN.
 * Refused before any launch: a null pointer (d_indices may be NULL), n <= 0, batch <= 0, capacity_steps <= 0, n_step outside
 * [1, 16], capacity_steps < n_step, capacity_steps n >= 2^31, a storage array, d_last_obs or a sample output that is not 16-byte
 * aligned (TG_ERR_ARG); obs_dim outside [1, 32] or act_dim outside [1, 8] (TG_ERR_UNSUPPORTED). */
typedef struct tg_replay {
    float*    d_obs;
    float*    d_act;
    float*    d_next_obs;
    float*    d_rew;
    float*    d_disc;
    uint8_t*  d_nstep;
    float*    d_last_obs;
    int32_t*  d_cursor;
    int32_t*  d_filled;
    int32_t*  d_open;
    int64_t   n;
    int32_t   capacity_steps;
    int32_t   obs_dim;
    int32_t   act_dim;
    int32_t   n_step;
    float     discount[17];
} tg_replay;
int  tg_replay_start(const tg_replay* r, const float* d_obs_in, void* stream);
int  tg_replay_push(const tg_replay* r, const float* d_actions, const float* d_obs_in, const float* d_reward, const uint8_t* d_terminated,
                    const uint8_t* d_truncated, const float* d_final_obs, void* stream);
int  tg_replay_sample(const tg_replay* r, int64_t batch, const int64_t* d_indices, uint64_t seed, uint64_t ordinal, float* o_obs,
                      float* o_act, float* o_rew, float* o_next_obs, float* o_disc, int64_t* o_idx, void* stream);

/* ---- Measurement instruments (bench.py's roofline object; nothing on the product path calls them) ----
 * tg_clock_probe_attach: the update's persistent kernels are bound by the package power limit, i.e. by the shader clock the chip
 *   can hold while they run -- a clock neither rocm-smi's sclk nor a kernel duration shows.  With a probe attached, thread 0 of
 *   every workgroup of the named kernel family stamps s_memtime (shader-clock ticks) and s_memrealtime (100 MHz) at entry and
 *   exit and adds the differences to d_probe[0] / d_probe[1] (and 1 to d_probe[2]): clock = 0.1 GHz x d_probe[0] / d_probe[1].
 *   d_probe: DEVICE array of TG_CLOCK_PROBE_U64 zeroed uint64 (the entry stamps are parked behind the sums), NULL detaches.
 *   Synchronous (a symbol write); per device.  Detached (the default) a kernel pays one scalar load and a branch.
 * tg_mfma_sustained_probe: the chain kernels' bare inner loop -- A fragments from LDS (ds_read_b128), B fragments in registers,
 *   dependent accumulator chains, two waves per SIMD, one workgroup per CU, random data, no global traffic after the prologue --
 *   for `iters` iterations: dtype 0 = v_mfma_f32_16x16x32_bf16 (the bf16 chain kernels' shape), 1 = v_mfma_f32_32x32x2_f32 (the
 *   fp32 chain learner's).  Run back to back until the clock has settled it measures the matrix rate the package sustains under
 *   its power limit: the ceiling the roofline's `sustained_peak` quotes beside the datasheet peak.  d_w: 64 KiB of operands,
 *   d_x: blocks x 512 x 256 B, d_out: blocks x 512 floats; tg_mfma_sustained_probe_flops: flops of one launch. */
enum { TG_PROBE_FWD_CHAIN = 0, TG_PROBE_BWD_CHAIN = 1, TG_PROBE_WEIGHT_GRAD = 2, TG_PROBE_F32_CHAIN = 3, TG_PROBE_F32_WEIGHT_GRAD = 4,
       TG_PROBE_MFMA_LOOP = 5, TG_PROBE_FWD_CHAIN_PLAIN = 6 /* tg_mlp_forward_chain without the loss head: no-grad passes */ };
#define TG_CLOCK_PROBE_U64 (4 + 2 * 4096)
int  tg_clock_probe_attach(int32_t family, void* d_probe);
int  tg_mfma_sustained_probe_blocks(void);
double tg_mfma_sustained_probe_flops(int32_t dtype, int32_t iters);
int  tg_mfma_sustained_probe(int32_t dtype, int32_t iters, const void* d_w, const void* d_x, float* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAJOPT_GRPO_HIP_H */
