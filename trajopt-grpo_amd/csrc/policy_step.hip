// The policy step of a loop on DeviceVecEnv (DeviceActor, trajopt-grpo_amd/policy_step.py): actor forward, sampling head and log-density,
// and the critic's value of the same rows, in ONE launch -- forward only, float32, on v_mfma_f32_16x16x4_f32.
//
// The machine is policy_tile.hpp's 16-row tile (lane layout, operand order, ring and tables: there).  Its A operands are four
// consecutive floats of a weight ROW, and they come from torch's own `nn.Linear.weight` storage on every call: no derived stream, no
// layout that could go stale after an in-place optimizer step, nothing to refresh.
//
// Split: 16 rows per wave, 4 waves per workgroup (64 rows), the net as grid dimension y: the actor's and the critic's workgroups run
// side by side in the same launch and may differ in width, depth and activation (one kernel, the six (H, activation) bodies behind a
// workgroup-uniform switch).  The other split the issue names -- 16 rows per workgroup, the waves splitting the output features --
// was not built: it needs an LDS exchange of the activations per layer, and was not probed.
//
// Weights: a ring of 3 slots of one 16-feature block (H / 16 KiB), two blocks in flight, counted vmcnt + one raw s_barrier per block
// (mfma_ring.hpp's discipline), for EVERY shape.  Why not resident where the net would fit (64-wide, or 128-wide and shallow): a
// workgroup sees 64 rows per round and at most a handful of rounds per launch (4,096 rows: one round on 64 workgroups; 65,536 rows: 2
// on 512), so a resident copy would be loaded once per one or two uses -- the same bytes through the same L2 as the ring moves, but
// all of them in front of the first product instead of under the products of the blocks before.  The first layer (K = S <= 32, rows of
// S floats: not 16-byte aligned in general) is staged once per workgroup as zero-padded scalars in operand order, with the biases and
// the head; the input rows are the vector env's own [n][S] buffer, loaded as scalars (clamped address, selected value: no load under a
// branch) and zero-padded to a multiple of 4 in registers.
//
// Head: <= 8 outputs as fp32 dot products over the lane's features, the four lane groups added in a fixed order (mlp_f32_wide.hip's).
// The epilogue runs per row: every lane group holds the same bits, lane group 0 stores.
//   gaussian   a = mu + exp(log_std) eps,  logp = sum_k(-0.5 eps_k^2 - log_std_k - 0.5 log 2 pi),  mean = mu
//   squashed   (mu, ls) = split(out), ls clamped to [lo, hi], u = mu + exp(ls) eps, a = tanh(u),
//              logp = the gaussian's - sum_k log(1 - a_k^2 + 1e-6),  mean = tanh(mu)
//   eps        the rollout kernels' float32 Box-Muller (fused_rollout_f32.hip) on Philox::draw(seed, env_offset + i, calls[i],
//              TG_POLICY_STEP_STREAM); calls[i] is a device counter the row's own lane increments: nothing changes by value between
//              two replays of a captured launch, and the draw of slot i at its k-th call depends on neither n, the grid nor a sharding.
//   deterministic: eps = 0 by select, the counters stay.
#include <stdlib.h>

#include "tg_common.hpp"
#include "policy_tile.hpp"

namespace tg {

struct PsArgs {
    PolicyNet net[2];               // [0] the actor, [1] the critic
    int32_t first_role;             // blockIdx.y + first_role: the net a workgroup runs (1: a critic-only launch)
    int32_t head, act_dim, deterministic;
    const float* x;                 // [rows][S], unpadded
    int64_t rows;
    const float* log_std;           // gaussian head: [A]
    uint32_t* calls;                // [rows]
    uint64_t seed;
    int64_t env_offset;
    float ls_lo, ls_hi;
    float* action; float* logp; float* mean; float* value;
};

template <int H, int kAct>
__device__ __attribute__((always_inline)) static inline void ps_forward(const PsArgs& a, const int S, const int nh, const int O,
                                                                        const int role, uint4* lds) {
    constexpr int NT = H / 16, D = kTileD, P = kTileP, SLOT = NT * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int n_hh = nh - 1, K4 = (S + 3) >> 2;
    const bool critic = role == 1;
    uint4* ring = lds;
    const NetTables<H> tb(reinterpret_cast<float*>(ring + D * SLOT), K4, nh, O);
    const int64_t rows = a.rows;
    const int64_t n_rounds = (rows + 63) / 64;

    // ---- the ring: block (l, mo) = output features 16 mo .. + 15 of H x H layer l, straight out of W_l ----
    int pre_l = 1, pre_mo = 0, pre_slot = 0, cur_slot = 0;
    auto dma_next = [&]() {
        ring_dma_rows<NT>(net_weight(a, critic, pre_l) + ((16 * pre_mo + j) * H + 4 * g), ring + pre_slot * SLOT, wave);
        pre_mo = (pre_mo + 1 == NT) ? 0 : pre_mo + 1;
        pre_l = pre_mo != 0 ? pre_l : (pre_l == n_hh ? 1 : pre_l + 1);
        pre_slot = (pre_slot + 1 == D) ? 0 : pre_slot + 1;
    };
    if (n_hh > 0) {
#pragma unroll
        for (int b = 0; b < P; ++b) dma_next();
    }
    stage_net_tables<H>(net_weight(a, critic, 0), S, nh, O, [&](int l) { return net_bias(a, critic, l); }, net_weight(a, critic, nh),
                        net_bias(a, critic, nh), tb.w0, tid);
    __syncthreads();                                                  // (the tables; drains the prologue's DMA too: once)
    auto no_tile = [](int, int, const f32x4&) {};

    for (int64_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const int64_t row = round * 64 + wave * 16 + j;
        const bool valid = row < rows;
        const int64_t rowc = valid ? row : rows - 1;
        f32x4 xin[NT];

        // ---- layer 0: lane group g holds x[4 s + g] of its row for the steps s < K4 (no load under a branch) ----
        float xr[kTileMaxIn / 4];
#pragma unroll
        for (int s = 0; s < kTileMaxIn / 4; ++s) {
            const int k = 4 * s + g;
            const bool in = k < S;
            const float v = a.x[rowc * S + (in ? k : 0)];
            xr[s] = in ? v : 0.f;
        }
        first_layer<H, kAct>(tb.w0, tb.bias, K4, lane, xr, xin, no_tile);
        hidden_layers<H, kAct>(ring, cur_slot, tb.bias, n_hh, lane, xin, dma_next, no_tile);
        const int A = critic ? 1 : a.act_dim;
        const bool squashed = !critic && a.head == TG_POLICY_HEAD_SQUASHED, det = a.deterministic != 0;
        float mu_k[4] = {0.f, 0.f, 0.f, 0.f}, ls_k[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < A) {
                mu_k[k] = head_out<NT>(tb.wh, tb.bh, xin, k, g);
                if (squashed) ls_k[k] = head_out<NT>(tb.wh, tb.bh, xin, A + k, g);
            }
        }
        const bool store = valid && g == 0;
        if (critic) {
            if (store) a.value[row] = mu_k[0];
            continue;
        }
        // ---- the actor's epilogue, per row ----
        const uint32_t calls = a.calls[rowc];
        uint32_t rnd[4];
        Philox::draw(a.seed, (uint64_t)(a.env_offset + rowc), calls, TG_POLICY_STEP_STREAM, rnd);
        float eps[4];
        box_muller_eps(rnd, A, eps);
        float logp = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < A) {
                const float e = det ? 0.f : eps[k];
                const float ls_free = a.log_std[k];
                const float ls = squashed ? fminf(fmaxf(ls_k[k], a.ls_lo), a.ls_hi) : ls_free;
                const float mu = mu_k[k];
                const float u = rn_add(mu, rn_mul(expf(ls), e));
                float act = u, mean = mu;
                float lp = gaussian_logp_term(e, ls);
                if (squashed) {
                    act = tanhf(u);
                    mean = tanhf(mu);
                    lp = rn_sub(lp, squash_logp_term(act));
                }
                logp = rn_add(logp, lp);
                if (store) {
                    a.action[row * A + k] = act;
                    a.mean[row * A + k] = mean;
                }
            }
        }
        if (store) {
            a.logp[row] = logp;
            if (!det) a.calls[row] = calls + 1u;
        }
    }
    // the ring's prefetches of a round that never came: let them land before the workgroup's LDS goes away
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(64 * kTileWaves, 2) void policy_step_kernel(PsArgs a) {
    extern __shared__ uint4 lds[];
    const int role = __builtin_amdgcn_readfirstlane((int)blockIdx.y + a.first_role);
    const bool critic = role == 1;
    const int S = critic ? a.net[1].S : a.net[0].S, H = critic ? a.net[1].H : a.net[0].H, nh = critic ? a.net[1].nh : a.net[0].nh;
    const int O = critic ? a.net[1].O : a.net[0].O, act = critic ? a.net[1].act : a.net[0].act;
    dispatch_width_act(H, act, [&](auto h, auto k) __attribute__((always_inline)) {
        ps_forward<decltype(h)::value, decltype(k)::value>(a, S, nh, O, role, lds);
    });
}

static int ps_launch(const char* who, PsArgs& args, int nets, int32_t grid_limit, hipStream_t st) {
    size_t shmem = 0;
    for (int r = args.first_role; r < args.first_role + nets; ++r) {
        const size_t b = ring_tables_lds_bytes(args.net[r]);
        shmem = b > shmem ? b : shmem;
    }
    static LdsOptIn opt_in;
    return launch_row_tiles(who, policy_step_kernel, opt_in, args, nets, shmem, grid_limit, 2, st);
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_policy_step_limits(int32_t* max_obs_dim, int32_t* max_hidden_layers, int32_t* max_act_dim) {
    TG_REQUIRE(max_obs_dim && max_hidden_layers && max_act_dim, "tg_policy_step_limits: null pointer");
    *max_obs_dim = kTileMaxIn; *max_hidden_layers = kPolicyLinear - 1; *max_act_dim = 4;
    return TG_OK;
}

int tg_policy_step(const tg_policy_net* actor, const tg_policy_net* critic, const tg_policy_step_args* s, void* stream) {
    const char* who = "tg_policy_step";
    TG_REQUIRE(s != nullptr, "%s: null arguments", who);
    TG_REQUIRE(s->head == TG_POLICY_HEAD_GAUSSIAN || s->head == TG_POLICY_HEAD_SQUASHED, "%s: unknown head %d", who, s->head);
    TG_REQUIRE(s->act_dim >= 1 && s->act_dim <= 4, "%s: act_dim=%d outside [1, 4]", who, s->act_dim);
    TG_REQUIRE(s->n > 0 && s->n < ((int64_t)1 << 31) && s->env_offset >= 0, "%s: n=%lld outside [1, 2^31) or a negative env_offset", who,
               (long long)s->n);
    const bool squashed = s->head == TG_POLICY_HEAD_SQUASHED;
    PsArgs args = {};
    if (int rc = policy_net_check(who, "the actor", actor, squashed ? 2 * s->act_dim : s->act_dim, true, args.net[0])) return rc;
    if (critic != nullptr) {
        if (int rc = policy_net_check(who, "the critic", critic, 1, true, args.net[1])) return rc;
        TG_REQUIRE(args.net[1].S == args.net[0].S, "%s: the critic reads %d inputs, the actor %d", who, args.net[1].S, args.net[0].S);
        TG_REQUIRE(s->d_value != nullptr, "%s: d_value is null with a critic", who);
    }
    TG_REQUIRE(s->d_obs && s->d_calls && s->d_action && s->d_logp && s->d_mean, "%s: null pointer", who);
    TG_REQUIRE(squashed || s->d_log_std != nullptr, "%s: the gaussian head needs d_log_std", who);
    TG_REQUIRE(!squashed || s->log_std_lo <= s->log_std_hi, "%s: log_std bounds [%g, %g] are empty", who, (double)s->log_std_lo,
               (double)s->log_std_hi);
    args.first_role = 0; args.head = s->head; args.act_dim = s->act_dim; args.deterministic = s->deterministic;
    args.x = s->d_obs; args.rows = s->n;
    args.log_std = s->d_log_std ? s->d_log_std : s->d_mean;          // (squashed: read and not used -- no load under a branch)
    args.calls = s->d_calls; args.seed = s->seed; args.env_offset = s->env_offset;
    args.ls_lo = s->log_std_lo; args.ls_hi = s->log_std_hi;
    args.action = s->d_action; args.logp = s->d_logp; args.mean = s->d_mean; args.value = s->d_value;
    return ps_launch(who, args, critic ? 2 : 1, s->grid_limit, (hipStream_t)stream);
}

int tg_policy_values(const tg_policy_net* critic, const float* d_x, int64_t m, float* d_value, int32_t grid_limit, void* stream) {
    const char* who = "tg_policy_values";
    PsArgs args = {};
    if (int rc = policy_net_check(who, "the critic", critic, 1, true, args.net[1])) return rc;
    TG_REQUIRE(d_x && d_value, "%s: null pointer", who);
    TG_REQUIRE(m > 0 && m < ((int64_t)1 << 31), "%s: m=%lld outside [1, 2^31)", who, (long long)m);
    args.net[0] = args.net[1];
    args.first_role = 1; args.x = d_x; args.rows = m; args.value = d_value;
    return ps_launch(who, args, 1, grid_limit, (hipStream_t)stream);
}

}  // extern "C"
