// The policy step of a loop on DeviceVecEnv (DeviceActor, trajopt-grpo_amd/policy_step.py): actor forward, sampling head and log-density,
// and the critic's value of the same rows, in ONE launch -- forward only, float32, on v_mfma_f32_16x16x4_f32.
//
// The machine is mlp_f32_wide.hip's 16-row tile: a wave owns 16 rows; lane (j = lane & 15, g = lane >> 4) of accumulator tile t holds
// features 16 t + 4 g + r (r = 0..3) of row j, and register r of the four lane groups IS the B operand of MFMA step (t, r) of the next
// layer.  The A operand of that step, lane (i, g), is W[out i][16 t + 4 g + r]: four consecutive floats of a weight ROW.  What is new
// here is where those floats come from: torch's own `nn.Linear.weight` storage, row-major [out][in], on every call.  The 16 output
// features of a block are one contiguous 16 x H float region of it; piece t of the block (1 KiB in LDS, lane (i, g) at byte 16 lane) is
// lane (i, g)'s 16 bytes at W + (16 mo + i) H + 16 t + 4 g: an LDS-DMA whose 64 lane addresses are 16 runs of 64 B.  No derived stream,
// no layout that could go stale after an in-place optimizer step, nothing to refresh.
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
#include "mfma_ring.hpp"
#include "act_f32.hpp"

namespace tg {

constexpr int kPsLinear = TG_POLICY_MAX_LAYERS;         // Linear layers of a net: up to 5 hidden layers and the head
constexpr int kPsWaves = 4;
constexpr int kPsD = 3, kPsP = kPsD - 1;                // ring slots, blocks in flight
constexpr int kPsMaxOut = 8;
constexpr int kPsMaxIn = 32;

struct PsNet {
    const float* w[kPsLinear];
    const float* b[kPsLinear];
    int32_t S, H, nh, O, act;                           // input width, hidden width, hidden layers, head outputs, TG_ACT_*
};

struct PsArgs {
    PsNet net[2];                   // [0] the actor, [1] the critic
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

__device__ static inline uint4 ps_lds_u4(const uint4* __restrict__ p) { return *p; }
__device__ static inline float4 ps_lds_f4(const float* __restrict__ p) { return *reinterpret_cast<const float4*>(p); }
__device__ static inline float ps_lds_f(const float* __restrict__ p) { return *p; }

static size_t ps_lds_bytes(const PsNet& n) {
    const int NT = n.H / 16, K4 = (n.S + 3) / 4;
    return (size_t)kPsD * NT * 1024 + (size_t)NT * K4 * 256 + (size_t)(n.nh + n.O) * n.H * 4 + kPsMaxOut * 4;
}

// Layer l's weight / bias pointer of the workgroup's net.  A run-time index into a local copy of the tables puts it into scratch:
// uniform selects over the kernel arguments themselves instead (l and `critic` are workgroup-uniform).
__device__ static inline const float* ps_weight(const PsArgs& a, bool critic, int l) {
    const float* r = critic ? a.net[1].w[0] : a.net[0].w[0];
#pragma unroll
    for (int q = 1; q < kPsLinear; ++q) r = l == q ? (critic ? a.net[1].w[q] : a.net[0].w[q]) : r;
    return r;
}
__device__ static inline const float* ps_bias(const PsArgs& a, bool critic, int l) {
    const float* r = critic ? a.net[1].b[0] : a.net[0].b[0];
#pragma unroll
    for (int q = 1; q < kPsLinear; ++q) r = l == q ? (critic ? a.net[1].b[q] : a.net[0].b[q]) : r;
    return r;
}
template <int H, int kAct>
__device__ __attribute__((always_inline)) static inline void ps_forward(const PsArgs& a, const int S, const int nh, const int O,
                                                                        const int role, uint4* lds) {
    constexpr int NT = H / 16, KS = NT, WPW = kPsWaves, D = kPsD, P = kPsP, SLOT = KS * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int n_hh = nh - 1, K4 = (S + 3) >> 2;
    const bool critic = role == 1;
    uint4* ring = lds;
    float* w0_s = reinterpret_cast<float*>(ring + D * SLOT);          // [NT][K4][64 lanes]: lane (i, g) of step s holds W0[16 mo + i][4 s + g]
    float* bias_s = w0_s + NT * K4 * 64;                              // [nh][H]
    float* wh_s = bias_s + nh * H;                                    // [O][H]
    float* bh_s = wh_s + O * H;                                       // [8]
    const int64_t rows = a.rows;
    const int64_t n_rounds = (rows + 63) / 64;

    // ---- the ring: block (l, mo) = output features 16 mo .. + 15 of H x H layer l, straight out of W_l ----
    int pre_l = 1, pre_mo = 0, pre_slot = 0, cur_slot = 0;
    auto dma_next = [&]() {
        const float* src = ps_weight(a, critic, pre_l) + ((16 * pre_mo + j) * H + 4 * g);
        uint4* slot = ring + pre_slot * SLOT;
#pragma unroll
        for (int q = 0; q < KS / WPW; ++q) {
            const int piece = q * WPW + wave;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint4*>(src + 16 * piece), (lds_void*)(slot + piece * 64), 16, 0, 0);
        }
        pre_mo = (pre_mo + 1 == NT) ? 0 : pre_mo + 1;
        pre_l = pre_mo != 0 ? pre_l : (pre_l == n_hh ? 1 : pre_l + 1);
        pre_slot = (pre_slot + 1 == D) ? 0 : pre_slot + 1;
    };
    if (n_hh > 0) {
#pragma unroll
        for (int b = 0; b < P; ++b) dma_next();
    }
    // ---- staged once per workgroup: the first layer in operand order, zero-padded to K4 steps; the biases; the head ----
    const float* w0 = ps_weight(a, critic, 0);
    for (int q = tid; q < NT * K4 * 64; q += 64 * WPW) {
        const int ln = q & 63, ps = q >> 6, mo = ps / K4, s = ps - mo * K4;
        const int k = 4 * s + (ln >> 4);
        const bool in = k < S;
        const float v = w0[(16 * mo + (ln & 15)) * S + (in ? k : 0)];
        w0_s[q] = in ? v : 0.f;
    }
    for (int l = 0; l < nh; ++l) {
        const float* bl = ps_bias(a, critic, l);
        for (int q = tid; q < H; q += 64 * WPW) bias_s[l * H + q] = bl[q];
    }
    {
        const float* Wh = ps_weight(a, critic, nh);
        const float* Bh = ps_bias(a, critic, nh);
        for (int q = tid; q < O * H; q += 64 * WPW) wh_s[q] = Wh[q];
        const float bv = Bh[tid < O ? tid : 0];
        if (tid < kPsMaxOut) bh_s[tid] = tid < O ? bv : 0.f;
    }
    __syncthreads();                                                  // (the tables; drains the prologue's DMA too: once)
    // counted wait for the block about to be consumed: behind its DMA there are always the pieces of the P - 1 later blocks.  The
    // input loads and output stores of a round are issued behind them too and are NOT counted: stricter, never weaker.
    constexpr int kWait = (P - 1) * (KS / WPW);

    auto act4 = [&](f32x4& v) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = act_f32<kAct>(v[r]);
    };
    // one 16-feature output tile against a whole H-wide operand (mlp_f32_wide.hip's tile_products): two accumulator chains, the A
    // operands of pieces t + 2, t + 3 requested before the products of pieces t, t + 1; the block's DMA successor is issued behind
    // the first reads
    auto tile_products = [&](const uint4* __restrict__ cur, const f32x4 (&xin)[NT], f32x4 acc) {
        const uint4* __restrict__ p = cur + lane;
        f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
        uint4 wa = ps_lds_u4(p), wb = ps_lds_u4(p + 64);
        dma_next();
#pragma unroll
        for (int t = 0; t < NT; t += 2) {
            uint4 na = wa, nb = wb;
            if (t + 2 < NT) { na = ps_lds_u4(p + (t + 2) * 64); nb = ps_lds_u4(p + (t + 3) * 64); }
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wa.x), xin[t][0], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wb.x), xin[t + 1][0], acc1, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wa.y), xin[t][1], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wb.y), xin[t + 1][1], acc1, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wa.z), xin[t][2], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wb.z), xin[t + 1][2], acc1, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wa.w), xin[t][3], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wb.w), xin[t + 1][3], acc1, 0, 0, 0);
            wa = na; wb = nb;
        }
        return acc + acc1;                                            // (a fixed order: deterministic)
    };

    for (int64_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const int64_t row = round * 64 + wave * 16 + j;
        const bool valid = row < rows;
        const int64_t rowc = valid ? row : rows - 1;
        f32x4 xin[NT], xout[NT];

        // ---- layer 0: lane group g holds x[4 s + g] of its row for the steps s < K4 (no load under a branch) ----
        float xr[kPsMaxIn / 4];
#pragma unroll
        for (int s = 0; s < kPsMaxIn / 4; ++s) {
            const int k = 4 * s + g;
            const bool in = k < S;
            const float v = a.x[rowc * S + (in ? k : 0)];
            xr[s] = in ? v : 0.f;
        }
#pragma unroll
        for (int mo = 0; mo < NT; ++mo) {
            const float4 b4 = ps_lds_f4(bias_s + 16 * mo + 4 * g);
            f32x4 acc = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int s = 0; s < kPsMaxIn / 4; ++s)
                if (s < K4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ps_lds_f(w0_s + (mo * K4 + s) * 64 + lane), xr[s], acc, 0, 0, 0);
            act4(acc);
            xin[mo] = acc;
        }
        // ---- hidden H x H layers: one ring block per 16 output features ----
        for (int l = 1; l <= n_hh; ++l) {
            const float* bias_l = bias_s + l * H + 4 * g;
#pragma unroll
            for (int mo = 0; mo < NT; ++mo) {
                TG_RING_WAIT(kWait)
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                const uint4* cur = ring + cur_slot * SLOT;
                cur_slot = (cur_slot + 1 == D) ? 0 : cur_slot + 1;
                const float4 b4 = ps_lds_f4(bias_l + 16 * mo);
                f32x4 acc = tile_products(cur, xin, f32x4{b4.x, b4.y, b4.z, b4.w});
                act4(acc);
                xout[mo] = acc;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) xin[t] = xout[t];
        }
        // ---- head: fp32 dot products over the lane's features, the four lane groups added in a fixed order ----
        // (a head row is addressed in LDS by a uniform run-time index: the squashed head's log-std rows A .. 2 A - 1 need no
        // run-time index into a register array)
        auto head_out = [&](int k) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float4 w = ps_lds_f4(wh_s + k * H + 16 * t + 4 * g);
                s = fmaf(xin[t][0], w.x, s);
                s = fmaf(xin[t][1], w.y, s);
                s = fmaf(xin[t][2], w.z, s);
                s = fmaf(xin[t][3], w.w, s);
            }
            // (g0 + g1) + (g2 + g3): every lane group ends up with the same bits
            const float p1 = __shfl_xor(s, 16, 64);
            const float pair = (g & 1) ? p1 + s : s + p1;
            const float p2 = __shfl_xor(pair, 32, 64);
            return ((g & 2) ? p2 + pair : pair + p2) + ps_lds_f(bh_s + k);
        };
        const int A = critic ? 1 : a.act_dim;
        const bool squashed = !critic && a.head == TG_POLICY_HEAD_SQUASHED, det = a.deterministic != 0;
        float mu_k[4] = {0.f, 0.f, 0.f, 0.f}, ls_k[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < A) {
                mu_k[k] = head_out(k);
                if (squashed) ls_k[k] = head_out(A + k);
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
        float eps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            if (2 * hh < A) {
                const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(Philox::u01(rnd[2 * hh])));
                const float rev = Philox::u01(rnd[2 * hh + 1]);
                eps[2 * hh] = rad * __builtin_amdgcn_cosf(rev);
                eps[2 * hh + 1] = rad * __builtin_amdgcn_sinf(rev);
            }
        }
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
                float lp = rn_sub(rn_sub(rn_mul(-0.5f, rn_mul(e, e)), ls), 0.91893853320467274f);
                if (squashed) {
                    act = tanhf(u);
                    mean = tanhf(mu);
                    lp = rn_sub(lp, logf(rn_add(rn_sub(1.0f, rn_mul(act, act)), 1e-6f)));
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

__global__ __launch_bounds__(64 * kPsWaves, 2) void policy_step_kernel(PsArgs a) {
    extern __shared__ uint4 lds[];
    const int role = __builtin_amdgcn_readfirstlane((int)blockIdx.y + a.first_role);
    const bool critic = role == 1;
    const int S = critic ? a.net[1].S : a.net[0].S, H = critic ? a.net[1].H : a.net[0].H, nh = critic ? a.net[1].nh : a.net[0].nh;
    const int O = critic ? a.net[1].O : a.net[0].O, act = critic ? a.net[1].act : a.net[0].act;
    const bool tanh_net = act == TG_ACT_TANH;
    if (H == 64) {
        if (tanh_net) ps_forward<64, TG_ACT_TANH>(a, S, nh, O, role, lds); else ps_forward<64, TG_ACT_RELU>(a, S, nh, O, role, lds);
    } else if (H == 128) {
        if (tanh_net) ps_forward<128, TG_ACT_TANH>(a, S, nh, O, role, lds); else ps_forward<128, TG_ACT_RELU>(a, S, nh, O, role, lds);
    } else {
        if (tanh_net) ps_forward<256, TG_ACT_TANH>(a, S, nh, O, role, lds); else ps_forward<256, TG_ACT_RELU>(a, S, nh, O, role, lds);
    }
}

// what both entries refuse about a net; `outs`: the head outputs the caller expects
static int ps_fill_net(const char* who, const char* name, const tg_policy_net* n, int outs, PsNet& out) {
    TG_REQUIRE(n != nullptr, "%s: the %s table is null", who, name);
    TG_REQUIRE(n->n_layers >= 2 && n->n_layers <= kPsLinear, "%s: %s has %d Linear layers, outside 2..%d (1..%d hidden layers)", who, name,
               n->n_layers, kPsLinear, kPsLinear - 1);
    TG_REQUIRE(n->activation == TG_ACT_RELU || n->activation == TG_ACT_TANH, "%s: %s has an unknown hidden activation %d", who, name,
               n->activation);
    const int L = n->n_layers, S = n->in_dim[0], H = n->out_dim[0], O = n->out_dim[L - 1];
    TG_REQUIRE(S >= 1 && S <= kPsMaxIn, "%s: %s has input width %d outside [1, %d]", who, name, S, kPsMaxIn);
    TG_REQUIRE(H == 64 || H == 128 || H == 256, "%s: %s has hidden width %d (64, 128 or 256)", who, name, H);
    for (int l = 0; l < L; ++l) {
        TG_REQUIRE(n->w[l] && n->b[l], "%s: %s layer %d has a null weight or bias", who, name, l);
        TG_REQUIRE((l == 0 || n->in_dim[l] == H) && (l == L - 1 || n->out_dim[l] == H), "%s: %s layer %d is %d -> %d, hidden width %d", who,
                   name, l, n->in_dim[l], n->out_dim[l], H);
        // the H x H layers are read 16 bytes at a time, everything else as floats
        const uintptr_t mask = (l > 0 && l < L - 1) ? 15 : 3;
        TG_REQUIRE(((uintptr_t)n->w[l] & mask) == 0 && ((uintptr_t)n->b[l] & 3) == 0, "%s: %s layer %d has a misaligned weight or bias pointer",
                   who, name, l);
        out.w[l] = n->w[l];
        out.b[l] = n->b[l];
    }
    for (int l = L; l < kPsLinear; ++l) { out.w[l] = n->w[0]; out.b[l] = n->b[0]; }
    TG_REQUIRE(O == outs, "%s: %s has %d head outputs, %d expected", who, name, O, outs);
    out.S = S; out.H = H; out.nh = L - 1; out.O = O; out.act = n->activation;
    return TG_OK;
}

static int ps_launch(const char* who, PsArgs& args, int nets, int32_t grid_limit, hipStream_t st) {
    size_t shmem = 0;
    for (int r = args.first_role; r < args.first_role + nets; ++r) {
        const size_t b = ps_lds_bytes(args.net[r]);
        shmem = b > shmem ? b : shmem;
    }
    static LdsOptIn opt_in;
    if (int rc = reserve_dynamic_lds((const void*)policy_step_kernel, shmem, opt_in, who)) return rc;
    const int64_t tiles = ceil_div(args.rows, 64);
    const int64_t cap = grid_limit > 0 ? grid_limit : 2 * device_cus();
    hipLaunchKernelGGL(policy_step_kernel, dim3((unsigned)(tiles < cap ? tiles : cap), (unsigned)nets), dim3(64 * kPsWaves), shmem, st, args);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_policy_step_limits(int32_t* max_obs_dim, int32_t* max_hidden_layers, int32_t* max_act_dim) {
    TG_REQUIRE(max_obs_dim && max_hidden_layers && max_act_dim, "tg_policy_step_limits: null pointer");
    *max_obs_dim = kPsMaxIn; *max_hidden_layers = kPsLinear - 1; *max_act_dim = 4;
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
    if (int rc = ps_fill_net(who, "the actor", actor, squashed ? 2 * s->act_dim : s->act_dim, args.net[0])) return rc;
    if (critic != nullptr) {
        if (int rc = ps_fill_net(who, "the critic", critic, 1, args.net[1])) return rc;
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
    if (int rc = ps_fill_net(who, "the critic", critic, 1, args.net[1])) return rc;
    TG_REQUIRE(d_x && d_value, "%s: null pointer", who);
    TG_REQUIRE(m > 0 && m < ((int64_t)1 << 31), "%s: m=%lld outside [1, 2^31)", who, (long long)m);
    args.net[0] = args.net[1];
    args.first_role = 1; args.x = d_x; args.rows = m; args.value = d_value;
    return ps_launch(who, args, 1, grid_limit, (hipStream_t)stream);
}

}  // extern "C"
