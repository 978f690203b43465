// Q critics on (obs, action) rows and the SAC target of a batch in ONE launch (DeviceActor.q_values / .sac_target,
// trajopt-grpo_amd/policy_step.py) -- forward only, float32, on v_mfma_f32_16x16x4_f32.
//
//   q_values     q1[m] = Q1(obs_m, act_m), and with a second net q2[m] = Q2(obs_m, act_m), qmin[m] = min(q1, q2)
//   sac_target   a', logp = the squashed head of actor(obs_m) at the slot's next Philox draw (tg_policy_step's arithmetic, its
//                counters, its stream constant), q1 = Q1'(obs_m, a'), q2 = Q2'(obs_m, a'),
//                y = rn_add(r, rn_mul(d, rn_sub(min(q1, q2), rn_mul(alpha, logp)))): one float32 rounding per operation (this file
//                is built without packed fp32 instructions, as segment.hip is), alpha read from a device scalar at every call
//
// The machine is policy_tile.hpp's 16-row tile (lane layout, operand order, ring and tables: there), the one policy_step.hip runs.
// Constants, LDS reads, the net refusals and the launch are that header's.  The tile routines and the sampling head in pq_forward
// are this file's OWN TEXT of the header's (tests/test_sac_target_gpu.py holds the actor's bits to tg_policy_step's): at B = 256 a
// launch is one round of four workgroups, 21.7 us from a graph, and every form of this body built on the header's routines -- one at
// a time or all together -- moved that by + 0.07 to + 0.4 us (and the 128-wide kernel by - 0.3 to + 0.3 us), reproducibly to
// 0.02 us.  Whoever changes a routine there changes its twin here.
//
// What is new: ONE wave runs up to three nets back to back on its 16 rows -- the actor, Q1, Q2 -- and keeps what passes from one
// to the next in registers.  A critic's input row is obs[row][0..S) followed by the A <= 4 action values, zero-padded to a multiple
// of 4: lane group g of first-layer step s holds input k = 4 s + g.  The observation part is loaded once per round (clamped address,
// selected value: no load under a divergent branch) and serves all three nets; the action part is selected from four registers by
// unrolled compares on k - S (a run-time index into a register array would go to scratch).  Those four registers are the actor
// epilogue's a' in sac_target -- every lane group holds the same bits there -- and four loads from the action buffer in q_values,
// so both forms feed the critics' first layer the same operands in the same order: sac_target's q1 / q2 are q_values' bit for bit.
// Two critics without an actor are the same wave loop run over nets 1..2 (`first` = 1): qmin needs no exchange and no atomics.
//
// The ring runs across the nets: the prefetch cursor is (net, layer, block) and wraps actor -> Q1 -> Q2 -> actor, skipping a net
// with one hidden layer (it has no H x H layer, so no ring block).  The prefetches issued in the last round point at the first
// blocks of the same nets' weights again; the vmcnt(0) at the kernel's end lets them land before the workgroup's LDS goes away.
//
// The staged tables (first layer in operand order, zero-padded to K4 = ceil(K / 4) steps; hidden biases; head rows and bias) of ALL
// nets of the launch are RESIDENT beside the ring, staged once per workgroup behind the ring's first DMAs.  Staging per net phase
// would need two more workgroup barriers per net and round and would put each net's table loads in front of its first product;
// the first layer through the ring would need 16-byte aligned rows, which rows of S + A floats are not.  LDS, with NT = H / 16:
//   ring 3 NT KiB  +  per net: NT K4 256 B (first layer) + nh H 4 B (biases) + O H 4 B (head) + 32 B (head bias)
//   20-256-256-8 actor with 24-256-256-1 twins (QuadPole):  48 + (20 + 2 + 8) + 2 (24 + 2 + 1) KiB + 96 B = 132 KiB + 96 B
//   5-128-128-2 with 6-128-128-1 twins (the SAC tool on CartPole):  24 + (4 + 1 + 1) + 2 (4 + 1 + 0.5) KiB + 96 B = 41 KiB + 96 B
//   the largest first layers at H = 256, 28 + 4 inputs, two hidden layers each: 48 + (28 + 2 + 8) + 2 (32 + 2 + 1) = 156 KiB: taken;
//   with five hidden layers each it is 165 KiB: refused by the entry with its figures (pq_plan).
// Above 80 KiB one workgroup fits a CU, so the grid is then one workgroup per CU instead of two: the tables are staged once
// for twice the rounds.  One kernel per width (the nets of a launch share it): the 256-wide body needs the register file of one
// wave per SIMD, the narrower ones keep two workgroups per CU.
#include <stdlib.h>

#include "tg_common.hpp"
#include "policy_tile.hpp"

namespace tg {

constexpr int kPqNets = 3;                              // [0] the actor, [1] Q1, [2] Q2

struct PqNet {
    const float* w[kPolicyLinear];
    const float* b[kPolicyLinear];
    int32_t K, nh, O;                                   // input width (the actor: S, a critic: S + A), hidden layers, head outputs
    int32_t tab;                                        // where the net's tables start behind the ring, in floats
};

struct PqArgs {
    PqNet net[kPqNets];
    int32_t first, last;            // the nets a wave runs, in order: 0..2 sac_target, 1..1 or 1..2 q_values
    int32_t H, act;                 // shared by the nets of a launch
    int32_t S, A;
    const float* obs;               // [rows][S], unpadded
    const float* act_in;            // q_values: [rows][A]
    int64_t rows;
    uint32_t* calls;                // sac_target from here on: [rows]
    uint64_t seed;
    int64_t env_offset;
    float ls_lo, ls_hi;
    const float* reward; const float* discount; const float* alpha;
    float* action; float* logp; float* y;
    float* q1; float* q2; float* qmin;
};

// A field of net n / layer l's pointers of net n.  A run-time index into a local copy of the tables puts it into scratch, and
// uniform selects over the 36 pointer arguments keep all of them in scalar registers: the tables are read where the launch put
// them, in the kernel-argument segment, by scalar loads at a workgroup-uniform index (n and l are workgroup-uniform).
typedef const __attribute__((address_space(4))) PqNet* PqNetTable;
static_assert(offsetof(PqArgs, net) == 0, "the net tables lead the kernel arguments");
__device__ static inline PqNetTable pq_nets() { return (PqNetTable)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr(); }
#define PQ_NET(a, n, field) (pq_nets()[n].field)
__device__ static inline const float* pq_weight(const PqArgs& a, int n, int l) { return pq_nets()[n].w[l]; }
__device__ static inline const float* pq_bias(const PqArgs& a, int n, int l) { return pq_nets()[n].b[l]; }

template <int H, int kAct>
__device__ __attribute__((always_inline)) static inline void pq_forward(const PqArgs& a, uint4* lds) {
    constexpr int NT = H / 16, KS = NT, WPW = kTileWaves, D = kTileD, P = kTileP, SLOT = KS * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int first = a.first, last = a.last, S = a.S, A = a.A;
    const bool sac = first == 0, twin = last == 2;
    uint4* ring = lds;
    float* tables = reinterpret_cast<float*>(ring + D * SLOT);
    const int64_t rows = a.rows;
    const int64_t n_rounds = (rows + 63) / 64;

    // ---- the ring: block (n, l, mo) = output features 16 mo .. + 15 of H x H layer l of net n, straight out of its W_l ----
    const int hh0 = a.net[0].nh - 1, hh1 = a.net[1].nh - 1, hh2 = a.net[2].nh - 1;          // (a net the launch does not run: 0)
    auto ring_layers = [&](int n) { return n == 0 ? hh0 : (n == 1 ? hh1 : hh2); };
    auto after = [&](int n) { return n == last ? first : n + 1; };
    // the first net with ring blocks at or behind n, cyclically over first..last (the caller knows that there is one)
    auto ring_net = [&](int n) {
        const int n1 = after(n), n2 = after(n1);
        return ring_layers(n) > 0 ? n : (ring_layers(n1) > 0 ? n1 : n2);
    };
    bool any_ring = false;
    for (int n = first; n <= last; ++n) any_ring = any_ring || ring_layers(n) > 0;
    int pre_n = any_ring ? ring_net(first) : first, pre_l = 1, pre_mo = 0, pre_slot = 0, cur_slot = 0;
    auto dma_next = [&]() {
        const float* src = pq_weight(a, pre_n, pre_l) + ((16 * pre_mo + j) * H + 4 * g);
        uint4* slot = ring + pre_slot * SLOT;
#pragma unroll
        for (int q = 0; q < KS / WPW; ++q) {
            const int piece = q * WPW + wave;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint4*>(src + 16 * piece), (lds_void*)(slot + piece * 64), 16, 0, 0);
        }
        pre_mo = (pre_mo + 1 == NT) ? 0 : pre_mo + 1;
        const bool hop = pre_mo == 0 && pre_l == ring_layers(pre_n);  // (selects, not branches: the block loops are unrolled around this)
        pre_l = hop ? 1 : (pre_mo == 0 ? pre_l + 1 : pre_l);
        pre_n = hop ? ring_net(after(pre_n)) : pre_n;
        pre_slot = (pre_slot + 1 == D) ? 0 : pre_slot + 1;
    };
    if (any_ring) {
#pragma unroll
        for (int b = 0; b < P; ++b) dma_next();
    }
    // ---- staged once per workgroup, per net: the first layer in operand order, zero-padded to K4 steps; the biases; the head ----
    for (int n = first; n <= last; ++n) {
        const int K = PQ_NET(a, n, K), nh = PQ_NET(a, n, nh), O = PQ_NET(a, n, O), K4 = (K + 3) >> 2;
        float* w0_s = tables + PQ_NET(a, n, tab);                     // [NT][K4][64 lanes]: lane (i, g) of step s holds W0[16 mo + i][4 s + g]
        float* bias_s = w0_s + NT * K4 * 64;                          // [nh][H]
        float* wh_s = bias_s + nh * H;                                // [O][H]
        float* bh_s = wh_s + O * H;                                   // [8]
        const float* w0 = pq_weight(a, n, 0);
        for (int q = tid; q < NT * K4 * 64; q += 64 * WPW) {
            const int ln = q & 63, ps = q >> 6, mo = ps / K4, s = ps - mo * K4;
            const int k = 4 * s + (ln >> 4);
            const bool in = k < K;
            const float v = w0[(16 * mo + (ln & 15)) * K + (in ? k : 0)];
            w0_s[q] = in ? v : 0.f;
        }
        for (int l = 0; l < nh; ++l) {
            const float* bl = pq_bias(a, n, l);
            for (int q = tid; q < H; q += 64 * WPW) bias_s[l * H + q] = bl[q];
        }
        const float* Wh = pq_weight(a, n, nh);
        const float* Bh = pq_bias(a, n, nh);
        for (int q = tid; q < O * H; q += 64 * WPW) wh_s[q] = Wh[q];
        const float bv = Bh[tid < O ? tid : 0];
        if (tid < kTileHeadBias) bh_s[tid] = tid < O ? bv : 0.f;
    }
    __syncthreads();                                                  // (the tables; drains the prologue's DMA too: once)
    // counted wait for the block about to be consumed: behind its DMA there are always the pieces of the P - 1 later blocks.  The
    // input loads and output stores of a round are issued behind them too and are NOT counted: stricter, never weaker.
    constexpr int kWait = (P - 1) * (KS / WPW);

    auto act4 = [&](f32x4& v) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = act_f32<kAct>(v[r]);
    };
    // one 16-feature output tile against a whole H-wide operand (policy_tile.hpp's tile_products)
    auto tile_products = [&](const uint4* __restrict__ cur, const f32x4 (&xin)[NT], f32x4 acc) {
        const uint4* __restrict__ p = cur + lane;
        f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
        uint4 wa = lds_u4(p), wb = lds_u4(p + 64);
        dma_next();
#pragma unroll
        for (int t = 0; t < NT; t += 2) {
            uint4 na = wa, nb = wb;
            if (t + 2 < NT) { na = lds_u4(p + (t + 2) * 64); nb = lds_u4(p + (t + 3) * 64); }
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
        const bool store = valid && g == 0;

        // ---- the observation part of every net's input row: lane group g holds obs[4 s + g] for the steps s (no load under a
        //      divergent branch); the action part: four registers, a' of the actor's epilogue below or the caller's rows ----
        float xo[kTileMaxIn / 4];
#pragma unroll
        for (int s = 0; s < kTileMaxIn / 4; ++s) {
            const int k = 4 * s + g;
            const bool in = k < S;
            const float v = a.obs[rowc * S + (in ? k : 0)];
            xo[s] = in ? v : 0.f;
        }
        float ak[4] = {0.f, 0.f, 0.f, 0.f};
        if (!sac) {                                                   // (workgroup-uniform)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = k < A;
                const float v = a.act_in[rowc * A + (in ? k : 0)];
                ak[k] = in ? v : 0.f;
            }
        }
        float logp = 0.f, q1v = 0.f, q2v = 0.f;
        uint32_t calls = 0;

        for (int n = first; n <= last; ++n) {
            const int nh = PQ_NET(a, n, nh), O = PQ_NET(a, n, O), K4 = (PQ_NET(a, n, K) + 3) >> 2, n_hh = nh - 1;
            const float* w0_s = tables + PQ_NET(a, n, tab);
            const float* bias_s = w0_s + NT * K4 * 64;
            const float* wh_s = bias_s + nh * H;
            const float* bh_s = wh_s + O * H;
            f32x4 xin[NT], xout[NT];

            // ---- layer 0: input k = 4 s + g is obs[k] below S and action k - S behind it (zero while the actor runs, and past A) ----
            float xr[kTileMaxIn / 4];
#pragma unroll
            for (int s = 0; s < kTileMaxIn / 4; ++s) {
                const int ka = 4 * s + g - S;
                const float av = ka == 0 ? ak[0] : (ka == 1 ? ak[1] : (ka == 2 ? ak[2] : (ka == 3 ? ak[3] : 0.f)));
                xr[s] = ka < 0 ? xo[s] : av;
            }
#pragma unroll
            for (int mo = 0; mo < NT; ++mo) {
                const float4 b4 = lds_f4(bias_s + 16 * mo + 4 * g);
                f32x4 acc = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int s = 0; s < kTileMaxIn / 4; ++s)
                    if (s < K4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(lds_f(w0_s + (mo * K4 + s) * 64 + lane), xr[s], acc, 0, 0, 0);
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
                    const float4 b4 = lds_f4(bias_l + 16 * mo);
                    f32x4 acc = tile_products(cur, xin, f32x4{b4.x, b4.y, b4.z, b4.w});
                    act4(acc);
                    xout[mo] = acc;
                }
#pragma unroll
                for (int t = 0; t < NT; ++t) xin[t] = xout[t];
            }
            // ---- head: fp32 dot products over the lane's features, the four lane groups added in a fixed order ----
            auto head_out = [&](int k) {
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float4 w = lds_f4(wh_s + k * H + 16 * t + 4 * g);
                    s = fmaf(xin[t][0], w.x, s);
                    s = fmaf(xin[t][1], w.y, s);
                    s = fmaf(xin[t][2], w.z, s);
                    s = fmaf(xin[t][3], w.w, s);
                }
                // (g0 + g1) + (g2 + g3): every lane group ends up with the same bits
                const float p1 = __shfl_xor(s, 16, 64);
                const float pair = (g & 1) ? p1 + s : s + p1;
                const float p2 = __shfl_xor(pair, 32, 64);
                return ((g & 2) ? p2 + pair : pair + p2) + lds_f(bh_s + k);
            };
            if (n != 0) {
                const float qv = head_out(0);
                q1v = n == 1 ? qv : q1v;
                q2v = n == 2 ? qv : q2v;
                continue;
            }
            // ---- the actor's epilogue, per row: tg_policy_step's squashed head; a' and logp stay in registers ----
            float mu_k[4] = {0.f, 0.f, 0.f, 0.f}, ls_k[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < A) {
                    mu_k[k] = head_out(k);
                    ls_k[k] = head_out(A + k);
                }
            }
            calls = a.calls[rowc];
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
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < A) {
                    const float e = eps[k];
                    const float ls = fminf(fmaxf(ls_k[k], a.ls_lo), a.ls_hi);
                    const float u = rn_add(mu_k[k], rn_mul(expf(ls), e));
                    float lp = rn_sub(rn_sub(rn_mul(-0.5f, rn_mul(e, e)), ls), 0.91893853320467274f);
                    const float act = tanhf(u);
                    lp = rn_sub(lp, logf(rn_add(rn_sub(1.0f, rn_mul(act, act)), 1e-6f)));
                    logp = rn_add(logp, lp);
                    ak[k] = act;
                }
            }
        }
        // ---- the round's stores, lane group 0 of a valid row ----
        if (sac) {
            const float y = rn_add(a.reward[rowc], rn_mul(a.discount[rowc], rn_sub(fminf(q1v, q2v), rn_mul(a.alpha[0], logp))));
            if (store) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < A) a.action[row * A + k] = ak[k];
                a.logp[row] = logp;
                a.calls[row] = calls + 1u;
                a.y[row] = y;
            }
        }
        if (store) {
            a.q1[row] = q1v;
            if (twin) {
                a.q2[row] = q2v;
                a.qmin[row] = fminf(q1v, q2v);
            }
        }
    }
    // the ring's prefetches of a round that never came: let them land before the workgroup's LDS goes away
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One kernel per width (the nets of a launch share it), the activation behind a workgroup-uniform switch.  The 256-wide body keeps
// two 64-register activation sets and what passes between the nets: it is given the register file of one wave per SIMD, which is
// all its LDS leaves room for at QuadPole's shapes anyway; the narrower bodies keep two workgroups per CU.
template <int H>
__global__ __launch_bounds__(64 * kTileWaves, H == 256 ? 1 : 2) void policy_q_kernel(PqArgs a) {
    extern __shared__ uint4 lds[];
    if (a.act == TG_ACT_TANH) pq_forward<H, TG_ACT_TANH>(a, lds); else pq_forward<H, TG_ACT_RELU>(a, lds);
}

// the shared verdict on one net, in this file's table form; `pointers`: the launches (tg_policy_q_fits reads the widths alone)
static int pq_fill_net(const char* who, const char* name, const tg_policy_net* n, int outs, bool pointers, PqNet& out, int& H_out, int& act_out) {
    PolicyNet c = {};
    if (int rc = policy_net_check(who, name, n, outs, pointers, c)) return rc;
    for (int l = 0; l < kPolicyLinear; ++l) { out.w[l] = c.w[l]; out.b[l] = c.b[l]; }
    out.K = c.S; out.nh = c.nh; out.O = c.O;
    H_out = c.H; act_out = c.act;
    return TG_OK;
}

// The nets of a launch (actor may be null: q_values; q2 may be null without an actor), what they must share, where their tables go
// and whether all of it fits: the one place that knows the LDS arithmetic of the header comment.
static int pq_plan(const char* who, const tg_policy_net* actor, const tg_policy_net* q1, const tg_policy_net* q2, int obs_dim, int act_dim,
                   bool pointers, PqArgs& args, size_t& shmem) {
    TG_REQUIRE(act_dim >= 1 && act_dim <= 4, "%s: act_dim=%d outside [1, 4]", who, act_dim);
    TG_REQUIRE(actor == nullptr || q2 != nullptr, "%s: the target needs both critics", who);
    const tg_policy_net* nets[kPqNets] = {actor, q1, q2};
    const char* names[kPqNets] = {"the actor", "Q1", "Q2"};
    int H[kPqNets] = {}, act[kPqNets] = {};
    args.first = actor ? 0 : 1;
    args.last = q2 ? 2 : 1;
    for (int n = args.first; n <= args.last; ++n)
        if (int rc = pq_fill_net(who, names[n], nets[n], n == 0 ? 2 * act_dim : 1, pointers, args.net[n], H[n], act[n])) return rc;
    const int f = args.first;
    for (int n = f + 1; n <= args.last; ++n)
        TG_REQUIRE(H[n] == H[f] && act[n] == act[f], "%s: %s is %d wide with activation %d, %s %d wide with %d: one kernel body runs "
                   "all nets of a launch", who, names[n], H[n], act[n], names[f], H[f], act[f]);
    if (actor) obs_dim = args.net[0].K;
    TG_REQUIRE(obs_dim >= 1 && obs_dim + act_dim <= kTileMaxIn, "%s: %d observations + %d actions outside [2, %d]", who, obs_dim, act_dim,
               kTileMaxIn);
    for (int n = 1; n <= args.last; ++n)
        TG_REQUIRE(args.net[n].K == obs_dim + act_dim, "%s: %s reads %d inputs, not %d observations + %d actions", who, names[n],
                   args.net[n].K, obs_dim, act_dim);
    args.H = H[f]; args.act = act[f]; args.S = obs_dim; args.A = act_dim;
    const int NT = args.H / 16;
    size_t floats = 0;
    for (int n = 0; n < kPqNets; ++n) {
        if (n < args.first || n > args.last) {                        // (never run: valid pointers, no ring block)
            args.net[n] = args.net[1];
            args.net[n].nh = 1;
            continue;
        }
        args.net[n].tab = (int32_t)floats;
        floats += (size_t)NT * ((args.net[n].K + 3) / 4) * 64 + (size_t)(args.net[n].nh + args.net[n].O) * args.H + kTileHeadBias;
    }
    shmem = (size_t)kTileD * NT * 1024 + floats * 4;
    TG_REQUIRE(shmem <= 160 * 1024, "%s: the ring (%d B) and the resident tables of %d nets (%zu B) need %zu B of LDS (> 160 KiB): "
               "fewer hidden layers or inputs, or a narrower width", who, kTileD * NT * 1024, args.last - args.first + 1, floats * 4, shmem);
    return TG_OK;
}

static int pq_launch(const char* who, PqArgs& args, size_t shmem, int32_t grid_limit, hipStream_t st) {
    static LdsOptIn opt_in[3];
    void (*const kernels[3])(PqArgs) = {policy_q_kernel<64>, policy_q_kernel<128>, policy_q_kernel<256>};
    const int v = args.H == 64 ? 0 : (args.H == 128 ? 1 : 2);
    return launch_row_tiles(who, kernels[v], opt_in[v], args, 1, shmem, grid_limit, (v == 2 || shmem > 80 * 1024) ? 1 : 2, st);
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_policy_q_fits(const tg_policy_net* actor, const tg_policy_net* q1, const tg_policy_net* q2, int32_t act_dim) {
    const char* who = "tg_policy_q_fits";
    PqArgs args = {};
    size_t shmem = 0;
    TG_REQUIRE(q1 != nullptr, "%s: the Q1 table is null", who);
    return pq_plan(who, actor, q1, q2, q1->in_dim[0] - act_dim, act_dim, false, args, shmem);
}

int tg_policy_q_values(const tg_policy_net* q1, const tg_policy_net* q2, const tg_policy_q_args* s, void* stream) {
    const char* who = "tg_policy_q_values";
    TG_REQUIRE(s != nullptr, "%s: null arguments", who);
    PqArgs args = {};
    size_t shmem = 0;
    if (int rc = pq_plan(who, nullptr, q1, q2, s->obs_dim, s->act_dim, true, args, shmem)) return rc;
    TG_REQUIRE(s->n > 0 && s->n < ((int64_t)1 << 31), "%s: n=%lld outside [1, 2^31)", who, (long long)s->n);
    TG_REQUIRE(s->d_obs && s->d_act && s->d_q1 && (q2 == nullptr || (s->d_q2 && s->d_qmin)), "%s: null pointer", who);
    args.obs = s->d_obs; args.act_in = s->d_act; args.rows = s->n;
    args.q1 = s->d_q1; args.q2 = s->d_q2; args.qmin = s->d_qmin;
    return pq_launch(who, args, shmem, s->grid_limit, (hipStream_t)stream);
}

int tg_policy_sac_target(const tg_policy_net* actor, const tg_policy_net* q1, const tg_policy_net* q2, const tg_policy_q_args* s,
                         void* stream) {
    const char* who = "tg_policy_sac_target";
    TG_REQUIRE(s != nullptr, "%s: null arguments", who);
    TG_REQUIRE(actor != nullptr, "%s: the actor table is null", who);
    PqArgs args = {};
    size_t shmem = 0;
    if (int rc = pq_plan(who, actor, q1, q2, s->obs_dim, s->act_dim, true, args, shmem)) return rc;
    TG_REQUIRE(s->obs_dim == args.S, "%s: obs_dim=%d, the actor reads %d inputs", who, s->obs_dim, args.S);
    TG_REQUIRE(s->n > 0 && s->n < ((int64_t)1 << 31) && s->env_offset >= 0, "%s: n=%lld outside [1, 2^31) or a negative env_offset", who,
               (long long)s->n);
    TG_REQUIRE(s->d_obs && s->d_reward && s->d_discount && s->d_alpha && s->d_calls && s->d_action && s->d_logp && s->d_y && s->d_q1 &&
               s->d_q2 && s->d_qmin, "%s: null pointer", who);
    TG_REQUIRE(s->log_std_lo <= s->log_std_hi, "%s: log_std bounds [%g, %g] are empty", who, (double)s->log_std_lo, (double)s->log_std_hi);
    args.obs = s->d_obs; args.rows = s->n;
    args.calls = s->d_calls; args.seed = s->seed; args.env_offset = s->env_offset;
    args.ls_lo = s->log_std_lo; args.ls_hi = s->log_std_hi;
    args.reward = s->d_reward; args.discount = s->d_discount; args.alpha = s->d_alpha;
    args.action = s->d_action; args.logp = s->d_logp; args.y = s->d_y;
    args.q1 = s->d_q1; args.q2 = s->d_q2; args.qmin = s->d_qmin;
    return pq_launch(who, args, shmem, s->grid_limit, (hipStream_t)stream);
}

}  // extern "C"
