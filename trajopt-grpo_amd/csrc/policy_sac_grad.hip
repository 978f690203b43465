// SAC's two gradient steps on DeviceActor (DeviceActor.rsample / .q_evaluate, trajopt-grpo_amd/policy_step.py): the reparameterised draw of
// the squashed head and the Q critics on [obs, action] rows, each forward AND backward in float32 on v_mfma_f32_16x16x4_f32, against
// torch's own row-major `nn.Linear` storage.  Four row-tile kernels and the head-gradient pair of this file, and policy_grad.hip's weight-gradient pair behind them:
//
//   tg_policy_q_eval_forward    policy_tile.hpp's forward, a wave owns 16 rows, the critic (Q1 / Q2) as grid dimension y.  The first
//                               layer's input is policy_q.hip's gather: lane group g of step s holds input k = 4 s + g, obs[k] below S
//                               and action k - S behind it, the action picked from four registers by unrolled compares.  Same operands
//                               in the same order: q1 / q2 are q_values()' bits.  Every hidden tile goes to acts[l][m][H] (one 16-byte
//                               store per lane and tile); Q1's workgroups also write the row [obs, act] once to xcat [m][S + A], so
//                               that the first layer's weight-gradient job has ONE row-major operand.
//   tg_policy_q_eval_backward   policy_bwd.hpp's backward data with O = 1, d_out = g_q.  New behind dZ_0: the action gradient
//                               g_act[row][k] = sum_o dZ_0[row][o] W_0[o][S + k].  The A action COLUMNS of W_0 are gathered once per
//                               workgroup into LDS as [A][H] rows behind the head row; lane (j, g) multiplies its NT x 4 dZ registers
//                               (features 16 t + 4 g + r of row j) against 16-byte LDS reads, and the four lane groups of a row are
//                               added by two cross-lane exchanges in the head's fixed order (g0 + g1) + (g2 + g3): no LDS round trip,
//                               no atomics.  Lane group 0 stores a zero-padded float4 per row into the critic's own [m][4] buffer; the
//                               node adds the two critics' buffers (one torch add: the same bits at every call).  Both critics back to
//                               back in one wave (policy_q.hip's form) was not built: it would halve the workgroups of a launch that
//                               at SAC's batch sizes has 4 to 16 per critic on 256 CUs.
//   tg_policy_rsample_forward   policy_step.hip's squashed-head forward and sampling, term by term (the same header routines: action
//                               and logp are act()'s bits), with the activation stores and, per row, what the backward needs:
//                               head_rows [m][8] = {inside_k ? exp(ls_k) eps_k : 0} x 4, {inside_k} x 4, where inside_k says that the
//                               pre-clamp log-std lies on the closed interval [lo, hi] (torch's clamp derivative); eps goes to the
//                               caller's [m][A] buffer; the tanh'd action is the node's own output.
//   tg_policy_rsample_backward  the head gradient per row on the vector unit, with s = 1 - a^2:
//                                   d_mu_k = g_a_k s + g_logp 2 a s / (s + 1e-6)            (eps is a constant of the node)
//                                   d_ls_k = d_mu_k exp(ls_k) eps_k inside_k - g_logp inside_k
//                               as d_out rows [m][8] = (d_mu_0.., d_ls_0.., zeros), then the shared body with 8 head outputs.
//   tg_policy_sac_weight_grad   policy_grad.hip's 64 x 64-tile / row-slab kernel and its fixed-order finishing pass over the first and
//                               hidden layers of this file's nets (a critic's first layer on xcat through the scalar staging path:
//                               S + A is no multiple of 4 in general), and the head layers -- <= 8 rows each, sums of cancelling
//                               terms over the whole batch -- on the vector unit in float64 (section 5).
//
// Actor and critics are NOT fused into one launch: the two nodes compose (SAC's critic step is q_evaluate alone, its actor step is
// rsample -> q_evaluate(detach_params)), and a deterministic-policy-gradient step is q_evaluate's action gradient alone.
#include <stdlib.h>

#include "tg_common.hpp"
#include "policy_tile.hpp"
#include "policy_bwd.hpp"

namespace tg {

constexpr int kSgActorOut = 8;                          // the squashed head: (mu, ls) pairs of <= 4 actions
constexpr int kSgQOut = 4;                              // a critic's d_out row: 1 value, zero-padded to 16 bytes

struct SgArgs {
    PolicyNet net[2];               // q_evaluate: Q1, Q2 (S = obs + act inputs); rsample: the actor
    int32_t S, A;                   // observations, actions
    const float* obs;               // [rows][S], unpadded
    const float* act;               // q_evaluate: [rows][A]
    int64_t rows;
    float* xcat;                    // q_evaluate: [rows][S + A]
    float* q[2];                    // [rows] per critic
    float* acts[2];                 // [nh][rows][H] per net
    float* dz[2];                   // [nh][rows][H] per net
    float* dout[2];                 // [rows][4] per critic; the actor: [rows][8]
    const float* g_q[2];
    float* g_act;                   // [2][rows][4], zero-padded; null: not built
    uint32_t* calls;                // rsample from here on: [rows]
    uint64_t seed;
    int64_t env_offset;
    float ls_lo, ls_hi;
    float* action; float* logp; float* eps; float* head_rows;
    const float* g_action; const float* g_logp;
};

// ---- 1. Q forward with stores: policy_tile.hpp's forward_tiles under the [obs, act] gather ---------------------------------------------
template <int H, int kAct>
__device__ __attribute__((always_inline)) static inline void sg_q_forward(const SgArgs& a, const int nh, const bool second, uint4* lds) {
    constexpr int NT = H / 16;
    const int g = (threadIdx.x & 63) >> 4;
    const int S = a.S, A = a.A, K = S + A;
    const int64_t rows = a.rows;
    float* acts = second ? a.acts[1] : a.acts[0];
    float* qout = second ? a.q[1] : a.q[0];
    // the input row: obs[k] below S (clamped address, selected value), the action behind it by unrolled compares on k - S
    auto inputs = [&](int64_t row, int64_t rowc, bool valid, float (&xr)[kTileMaxIn / 4]) {
        float ak[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = k < A;
            const float v = a.act[rowc * A + (in ? k : 0)];
            ak[k] = in ? v : 0.f;
        }
#pragma unroll
        for (int s = 0; s < kTileMaxIn / 4; ++s) {
            const int k = 4 * s + g, ka = k - S;
            const bool in = k < S;
            const float v = a.obs[rowc * S + (in ? k : 0)];
            const float av = ka == 0 ? ak[0] : (ka == 1 ? ak[1] : (ka == 2 ? ak[2] : (ka == 3 ? ak[3] : 0.f)));
            xr[s] = in ? v : av;
            if (!second && valid && k < K) a.xcat[row * K + k] = xr[s];
        }
    };
    // the lane's 16 bytes of layer l's tile mo: features 16 mo + 4 g .. + 3 of its row
    auto store_act = [&](int64_t row, bool valid, int l, int mo, const f32x4& v) {
        if (valid) *reinterpret_cast<float4*>(acts + ((int64_t)l * rows + row) * H + 16 * mo + 4 * g) = float4{v[0], v[1], v[2], v[3]};
    };
    auto head = [&](int64_t row, int64_t, bool valid, const f32x4 (&xin)[NT], const NetTables<H>& tb) {
        const float qv = head_out<NT>(tb.wh, tb.bh, xin, 0, g);
        if (valid && g == 0) qout[row] = qv;
    };
    forward_tiles<H, kAct>(a, second, K, nh, 1, lds, inputs, store_act, head);
}

// ---- 2. Q backward data with the action gradient -------------------------------------------------------------------------------------
template <int H, int kAct>
__device__ __attribute__((always_inline)) static inline void sg_q_backward(const SgArgs& a, const int nh, const bool second, uint4* lds) {
    constexpr int NT = H / 16;
    const int tid = threadIdx.x, g = (tid & 63) >> 4;
    const int S = a.S, A = a.A, K = S + A;
    const bool with_act = a.g_act != nullptr;                         // (workgroup-uniform)
    float* wa_s = bwd_lds_extra<H>(lds, 1);                           // [A][H]: W_0[o][S + k] at k H + o
    if (with_act) {
        const float* W0 = net_weight(a, second, 0);
        for (int q = tid; q < A * H; q += 64 * kTileWaves) {
            const int k = q / H, o = q - k * H;
            wa_s[q] = W0[o * K + S + k];
        }
    }                                                                 // (backward_tiles' barrier stands between this and the reads)
    const float* gq = second ? a.g_q[1] : a.g_q[0];
    float* doutb = second ? a.dout[1] : a.dout[0];
    float* gact = a.g_act + (second ? a.rows * 4 : 0);
    auto head_grad = [&](int64_t row, int64_t rowc, bool store, float (&d_out)[kSgQOut]) {
        d_out[0] = gq[rowc];
        d_out[1] = d_out[2] = d_out[3] = 0.f;
        if (store) *reinterpret_cast<float4*>(doutb + row * 4) = float4{d_out[0], 0.f, 0.f, 0.f};
    };
    auto action_grad = [&](const f32x4 (&dz)[NT], int64_t row, bool valid) {
        if (!with_act) return;
        float ga[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < A) {
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float4 w = lds_f4(wa_s + k * H + 16 * t + 4 * g);
                    s = fmaf(dz[t][0], w.x, s);
                    s = fmaf(dz[t][1], w.y, s);
                    s = fmaf(dz[t][2], w.z, s);
                    s = fmaf(dz[t][3], w.w, s);
                }
                // (g0 + g1) + (g2 + g3): every lane group ends up with the same bits
                const float p1 = __shfl_xor(s, 16, 64);
                const float pair = (g & 1) ? p1 + s : s + p1;
                const float p2 = __shfl_xor(pair, 32, 64);
                ga[k] = (g & 2) ? p2 + pair : pair + p2;
            }
        }
        if (valid && g == 0) *reinterpret_cast<float4*>(gact + row * 4) = float4{ga[0], ga[1], ga[2], ga[3]};
    };
    backward_tiles<H, kAct, kSgQOut>(a, second, nh, 1, second ? a.acts[1] : a.acts[0], second ? a.dz[1] : a.dz[0], lds, head_grad,
                                     action_grad);
}

// ---- 3. rsample forward: policy_step.hip's squashed head, with what the backward needs -----------------------------------------------
template <int H, int kAct>
__device__ __attribute__((always_inline)) static inline void sg_rsample_forward(const SgArgs& a, const int nh, const int O, uint4* lds) {
    constexpr int NT = H / 16;
    const int g = (threadIdx.x & 63) >> 4;
    const int S = a.S, A = a.A;
    const int64_t rows = a.rows;
    auto inputs = [&](int64_t, int64_t rowc, bool, float (&xr)[kTileMaxIn / 4]) {
#pragma unroll
        for (int s = 0; s < kTileMaxIn / 4; ++s) {
            const int k = 4 * s + g;
            const bool in = k < S;
            const float v = a.obs[rowc * S + (in ? k : 0)];
            xr[s] = in ? v : 0.f;
        }
    };
    auto store_act = [&](int64_t row, bool valid, int l, int mo, const f32x4& v) {
        if (valid) *reinterpret_cast<float4*>(a.acts[0] + ((int64_t)l * rows + row) * H + 16 * mo + 4 * g) = float4{v[0], v[1], v[2], v[3]};
    };
    auto head = [&](int64_t row, int64_t rowc, bool valid, const f32x4 (&xin)[NT], const NetTables<H>& tb) {
        const bool store = valid && g == 0;
        // ---- tg_policy_step's epilogue, term by term ----
        const uint32_t calls = a.calls[rowc];
        uint32_t rnd[4];
        Philox::draw(a.seed, (uint64_t)(a.env_offset + rowc), calls, TG_POLICY_STEP_STREAM, rnd);
        float eps[4];
        box_muller_eps(rnd, A, eps);
        float logp = 0.f;
        float4 se = {0.f, 0.f, 0.f, 0.f}, inside = {0.f, 0.f, 0.f, 0.f};
        auto one = [&](const int k, float& se_k, float& inside_k) {
            if (k < A) {
                const float mu = head_out<NT>(tb.wh, tb.bh, xin, k, g), raw = head_out<NT>(tb.wh, tb.bh, xin, A + k, g);
                const float e = eps[k];
                const float ls = fminf(fmaxf(raw, a.ls_lo), a.ls_hi);
                const float sd_e = rn_mul(expf(ls), e);
                const float act = tanhf(rn_add(mu, sd_e));
                logp = rn_add(logp, rn_sub(gaussian_logp_term(e, ls), squash_logp_term(act)));
                const bool in = raw >= a.ls_lo && raw <= a.ls_hi;
                se_k = in ? sd_e : 0.f;
                inside_k = in ? 1.f : 0.f;
                if (store) {
                    a.action[row * A + k] = act;
                    a.eps[row * A + k] = e;
                }
            }
        };
        one(0, se.x, inside.x);
        one(1, se.y, inside.y);
        one(2, se.z, inside.z);
        one(3, se.w, inside.w);
        if (store) {
            a.logp[row] = logp;
            a.calls[row] = calls + 1u;
            *reinterpret_cast<float4*>(a.head_rows + row * 8) = se;
            *reinterpret_cast<float4*>(a.head_rows + row * 8 + 4) = inside;
        }
    };
    forward_tiles<H, kAct>(a, false, S, nh, O, lds, inputs, store_act, head);
}

// ---- 4. rsample backward: the squashed head's gradient, then the shared body with 8 head outputs -------------------------------------
template <int H, int kAct>
__device__ __attribute__((always_inline)) static inline void sg_rsample_backward(const SgArgs& a, const int nh, const int O, uint4* lds) {
    const int A = a.A;
    auto head_grad = [&](int64_t row, int64_t rowc, bool store, float (&d_out)[kSgActorOut]) {
        const float gl = a.g_logp[rowc];
        const float4 h0 = *reinterpret_cast<const float4*>(a.head_rows + rowc * 8);
        const float4 h1 = *reinterpret_cast<const float4*>(a.head_rows + rowc * 8 + 4);
        const float se[4] = {h0.x, h0.y, h0.z, h0.w}, in[4] = {h1.x, h1.y, h1.z, h1.w};
        float d_mu[4] = {0.f, 0.f, 0.f, 0.f}, d_ls[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < A) {
                const float av = a.action[rowc * A + k], ga = a.g_action[rowc * A + k];
                const float s = fmaf(-av, av, 1.0f);
                d_mu[k] = fmaf(ga, s, gl * (2.0f * av * s / (s + 1e-6f)));
                d_ls[k] = fmaf(d_mu[k], se[k], -in[k] * gl);
            }
        }
        // rows (mu_0 .. mu_{A-1}, ls_0 .. ls_{A-1}, zeros): unrolled compares on q - A, no run-time register index
#pragma unroll
        for (int q = 0; q < kSgActorOut; ++q) {
            const int ka = q - A;
            const float lsv = ka == 0 ? d_ls[0] : (ka == 1 ? d_ls[1] : (ka == 2 ? d_ls[2] : (ka == 3 ? d_ls[3] : 0.f)));
            d_out[q] = (q < 4 && q < A) ? d_mu[q < 4 ? q : 0] : lsv;
        }
        if (store) {
            *reinterpret_cast<float4*>(a.dout[0] + row * 8) = float4{d_out[0], d_out[1], d_out[2], d_out[3]};
            *reinterpret_cast<float4*>(a.dout[0] + row * 8 + 4) = float4{d_out[4], d_out[5], d_out[6], d_out[7]};
        }
    };
    backward_tiles<H, kAct, kSgActorOut>(a, false, nh, O, a.acts[0], a.dz[0], lds, head_grad, [](const f32x4 (&)[H / 16], int64_t, bool) {});
}

// One kernel per pass; the six (H, activation) bodies behind a workgroup-uniform switch (policy_step.hip's form).
#define SG_NET_FIELDS(second)                                                                                                          \
    const int H = second ? a.net[1].H : a.net[0].H, nh = second ? a.net[1].nh : a.net[0].nh, O = second ? a.net[1].O : a.net[0].O,     \
              act = second ? a.net[1].act : a.net[0].act;

__global__ __launch_bounds__(64 * kTileWaves, 2) void policy_q_eval_forward_kernel(SgArgs a) {
    extern __shared__ uint4 lds[];
    const bool second = __builtin_amdgcn_readfirstlane((int)blockIdx.y) == 1;
    SG_NET_FIELDS(second)
    dispatch_width_act(H, act, [&](auto h, auto k) __attribute__((always_inline)) {
        sg_q_forward<decltype(h)::value, decltype(k)::value>(a, nh, second, lds);
    });
}

__global__ __launch_bounds__(64 * kTileWaves, 2) void policy_q_eval_backward_kernel(SgArgs a) {
    extern __shared__ uint4 lds[];
    const bool second = __builtin_amdgcn_readfirstlane((int)blockIdx.y) == 1;
    SG_NET_FIELDS(second)
    dispatch_width_act(H, act, [&](auto h, auto k) __attribute__((always_inline)) {
        sg_q_backward<decltype(h)::value, decltype(k)::value>(a, nh, second, lds);
    });
}

__global__ __launch_bounds__(64 * kTileWaves, 2) void policy_rsample_forward_kernel(SgArgs a) {
    extern __shared__ uint4 lds[];
    SG_NET_FIELDS(false)
    dispatch_width_act(H, act, [&](auto h, auto k) __attribute__((always_inline)) {
        sg_rsample_forward<decltype(h)::value, decltype(k)::value>(a, nh, O, lds);
    });
}

__global__ __launch_bounds__(64 * kTileWaves, 2) void policy_rsample_backward_kernel(SgArgs a) {
    extern __shared__ uint4 lds[];
    SG_NET_FIELDS(false)
    dispatch_width_act(H, act, [&](auto h, auto k) __attribute__((always_inline)) {
        sg_rsample_backward<decltype(h)::value, decltype(k)::value>(a, nh, O, lds);
    });
}

// ---- 5. the head layers' gradients, accumulated in float64 ---------------------------------------------------------------------------
// dW_head [O][H] = d_out^T A_top and db_head [O] = the column sums of d_out are sums over ALL rows of a batch of terms of both signs
// (the loss weights of a batch cancel), O <= 8 rows of them: a float32 accumulation in any fixed order leaves a few ulps of the
// largest PARTIAL sum, which can be ten times the result.  They are taken off the MFMA tile kernel (where a head was a zero-padded
// 64 x 64 tile) and added on the vector unit in float64 -- float x float is exact there -- thread c owning column c of A_top, one
// workgroup per net and row slab (policy_bwd.hpp's slabs), partials [slab][8][H + 1] added over the slabs in index order by the
// finishing kernel and rounded to float32 once.  No atomics, the same bits at every call.
struct SgHeadArgs {
    const float* dout[2];           // [rows][ld]
    const float* top[2];            // the top hidden layer's activations [rows][H]
    float* gw[2]; float* gb[2];     // [O][H], [O]
    double* part[2];                // [n_slabs][8][H + 1]
    int32_t ld[2], O[2], H[2];
    int32_t n_slabs;
    int64_t rows, slab_rows;
};

__global__ __launch_bounds__(256) void policy_sac_head_grad_kernel(SgHeadArgs a) {
    const bool second = blockIdx.x == 1;
    const int H = second ? a.H[1] : a.H[0], O = second ? a.O[1] : a.O[0], ld = second ? a.ld[1] : a.ld[0];
    const float* dout = second ? a.dout[1] : a.dout[0];
    const float* top = second ? a.top[1] : a.top[0];
    const int c = threadIdx.x, cc = c < H ? c : 0, slab = blockIdx.y;
    const int64_t r0 = (int64_t)slab * a.slab_rows, r1 = r0 + a.slab_rows < a.rows ? r0 + a.slab_rows : a.rows;
    double w[kSgActorOut], b[kSgActorOut];
#pragma unroll
    for (int k = 0; k < kSgActorOut; ++k) w[k] = b[k] = 0.0;
    for (int64_t row = r0; row < r1; ++row) {
        const double av = top[row * H + cc];
#pragma unroll
        for (int k = 0; k < kSgActorOut; ++k) {
            if (k < O) {
                const double dv = dout[row * ld + k];
                w[k] = fma(dv, av, w[k]);
                b[k] += dv;
            }
        }
    }
    double* p = (second ? a.part[1] : a.part[0]) + (int64_t)slab * kSgActorOut * (H + 1);
#pragma unroll
    for (int k = 0; k < kSgActorOut; ++k) {
        if (k < O) {
            if (c < H) p[k * (H + 1) + c] = w[k];
            if (c == 0) p[k * (H + 1) + H] = b[k];
        }
    }
}

__global__ __launch_bounds__(256) void policy_sac_head_grad_finish_kernel(SgHeadArgs a) {
    const bool second = blockIdx.x == 1;
    const int H = second ? a.H[1] : a.H[0], O = second ? a.O[1] : a.O[0];
    const double* part = second ? a.part[1] : a.part[0];
    float* gw = second ? a.gw[1] : a.gw[0];
    float* gb = second ? a.gb[1] : a.gb[0];
    const int c = threadIdx.x;
    if (c < H) {
        for (int k = 0; k < O; ++k) {
            double s = 0.0;
            for (int q = 0; q < a.n_slabs; ++q) s += part[((int64_t)q * kSgActorOut + k) * (H + 1) + c];
            gw[k * H + c] = (float)s;
        }
    }
    if (c < O) {                                                      // (column H of row c: the bias sum)
        double s = 0.0;
        for (int q = 0; q < a.n_slabs; ++q) s += part[((int64_t)q * kSgActorOut + c) * (H + 1) + H];
        gb[c] = (float)s;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// the shared verdict on a net and whether both of its passes fit; `extra`: floats behind the backward's head rows (a critic's
// action columns); `pointers`: the launches (the workspace entry reads widths)
static int sg_fill_net(const char* who, const char* name, const tg_policy_net* n, int outs, int extra, bool pointers, PolicyNet& out) {
    if (int rc = policy_net_check(who, name, n, outs, pointers, out)) return rc;
    const size_t fwd = ring_tables_lds_bytes(out), bwd = bwd_lds_bytes(out, extra);
    TG_REQUIRE(fwd <= 160 * 1024 && bwd <= 160 * 1024, "%s: %s needs %zu B (forward) / %zu B (backward) of LDS (> 160 KiB)", who, name, fwd, bwd);
    return TG_OK;
}

static int sg_check_dims(const char* who, int obs_dim, int act_dim, int64_t m) {
    TG_REQUIRE(act_dim >= 1 && act_dim <= 4, "%s: act_dim=%d outside [1, 4]", who, act_dim);
    TG_REQUIRE(obs_dim >= 1 && obs_dim + act_dim <= kTileMaxIn, "%s: %d observations + %d actions outside [2, %d]", who, obs_dim, act_dim,
               kTileMaxIn);
    TG_REQUIRE(m > 0 && m < ((int64_t)1 << 31), "%s: m=%lld outside [1, 2^31)", who, (long long)m);
    return TG_OK;
}

// the critics of a q_evaluate launch and the tensors all three of its entries need
static int sg_plan_q(const char* who, const tg_policy_net* q1, const tg_policy_net* q2, const tg_policy_sac_grad_args* s, SgArgs& args) {
    TG_REQUIRE(s != nullptr, "%s: null arguments", who);
    if (int rc = sg_check_dims(who, s->obs_dim, s->act_dim, s->m)) return rc;
    const tg_policy_net* nets[2] = {q1, q2};
    const char* names[2] = {"Q1", "Q2"};
    for (int r = 0; r < (q2 ? 2 : 1); ++r) {
        if (int rc = sg_fill_net(who, names[r], nets[r], 1, s->act_dim * (nets[r] ? nets[r]->out_dim[0] : 0), true, args.net[r])) return rc;
        TG_REQUIRE(args.net[r].S == s->obs_dim + s->act_dim, "%s: %s reads %d inputs, not %d observations + %d actions", who, names[r],
                   args.net[r].S, s->obs_dim, s->act_dim);
    }
    if (q2 == nullptr) args.net[1] = args.net[0];
    float* const acts[2] = {s->d_acts1, s->d_acts2};
    TG_REQUIRE(s->d_obs && s->d_xcat && s->d_acts1 && (q2 == nullptr || s->d_acts2), "%s: null pointer", who);
    TG_REQUIRE((((uintptr_t)s->d_acts1 | (uintptr_t)s->d_acts2) & 15) == 0, "%s: the activations are not 16-B aligned", who);
    args.S = s->obs_dim; args.A = s->act_dim; args.obs = s->d_obs; args.rows = s->m; args.xcat = s->d_xcat;
    args.acts[0] = acts[0]; args.acts[1] = acts[1];
    return TG_OK;
}

static int sg_plan_q_backward(const char* who, const tg_policy_net* q2, const tg_policy_sac_grad_args* s, SgArgs& args) {
    TG_REQUIRE(s->d_g_q1 && s->d_dz1 && s->d_dout1 && (q2 == nullptr || (s->d_g_q2 && s->d_dz2 && s->d_dout2)), "%s: null pointer", who);
    TG_REQUIRE((((uintptr_t)s->d_dz1 | (uintptr_t)s->d_dz2 | (uintptr_t)s->d_dout1 | (uintptr_t)s->d_dout2 | (uintptr_t)s->d_g_act) & 15) == 0,
               "%s: dZ / d_out / the action gradient are not 16-B aligned", who);
    args.g_q[0] = s->d_g_q1; args.g_q[1] = s->d_g_q2;
    args.dz[0] = s->d_dz1; args.dz[1] = s->d_dz2;
    args.dout[0] = s->d_dout1; args.dout[1] = s->d_dout2;
    args.g_act = s->d_g_act;
    return TG_OK;
}

// the actor of an rsample launch and the tensors all three of its entries need
static int sg_plan_actor(const char* who, const tg_policy_net* actor, const tg_policy_sac_grad_args* s, SgArgs& args) {
    TG_REQUIRE(s != nullptr, "%s: null arguments", who);
    if (int rc = sg_check_dims(who, s->obs_dim, s->act_dim, s->m)) return rc;
    if (int rc = sg_fill_net(who, "the actor", actor, 2 * s->act_dim, 0, true, args.net[0])) return rc;
    TG_REQUIRE(args.net[0].S == s->obs_dim, "%s: obs_dim=%d, the actor reads %d inputs", who, s->obs_dim, args.net[0].S);
    args.net[1] = args.net[0];
    TG_REQUIRE(s->d_obs && s->d_action && s->d_head_rows && s->d_acts1, "%s: null pointer", who);
    TG_REQUIRE((((uintptr_t)s->d_acts1 | (uintptr_t)s->d_head_rows) & 15) == 0, "%s: the activations / head rows are not 16-B aligned", who);
    args.S = s->obs_dim; args.A = s->act_dim; args.obs = s->d_obs; args.rows = s->m;
    args.action = s->d_action; args.head_rows = s->d_head_rows; args.acts[0] = args.acts[1] = s->d_acts1;
    return TG_OK;
}

static int sg_plan_actor_backward(const char* who, const tg_policy_sac_grad_args* s, SgArgs& args) {
    TG_REQUIRE(s->d_g_action && s->d_g_logp && s->d_dz1 && s->d_dout1, "%s: null pointer", who);
    TG_REQUIRE((((uintptr_t)s->d_dz1 | (uintptr_t)s->d_dout1) & 15) == 0, "%s: dZ / d_out are not 16-B aligned", who);
    args.g_action = s->d_g_action; args.g_logp = s->d_g_logp;
    args.dz[0] = args.dz[1] = s->d_dz1;
    args.dout[0] = args.dout[1] = s->d_dout1;
    return TG_OK;
}

template <typename K>
static int sg_launch(const char* who, K kernel, LdsOptIn& opt_in, const SgArgs& args, int nets, bool backward, int extra_per_h,
                     int32_t grid_limit, hipStream_t st) {
    size_t shmem = 0;
    for (int r = 0; r < nets; ++r) {
        const size_t b = backward ? bwd_lds_bytes(args.net[r], extra_per_h * args.net[r].H) : ring_tables_lds_bytes(args.net[r]);
        shmem = b > shmem ? b : shmem;
    }
    return launch_row_tiles(who, kernel, opt_in, args, nets, shmem, grid_limit, 2, st);
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_policy_sac_grad_workspace(const tg_policy_net* actor, const tg_policy_net* q1, const tg_policy_net* q2, int32_t act_dim, int64_t m,
                                 int64_t* act_floats, int64_t* grad_floats, int64_t* partial_floats) {
    const char* who = "tg_policy_sac_grad_workspace";
    TG_REQUIRE((actor || q1) && act_floats && grad_floats && partial_floats, "%s: null pointer", who);
    TG_REQUIRE(q2 == nullptr || q1 != nullptr, "%s: Q2 without Q1", who);
    TG_REQUIRE(act_dim >= 1 && act_dim <= 4, "%s: act_dim=%d outside [1, 4]", who, act_dim);
    TG_REQUIRE(m > 0 && m < ((int64_t)1 << 31), "%s: m=%lld outside [1, 2^31)", who, (long long)m);
    const tg_policy_net* nets[3] = {actor, q1, q2};
    const char* names[3] = {"the actor", "Q1", "Q2"};
    int64_t slab_rows, tiles[2] = {0, 0};
    int32_t n_slabs;
    pg_slabs(m, slab_rows, n_slabs);
    for (int r = 0; r < 3; ++r) {
        act_floats[r] = grad_floats[r] = 0;
        if (nets[r] == nullptr) continue;
        PolicyNet n = {};
        const int L = nets[r]->n_layers, H0 = L >= 1 ? nets[r]->out_dim[0] : 0;
        if (int rc = sg_fill_net(who, names[r], nets[r], r == 0 ? 2 * act_dim : 1, r == 0 ? 0 : act_dim * H0, false, n)) return rc;
        TG_REQUIRE(r == 0 || n.S > act_dim, "%s: %s reads %d inputs, no observation beside %d actions", who, names[r], n.S, act_dim);
        act_floats[r] = (int64_t)n.nh * m * n.H;
        grad_floats[r] = pg_grad_floats(n);
        tiles[r != 0] += pg_tiles(n);
    }
    partial_floats[0] = tiles[0] * n_slabs * kPgPartial;
    partial_floats[1] = tiles[1] * n_slabs * kPgPartial;
    return TG_OK;
}

int tg_policy_q_eval_forward(const tg_policy_net* q1, const tg_policy_net* q2, const tg_policy_sac_grad_args* s, void* stream) {
    const char* who = "tg_policy_q_eval_forward";
    SgArgs args = {};
    if (int rc = sg_plan_q(who, q1, q2, s, args)) return rc;
    TG_REQUIRE(s->d_act && s->d_q1 && (q2 == nullptr || s->d_q2), "%s: null pointer", who);
    args.act = s->d_act; args.q[0] = s->d_q1; args.q[1] = s->d_q2;
    static LdsOptIn opt_in;
    return sg_launch(who, policy_q_eval_forward_kernel, opt_in, args, q2 ? 2 : 1, false, 0, s->grid_limit, (hipStream_t)stream);
}

int tg_policy_q_eval_backward(const tg_policy_net* q1, const tg_policy_net* q2, const tg_policy_sac_grad_args* s, void* stream) {
    const char* who = "tg_policy_q_eval_backward";
    SgArgs args = {};
    if (int rc = sg_plan_q(who, q1, q2, s, args)) return rc;
    if (int rc = sg_plan_q_backward(who, q2, s, args)) return rc;
    static LdsOptIn opt_in;
    return sg_launch(who, policy_q_eval_backward_kernel, opt_in, args, q2 ? 2 : 1, true, s->act_dim, s->grid_limit, (hipStream_t)stream);
}

int tg_policy_rsample_forward(const tg_policy_net* actor, const tg_policy_sac_grad_args* s, void* stream) {
    const char* who = "tg_policy_rsample_forward";
    SgArgs args = {};
    if (int rc = sg_plan_actor(who, actor, s, args)) return rc;
    TG_REQUIRE(s->d_calls && s->d_logp && s->d_eps, "%s: null pointer", who);
    TG_REQUIRE(s->env_offset >= 0, "%s: a negative env_offset", who);
    TG_REQUIRE(s->log_std_lo <= s->log_std_hi, "%s: log_std bounds [%g, %g] are empty", who, (double)s->log_std_lo, (double)s->log_std_hi);
    args.calls = s->d_calls; args.seed = s->seed; args.env_offset = s->env_offset;
    args.ls_lo = s->log_std_lo; args.ls_hi = s->log_std_hi;
    args.logp = s->d_logp; args.eps = s->d_eps;
    static LdsOptIn opt_in;
    return sg_launch(who, policy_rsample_forward_kernel, opt_in, args, 1, false, 0, s->grid_limit, (hipStream_t)stream);
}

int tg_policy_rsample_backward(const tg_policy_net* actor, const tg_policy_sac_grad_args* s, void* stream) {
    const char* who = "tg_policy_rsample_backward";
    SgArgs args = {};
    if (int rc = sg_plan_actor(who, actor, s, args)) return rc;
    if (int rc = sg_plan_actor_backward(who, s, args)) return rc;
    static LdsOptIn opt_in;
    return sg_launch(who, policy_rsample_backward_kernel, opt_in, args, 1, true, 0, s->grid_limit, (hipStream_t)stream);
}

int tg_policy_sac_weight_grad(const tg_policy_net* actor, const tg_policy_net* q1, const tg_policy_net* q2,
                              const tg_policy_sac_grad_args* s, void* stream) {
    const char* who = "tg_policy_sac_weight_grad";
    TG_REQUIRE((actor != nullptr) != (q1 != nullptr), "%s: the actor's layers or the critics', one launch each", who);
    SgArgs args = {};
    PgDwArgs d = {};
    int tiles = 0, nets = 1;
    float* grads[2] = {s ? s->d_grad1 : nullptr, s ? s->d_grad2 : nullptr};
    if (actor) {
        if (int rc = sg_plan_actor(who, actor, s, args)) return rc;
        if (int rc = sg_plan_actor_backward(who, s, args)) return rc;
    } else {
        if (int rc = sg_plan_q(who, q1, q2, s, args)) return rc;
        if (int rc = sg_plan_q_backward(who, q2, s, args)) return rc;
        nets = q2 ? 2 : 1;
    }
    TG_REQUIRE(s->d_grad1 && s->d_partials && (nets == 1 || s->d_grad2), "%s: null gradient or partials pointer", who);
    TG_REQUIRE(((uintptr_t)s->d_partials & 15) == 0, "%s: the partials are not 16-B aligned", who);
    const int ld_dout = actor ? kSgActorOut : kSgQOut;
    for (int r = 0; r < nets; ++r)
        pg_add_net_jobs(d, tiles, args.net[r], s->m, actor ? args.obs : args.xcat, args.acts[r], args.dz[r], args.dout[r], ld_dout, grads[r],
                        false);
    // the heads: their float64 partials lie where the workspace entry counted the heads' tiles, behind the tiles in use
    SgHeadArgs h = {};
    h.rows = s->m;
    pg_slabs(s->m, h.slab_rows, h.n_slabs);
    int64_t at = (int64_t)tiles * h.n_slabs * kPgPartial;
    for (int r = 0; r < nets; ++r) {
        const PolicyNet& n = args.net[r];
        h.dout[r] = args.dout[r]; h.ld[r] = ld_dout; h.O[r] = n.O; h.H[r] = n.H;
        h.top[r] = args.acts[r] + (int64_t)(n.nh - 1) * s->m * n.H;
        h.gw[r] = grads[r] + pg_grad_floats(n) - (int64_t)n.O * (n.H + 1);
        h.gb[r] = h.gw[r] + (int64_t)n.O * n.H;
        h.part[r] = reinterpret_cast<double*>(s->d_partials + at);
        static_assert(2 * kSgActorOut * (256 + 1) <= kPgPartial, "a head's float64 partial fits one tile's partial");
        at += (int64_t)(n.H / kPgTile) * h.n_slabs * kPgPartial;
    }
    hipStream_t st = (hipStream_t)stream;
    if (int rc = policy_weight_grad_launch(who, d, tiles, s->m, s->d_partials, st)) return rc;
    hipLaunchKernelGGL(policy_sac_head_grad_kernel, dim3((unsigned)nets, (unsigned)h.n_slabs), dim3(256), 0, st, h);
    TG_LAUNCH_CHECK(who);
    hipLaunchKernelGGL(policy_sac_head_grad_finish_kernel, dim3((unsigned)nets), dim3(256), 0, st, h);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

}  // extern "C"
