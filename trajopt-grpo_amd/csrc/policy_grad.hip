// The learner side of DeviceActor (DeviceActor.evaluate, trajopt-grpo_amd/policy_step.py): stored (obs, action) rows re-evaluated
// forward and backward in float32 on v_mfma_f32_16x16x4_f32, against torch's own row-major `nn.Linear` storage -- weights are READ
// where torch keeps them and gradients are WRITTEN in torch's [out][in] / [out] layout.  Three launches:
//
//   tg_policy_eval_forward      policy_tile.hpp's forward as policy_step.hip runs it (a wave owns 16 rows, 4 waves per workgroup, the
//                               net as grid dimension y) with two differences: every hidden layer's 16 x H post-activation tile goes
//                               to acts[l][m][H] (lane (j, g)'s registers r = 0..3 of tile t are features 16 t + 4 g + r of row j:
//                               one 16-byte store), and the epilogue takes the action from memory.  No Philox.
//   tg_policy_eval_backward     backward data on the same split.  Head gradient and dA_top = d_out . W_head on the vector unit, then per
//                               H x H layer from the top: dZ_l = dA_l * act'(acts[l]) (stored [m][H]), dA_{l-1} = dZ_l . W_l on MFMAs.
//   tg_policy_eval_weight_grad  dW_l = dZ_l^T A_{l-1}, db_l = column sums of dZ_l, for every layer of both nets in one launch, and a
//                               fixed-order finishing pass.
//
// The backward-data body and the weight-gradient argument tables are policy_bwd.hpp's, shared with policy_sac_grad.hip (rsample,
// q_evaluate), which reaches the weight-gradient kernels of this file through policy_weight_grad_launch.
//
// Backward data, the form chosen: the operand of step (t, r) is W_l[16 t + 4 g + r][16 ti + ii] -- a COLUMN piece of W_l.  The ring
// runs over the same contiguous 16-output-row regions of W_l as the forward (block t = rows 16 t .. 16 t + 15, 16 H floats in one
// run, so the DMA is a linear copy: lane `lane` of piece p moves bytes 1024 p + 16 lane), landed plain row-major in LDS, and all
// H / 16 input-feature accumulator tiles of the wave's 16 rows stay live (64 registers at H = 256) while the block is consumed:
// lane (ii, g) reads the 4 bytes at row 4 g + r, column 16 ti + ii, and each such read feeds one MFMA.  The four lane groups read
// four different 4-row groups, so every 4-row group (H / 64 DMA pieces) is followed by 16 floats of padding: the groups' reads fall
// into four different quarters of the banks.  Why not the transposing 16 x 16 sub-block read: it keeps one accumulator tile live
// instead of H / 16, but needs H / 16 passes over the ring per layer (each block re-fetched per input tile) or a transposed copy
// of W_l in LDS (64 KiB+ at H = 256 beside the ring); the accumulators fit (128 VGPRs with the dZ operands at H = 256, the
// forward's count), so the single pass wins on bytes moved.
//
// Weight gradient: a workgroup owns a 64 x 64 output tile of one layer and a slab of rows; per 64 rows it stages the dZ columns and
// the A columns of its tile through LDS (row stride 80 floats: the four lane groups' rows land in different bank quarters), wave w
// owns output rows 16 w .. 16 w + 15 against the four 16-column tiles (one A read per four B reads).  Both operands are row-major
// over rows, which is what the 16x16x4 fragments want: lane (i, g) reads element [4 s + g][i].  The head (O <= 4 rows of dW) and
// the first layer (K = S <= 32 columns) run as zero-PADDED TILES of the same body, not on the vector unit: operand columns past
// the width are staged as zeros and never stored.  Bias sums: the workgroups of column tile 0 add their staged dZ columns on the
// vector unit.  Partials [tile][slab][64 x 64 + 64] are added over the slabs in index order by the finishing pass: no atomics, the
// same bits at every call.  The slab count depends on m alone (<= 32 slabs of whole 64-row chunks).
#include <stdlib.h>

#include "tg_common.hpp"
#include "policy_tile.hpp"
#include "policy_bwd.hpp"

namespace tg {

constexpr int kPgMaxOut = 4;                            // gaussian head: <= 4 means; a critic: 1

struct PgArgs {
    PolicyNet net[2];               // [0] the actor, [1] the critic
    int32_t act_dim;
    const float* x;                 // [rows][S], unpadded
    const float* action;            // [rows][A]
    int64_t rows;
    const float* log_std;           // [A]
    float* mu; float* logp; float* entropy; float* value;
    float* acts[2];                 // [nh][rows][H] per net
    const float* g_logp; const float* g_entropy; const float* g_value;
    float* dz[2];                   // [nh][rows][H] per net
    float* dout[2];                 // [rows][4] per net, zero-padded
    float* std_rows;                // [rows][4], zero-padded
};

static size_t pg_bwd_lds_bytes(const PolicyNet& n) { return bwd_lds_bytes(n); }

// ---- 1. forward: the shared tile forward, the activation stores as its on_tile, the epilogue on a given action ------------------------
template <int H, int kAct>
__device__ __attribute__((always_inline)) static inline void pg_forward(const PgArgs& a, const int S, const int nh, const int O,
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
    float* acts = critic ? a.acts[1] : a.acts[0];

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
    __syncthreads();

    for (int64_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const int64_t row = round * 64 + wave * 16 + j;
        const bool valid = row < rows;
        const int64_t rowc = valid ? row : rows - 1;
        f32x4 xin[NT];
        // the lane's 16 bytes of layer l's tile mo: features 16 mo + 4 g .. + 3 of its row
        auto store_act = [&](int l, int mo, const f32x4& v) {
            if (valid) *reinterpret_cast<float4*>(acts + ((int64_t)l * rows + row) * H + 16 * mo + 4 * g) = float4{v[0], v[1], v[2], v[3]};
        };

        float xr[kTileMaxIn / 4];
#pragma unroll
        for (int s = 0; s < kTileMaxIn / 4; ++s) {
            const int k = 4 * s + g;
            const bool in = k < S;
            const float v = a.x[rowc * S + (in ? k : 0)];
            xr[s] = in ? v : 0.f;
        }
        first_layer<H, kAct>(tb.w0, tb.bias, K4, lane, xr, xin, store_act);
        hidden_layers<H, kAct>(ring, cur_slot, tb.bias, n_hh, lane, xin, dma_next, store_act);
        const int A = critic ? 1 : a.act_dim;
        float mu_k[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < A) mu_k[k] = head_out<NT>(tb.wh, tb.bh, xin, k, g);
        const bool store = valid && g == 0;
        if (critic) {
            if (store) a.value[row] = mu_k[0];
            continue;
        }
        // ---- the actor's epilogue on the GIVEN action: eps = (a - mu) / exp(log_std), then act()'s expression term by term ----
        float logp = 0.f, ent = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < A) {
                const float ls = a.log_std[k];
                const float av = a.action[rowc * A + k];
                const float e = rn_div(rn_sub(av, mu_k[k]), expf(ls));
                logp = rn_add(logp, gaussian_logp_term(e, ls));
                ent = rn_add(ent, rn_add(ls, 1.4189385332046727f));
                if (store) a.mu[row * A + k] = mu_k[k];
            }
        }
        if (store) {
            a.logp[row] = logp;
            a.entropy[row] = ent;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- 2. backward data: policy_bwd.hpp's body under the gaussian head's / the critic's head gradient -----------------------------------
template <int H, int kAct>
__device__ __attribute__((always_inline)) static inline void pg_backward(const PgArgs& a, const int nh, const int O, const int role,
                                                                         uint4* lds) {
    const bool critic = role == 1;
    float* doutb = critic ? a.dout[1] : a.dout[0];
    auto head_grad = [&](int64_t row, int64_t rowc, bool store, float (&d_out)[kPgMaxOut]) {
        float d_std[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kPgMaxOut; ++k) d_out[k] = 0.f;
        if (critic) {
            d_out[0] = a.g_value[rowc];
        } else {
            const float gl = a.g_logp[rowc], ge = a.g_entropy[rowc];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < a.act_dim) {
                    const float inv = expf(-a.log_std[k]);
                    const float e = (a.action[rowc * a.act_dim + k] - a.mu[rowc * a.act_dim + k]) * inv;
                    d_out[k] = gl * e * inv;
                    d_std[k] = fmaf(gl, fmaf(e, e, -1.0f), ge);
                }
            }
        }
        if (store) {
            *reinterpret_cast<float4*>(doutb + row * 4) = float4{d_out[0], d_out[1], d_out[2], d_out[3]};
            if (!critic) *reinterpret_cast<float4*>(a.std_rows + row * 4) = float4{d_std[0], d_std[1], d_std[2], d_std[3]};
        }
    };
    backward_tiles<H, kAct, kPgMaxOut>(a, critic, nh, O, critic ? a.acts[1] : a.acts[0], critic ? a.dz[1] : a.dz[0], lds, head_grad,
                                       [](const f32x4 (&)[H / 16], int64_t, bool) {});
}

__global__ __launch_bounds__(64 * kTileWaves, 2) void policy_eval_forward_kernel(PgArgs a) {
    extern __shared__ uint4 lds[];
    const int role = __builtin_amdgcn_readfirstlane((int)blockIdx.y);
    const bool critic = role == 1;
    const int S = critic ? a.net[1].S : a.net[0].S, H = critic ? a.net[1].H : a.net[0].H, nh = critic ? a.net[1].nh : a.net[0].nh;
    const int O = critic ? a.net[1].O : a.net[0].O, act = critic ? a.net[1].act : a.net[0].act;
    dispatch_width_act(H, act, [&](auto h, auto k) __attribute__((always_inline)) {
        pg_forward<decltype(h)::value, decltype(k)::value>(a, S, nh, O, role, lds);
    });
}

__global__ __launch_bounds__(64 * kTileWaves, 2) void policy_eval_backward_kernel(PgArgs a) {
    extern __shared__ uint4 lds[];
    const int role = __builtin_amdgcn_readfirstlane((int)blockIdx.y);
    const bool critic = role == 1;
    const int H = critic ? a.net[1].H : a.net[0].H, nh = critic ? a.net[1].nh : a.net[0].nh;
    const int O = critic ? a.net[1].O : a.net[0].O, act = critic ? a.net[1].act : a.net[0].act;
    dispatch_width_act(H, act, [&](auto h, auto k) __attribute__((always_inline)) {
        pg_backward<decltype(h)::value, decltype(k)::value>(a, nh, O, role, lds);
    });
}

// ---- 3. weight gradient --------------------------------------------------------------------------------------------------------------
// (PgJob / PgDwArgs: policy_bwd.hpp)
__device__ static inline int pg_job_of(const PgDwArgs& a, int tile) {
    int jb = 0;
    for (int q = 1; q < kPgJobs; ++q) jb = (q < a.n_jobs && tile >= a.job[q].tile_base) ? q : jb;
    return jb;
}

// 64 rows x 64 columns of a row-major operand into LDS (row stride kPgLd), zeros past the rows and past the width
__device__ static inline void pg_stage(float* __restrict__ dst, const float* __restrict__ src, int64_t ld, int width, bool vec, int64_t r0,
                                       int64_t r_end, int col0, int tid) {
#pragma unroll
    for (int q = tid; q < kPgTile * kPgTile / 4; q += 64 * kTileWaves) {
        const int rr = q >> 4, c = col0 + 4 * (q & 15);
        const int64_t row = r0 + rr;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
            const bool ok = row < r_end && c < width;
            const float4 t = *reinterpret_cast<const float4*>(src + (ok ? row * ld + c : 0));
            v = float4{ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f};
        } else {
            auto one = [&](int k) {                                   // (clamped address, selected value: no load under a branch)
                const bool ok = row < r_end && c + k < width;
                const float t = src[ok ? row * ld + c + k : 0];
                return ok ? t : 0.f;
            };
            v = float4{one(0), one(1), one(2), one(3)};
        }
        *reinterpret_cast<float4*>(dst + rr * kPgLd + 4 * (q & 15)) = v;
    }
}

__global__ __launch_bounds__(64 * kTileWaves) void policy_eval_weight_grad_kernel(PgDwArgs a) {
    __shared__ float dz_s[kPgTile * kPgLd];
    __shared__ float a_s[kPgTile * kPgLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x, slab = blockIdx.y;
    const PgJob& jb = a.job[pg_job_of(a, tile)];
    const int local = tile - jb.tile_base, to = local / jb.tiles_i, ti0 = local - to * jb.tiles_i;
    const int64_t r_begin = (int64_t)slab * a.slab_rows;
    const int64_t r_end = r_begin + a.slab_rows < a.rows ? r_begin + a.slab_rows : a.rows;
    const bool with_bias = ti0 == 0;

    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;                                                 // column tid & 63 of dz over rows 16 (tid >> 6) .. + 15 of every chunk
    for (int64_t r0 = r_begin; r0 < r_end; r0 += kPgTile) {
        __syncthreads();                                              // (everyone has finished with the chunk before)
        pg_stage(dz_s, jb.dz, jb.ld_dz, jb.w_dz, jb.vec_dz != 0, r0, r_end, kPgTile * to, tid);
        pg_stage(a_s, jb.a, jb.ld_a, jb.w_a, jb.vec_a != 0, r0, r_end, kPgTile * ti0, tid);
        __syncthreads();
        // lane (i, g) of step s: dz[4 s + g][16 wave + i] and a[4 s + g][16 t + i]
        const float* __restrict__ pa = dz_s + g * kPgLd + 16 * wave + i;
        const float* __restrict__ pb = a_s + g * kPgLd + i;
#pragma unroll
        for (int s = 0; s < kPgTile / 4; ++s) {
            const float av = pa[4 * s * kPgLd];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, pb[4 * s * kPgLd + 16 * t], acc[t], 0, 0, 0);
        }
        if (with_bias) {
            const float* __restrict__ pc = dz_s + 16 * (tid >> 6) * kPgLd + (tid & 63);
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) bsum += pc[rr * kPgLd];
        }
    }
    // the partial: lane (i, g) register r of tile t is dW[16 wave + 4 g + r][16 t + i] of the 64 x 64 tile
    float* part = a.partials + ((int64_t)tile * a.n_slabs + slab) * kPgPartial;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(16 * wave + 4 * g + r) * kPgTile + 16 * t + i] = acc[t][r];
    }
    if (with_bias) {
        __syncthreads();
        dz_s[tid] = bsum;
        __syncthreads();
        if (tid < kPgTile) part[kPgTile * kPgTile + tid] = (dz_s[tid] + dz_s[64 + tid]) + (dz_s[128 + tid] + dz_s[192 + tid]);
    }
}

// the slabs of a tile added in index order, written where torch keeps the gradient
__global__ __launch_bounds__(256) void policy_eval_weight_grad_finish_kernel(PgDwArgs a) {
    const int tile = blockIdx.x;
    const PgJob& jb = a.job[pg_job_of(a, tile)];
    const int local = tile - jb.tile_base, to = local / jb.tiles_i, ti0 = local - to * jb.tiles_i;
    const float* part = a.partials + (int64_t)tile * a.n_slabs * kPgPartial;
    for (int e = threadIdx.x; e < kPgPartial; e += 256) {
        if (e >= kPgTile * kPgTile && ti0 != 0) break;
        float s = 0.f;
        for (int q = 0; q < a.n_slabs; ++q) s += part[(int64_t)q * kPgPartial + e];
        if (e < kPgTile * kPgTile) {
            const int o = kPgTile * to + e / kPgTile, c = kPgTile * ti0 + e % kPgTile;
            if (o < jb.No && c < jb.Ni) jb.gw[(int64_t)o * jb.Ni + c] = s;
        } else {
            const int o = kPgTile * to + e - kPgTile * kPgTile;
            if (o < jb.No) jb.gb[o] = s;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// the shared verdict on a net, and whether both passes fit; `pointers`: the launches (the workspace entry reads widths)
static int pg_fill_net(const char* who, const char* name, const tg_policy_net* n, int outs, bool pointers, PolicyNet& out) {
    if (int rc = policy_net_check(who, name, n, outs, pointers, out)) return rc;
    const size_t fwd = ring_tables_lds_bytes(out), bwd = pg_bwd_lds_bytes(out);
    TG_REQUIRE(fwd <= 160 * 1024 && bwd <= 160 * 1024, "%s: %s needs %zu B (forward) / %zu B (backward) of LDS (> 160 KiB)", who, name, fwd, bwd);
    return TG_OK;
}

// the nets and the tensors every launch needs; `forward`: the three results too
static int pg_plan(const char* who, const tg_policy_net* actor, const tg_policy_net* critic, const tg_policy_eval_args* s, bool forward,
                   PgArgs& args) {
    TG_REQUIRE(s != nullptr, "%s: null arguments", who);
    TG_REQUIRE(s->act_dim >= 1 && s->act_dim <= 4, "%s: act_dim=%d outside [1, 4]", who, s->act_dim);
    TG_REQUIRE(s->m > 0 && s->m < ((int64_t)1 << 31), "%s: m=%lld outside [1, 2^31)", who, (long long)s->m);
    if (int rc = pg_fill_net(who, "the actor", actor, s->act_dim, true, args.net[0])) return rc;
    if (critic != nullptr) {
        if (int rc = pg_fill_net(who, "the critic", critic, 1, true, args.net[1])) return rc;
        TG_REQUIRE(args.net[1].S == args.net[0].S, "%s: the critic reads %d inputs, the actor %d", who, args.net[1].S, args.net[0].S);
        TG_REQUIRE((s->d_value || !forward) && s->d_acts_critic, "%s: d_value / d_acts_critic is null with a critic", who);
    } else {
        args.net[1] = args.net[0];
    }
    TG_REQUIRE(s->d_obs && s->d_act && s->d_log_std && s->d_mu && s->d_acts_actor, "%s: null pointer", who);
    TG_REQUIRE(!forward || (s->d_logp && s->d_entropy), "%s: d_logp / d_entropy is null", who);
    TG_REQUIRE((((uintptr_t)s->d_acts_actor | (uintptr_t)s->d_acts_critic) & 15) == 0, "%s: the activations are not 16-B aligned", who);
    args.act_dim = s->act_dim; args.x = s->d_obs; args.action = s->d_act; args.rows = s->m; args.log_std = s->d_log_std;
    args.mu = s->d_mu; args.logp = s->d_logp; args.entropy = s->d_entropy; args.value = s->d_value;
    args.acts[0] = s->d_acts_actor; args.acts[1] = s->d_acts_critic;
    return TG_OK;
}

static int pg_plan_backward(const char* who, const tg_policy_net* critic, const tg_policy_eval_args* s, PgArgs& args) {
    TG_REQUIRE(s->d_g_logp && s->d_g_entropy && s->d_dz_actor && s->d_dout_actor && s->d_std_rows, "%s: null pointer", who);
    TG_REQUIRE(critic == nullptr || (s->d_g_value && s->d_dz_critic && s->d_dout_critic), "%s: null pointer with a critic", who);
    TG_REQUIRE((((uintptr_t)s->d_dz_actor | (uintptr_t)s->d_dz_critic | (uintptr_t)s->d_dout_actor | (uintptr_t)s->d_dout_critic |
                 (uintptr_t)s->d_std_rows) & 15) == 0, "%s: dZ / d_out / the log-std rows are not 16-B aligned", who);
    args.g_logp = s->d_g_logp; args.g_entropy = s->d_g_entropy; args.g_value = s->d_g_value;
    args.dz[0] = s->d_dz_actor; args.dz[1] = s->d_dz_critic;
    args.dout[0] = s->d_dout_actor; args.dout[1] = s->d_dout_critic;
    args.std_rows = s->d_std_rows;
    return TG_OK;
}

template <typename K>
static int pg_launch(const char* who, K kernel, LdsOptIn& opt_in, const PgArgs& args, int nets, bool backward, int32_t grid_limit,
                     hipStream_t st) {
    size_t shmem = 0;
    for (int r = 0; r < nets; ++r) {
        const size_t b = backward ? pg_bwd_lds_bytes(args.net[r]) : ring_tables_lds_bytes(args.net[r]);
        shmem = b > shmem ? b : shmem;
    }
    return launch_row_tiles(who, kernel, opt_in, args, nets, shmem, grid_limit, 2, st);
}

int policy_weight_grad_launch(const char* who, PgDwArgs& d, int tiles, int64_t m, float* partials, hipStream_t st) {
    d.rows = m;
    pg_slabs(m, d.slab_rows, d.n_slabs);
    d.partials = partials;
    hipLaunchKernelGGL(policy_eval_weight_grad_kernel, dim3((unsigned)tiles, (unsigned)d.n_slabs), dim3(64 * kTileWaves), 0, st, d);
    TG_LAUNCH_CHECK(who);
    hipLaunchKernelGGL(policy_eval_weight_grad_finish_kernel, dim3((unsigned)tiles), dim3(256), 0, st, d);
    hipError_t e = hipGetLastError();                                 // (told apart from a failure of the launch before it)
    if (e != hipSuccess) return set_error(TG_ERR_HIP, "%s(finish): %s", who, hipGetErrorString(e));
    return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_policy_eval_workspace(const tg_policy_net* actor, const tg_policy_net* critic, int64_t m, int64_t* act_floats, int64_t* grad_floats,
                             int64_t* partial_floats) {
    const char* who = "tg_policy_eval_workspace";
    TG_REQUIRE(actor && act_floats && grad_floats && partial_floats, "%s: null pointer", who);
    TG_REQUIRE(m > 0 && m < ((int64_t)1 << 31), "%s: m=%lld outside [1, 2^31)", who, (long long)m);
    const tg_policy_net* nets[2] = {actor, critic};
    int64_t slab_rows, tiles = 0;
    int32_t n_slabs;
    pg_slabs(m, slab_rows, n_slabs);
    for (int r = 0; r < 2; ++r) {
        act_floats[r] = grad_floats[r] = 0;
        if (nets[r] == nullptr) continue;
        PolicyNet n = {};
        const int L = nets[r]->n_layers;                             // (the head's own width here; its range is checked below)
        const int outs = L >= 1 && L <= kPolicyLinear ? nets[r]->out_dim[L - 1] : 0;
        if (int rc = pg_fill_net(who, r ? "the critic" : "the actor", nets[r], outs, false, n)) return rc;
        TG_REQUIRE(n.O >= 1 && n.O <= (r ? 1 : kPgMaxOut), "%s: %s has %d head outputs (the gaussian head: 1..%d, a critic: 1)", who,
                   r ? "the critic" : "the actor", n.O, kPgMaxOut);
        act_floats[r] = (int64_t)n.nh * m * n.H;
        grad_floats[r] = pg_grad_floats(n);
        tiles += pg_tiles(n);
    }
    *partial_floats = tiles * n_slabs * kPgPartial;
    return TG_OK;
}

int tg_policy_eval_forward(const tg_policy_net* actor, const tg_policy_net* critic, const tg_policy_eval_args* s, void* stream) {
    const char* who = "tg_policy_eval_forward";
    PgArgs args = {};
    if (int rc = pg_plan(who, actor, critic, s, true, args)) return rc;
    static LdsOptIn opt_in;
    return pg_launch(who, policy_eval_forward_kernel, opt_in, args, critic ? 2 : 1, false, s->grid_limit, (hipStream_t)stream);
}

int tg_policy_eval_backward(const tg_policy_net* actor, const tg_policy_net* critic, const tg_policy_eval_args* s, void* stream) {
    const char* who = "tg_policy_eval_backward";
    PgArgs args = {};
    if (int rc = pg_plan(who, actor, critic, s, false, args)) return rc;
    if (int rc = pg_plan_backward(who, critic, s, args)) return rc;
    static LdsOptIn opt_in;
    return pg_launch(who, policy_eval_backward_kernel, opt_in, args, critic ? 2 : 1, true, s->grid_limit, (hipStream_t)stream);
}

int tg_policy_eval_weight_grad(const tg_policy_net* actor, const tg_policy_net* critic, const tg_policy_eval_args* s, void* stream) {
    const char* who = "tg_policy_eval_weight_grad";
    PgArgs args = {};
    if (int rc = pg_plan(who, actor, critic, s, false, args)) return rc;
    if (int rc = pg_plan_backward(who, critic, s, args)) return rc;
    TG_REQUIRE(s->d_grad_actor && s->d_partials && (critic == nullptr || s->d_grad_critic), "%s: null gradient or partials pointer", who);
    PgDwArgs d = {};
    float* grads[2] = {s->d_grad_actor, s->d_grad_critic};
    int tiles = 0;
    for (int r = 0; r < (critic ? 2 : 1); ++r)
        pg_add_net_jobs(d, tiles, args.net[r], s->m, args.x, args.acts[r], args.dz[r], args.dout[r], 4, grads[r]);
    return policy_weight_grad_launch(who, d, tiles, s->m, s->d_partials, (hipStream_t)stream);
}

}  // extern "C"
