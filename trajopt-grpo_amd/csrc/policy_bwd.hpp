// The backward side of the DeviceActor kernels that policy_grad.hip (evaluate) and policy_sac_grad.hip (rsample, q_evaluate) share:
// the ONE definition of the backward-data body, and the host side of the weight-gradient launch.  Like policy_tile.hpp, the device
// part is a primitive that is inlined into its caller's kernel (no device symbol crosses a translation unit); the weight-gradient
// KERNELS live in policy_grad.hip alone and are reached from a second file through the host function policy_weight_grad_launch.
//
// Backward data (the form, and why: policy_grad.hip's header comment): a wave owns 16 rows; the ring runs over the 16-output-row
// blocks of W_l from the top H x H layer down, landed row-major with 16 floats of padding behind every 4-row group; all H / 16
// accumulator tiles stay live and every 4-byte LDS read feeds one MFMA.  What differs between the callers is an argument:
//   kMaxOut     head outputs the vector-unit product dA_top = d_out . W_head is unrolled over (gaussian head / a critic: 4, the
//               squashed head's (mu, ls) pairs: 8)
//   head_grad   (row, rowc, store, d_out): fills the row's d_out[kMaxOut] (zeros past the head's width) and stores what its
//               weight-gradient job reads
//   on_dz0      (dz, row, valid): sees the wave's dZ_0 registers once the first layer's dZ is formed (q_evaluate: the action gradient)
#pragma once
#include "policy_tile.hpp"

namespace tg {

constexpr int kPgMaxSlabs = 32;
constexpr int kPgTile = 64, kPgLd = 80;                 // weight gradient: tile edge, LDS row stride (floats)
constexpr int kPgPartial = kPgTile * kPgTile + kPgTile; // floats of one partial: the tile and its bias sums
constexpr int kPgJobs = 2 * kPolicyLinear;

// ring slots of 16 H + 64 floats, the head rows [O][H] behind them, `extra` floats of the caller's behind those
static size_t bwd_lds_bytes(const PolicyNet& n, int extra = 0) {
    return (size_t)kTileD * (16 * n.H + 64) * 4 + ((size_t)n.O * n.H + extra) * 4;
}
template <int H>
__device__ static inline float* bwd_lds_extra(uint4* lds, int O) {
    return reinterpret_cast<float*>(lds) + kTileD * 4 * (4 * H + 16) + O * H;
}

template <int H, int kAct, int kMaxOut, typename Args, typename HeadGrad, typename OnDz0>
__device__ __attribute__((always_inline)) static inline void backward_tiles(const Args& a, const bool critic, const int nh, const int O,
                                                                            const float* acts, float* dzb, uint4* lds,
                                                                            HeadGrad&& head_grad, OnDz0&& on_dz0) {
    // a 16-output-row block of W_l: four 4-row groups of 4 H floats (H / 64 DMA pieces each), 16 floats of padding behind each
    constexpr int NT = H / 16, WPW = kTileWaves, D = kTileD, P = kTileP, PPG = H / 64, GROUP = 4 * H + 16, SLOT = 4 * GROUP;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int n_hh = nh - 1;
    float* ring = reinterpret_cast<float*>(lds);
    float* wh_s = ring + D * SLOT;                                    // [O][H]
    const int64_t rows = a.rows;
    const int64_t n_rounds = (rows + 63) / 64;

    // ---- the ring: block (l, t) = rows 16 t .. + 15 of W_l, l from the top H x H layer down to layer 1 ----
    int pre_l = n_hh, pre_t = 0, pre_slot = 0, cur_slot = 0;
    auto dma_next = [&]() {
        const float* src = net_weight(a, critic, pre_l) + (16 * pre_t * H + 4 * lane);
        float* slot = ring + pre_slot * SLOT;
#pragma unroll
        for (int q = 0; q < NT / WPW; ++q) {
            const int piece = q * WPW + wave;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint4*>(src + 256 * piece),
                                             (lds_void*)(slot + (piece / PPG) * GROUP + (piece % PPG) * 256), 16, 0, 0);
        }
        pre_t = (pre_t + 1 == NT) ? 0 : pre_t + 1;
        pre_l = pre_t != 0 ? pre_l : (pre_l == 1 ? n_hh : pre_l - 1);
        pre_slot = (pre_slot + 1 == D) ? 0 : pre_slot + 1;
    };
    if (n_hh > 0) {
#pragma unroll
        for (int b = 0; b < P; ++b) dma_next();
    }
    {
        const float* Wh = net_weight(a, critic, nh);
        for (int q = tid; q < O * H; q += 64 * WPW) wh_s[q] = Wh[q];
    }
    __syncthreads();                                                  // (the head; drains the prologue's DMA too: once)
    constexpr int kWait = (P - 1) * (NT / WPW);

    for (int64_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const int64_t row = round * 64 + wave * 16 + j;
        const bool valid = row < rows;
        const int64_t rowc = valid ? row : rows - 1;
        // ---- the head's gradient, per row (every lane group holds the same bits, lane group 0 stores) ----
        float d_out[kMaxOut];
        head_grad(row, rowc, valid && g == 0, d_out);
        // dZ_l = dA * act'(acts[l]) from the stored activation, kept as the next product's B operand and stored [m][H]
        f32x4 dz[NT];
        auto mask_store = [&](int l, const f32x4 (&dA)[NT]) {
            const int64_t at = ((int64_t)l * rows + rowc) * H + 4 * g;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float4 av = *reinterpret_cast<const float4*>(acts + at + 16 * t);
                const float h[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (kAct == TG_ACT_TANH) dz[t][r] = dA[t][r] * fmaf(-h[r], h[r], 1.0f);
                    else dz[t][r] = h[r] > 0.f ? dA[t][r] : 0.f;
                }
                if (valid) *reinterpret_cast<float4*>(dzb + at + 16 * t) = float4{dz[t][0], dz[t][1], dz[t][2], dz[t][3]};
            }
        };
        // ---- dA_top = d_out . W_head on the vector unit ----
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < kMaxOut; ++k) {
                if (k < O) {
                    const float4 w = lds_f4(wh_s + k * H + 16 * t + 4 * g);
                    acc[t][0] = fmaf(d_out[k], w.x, acc[t][0]);
                    acc[t][1] = fmaf(d_out[k], w.y, acc[t][1]);
                    acc[t][2] = fmaf(d_out[k], w.z, acc[t][2]);
                    acc[t][3] = fmaf(d_out[k], w.w, acc[t][3]);
                }
            }
        }
        mask_store(n_hh, acc);
        // ---- H x H layers from the top down: dA_{l-1}[row][16 ti + ii] = sum_o dZ_l[row][o] W_l[o][16 ti + ii] ----
        for (int l = n_hh; l >= 1; --l) {
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                TG_RING_WAIT(kWait)
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                const float* __restrict__ p = ring + cur_slot * SLOT + g * GROUP + j;
                cur_slot = (cur_slot + 1 == D) ? 0 : cur_slot + 1;
                dma_next();                                           // (refills the slot of the block before this one)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti)
                        acc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(lds_f(p + r * H + 16 * ti), dz[t][r], acc[ti], 0, 0, 0);
                }
            }
            mask_store(l - 1, acc);
        }
        on_dz0(dz, row, valid);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- weight gradient: the argument tables of policy_grad.hip's kernels, and their host side ------------------------------------------
// One Linear layer of one net: dW [No][Ni] = dz^T a over the rows, db [No] = column sums of dz.  `w_dz` / `w_a`: the operands' stored
// widths (a head's d_out rows are zero-padded to 4 or 8); `vec_*`: 16-byte loads (an aligned base, a leading dimension and a width
// that are multiples of 4), else floats one by one (the observations, a critic's [obs, act] rows).
struct PgJob {
    const float* dz; const float* a;
    float* gw; float* gb;
    int32_t ld_dz, w_dz, ld_a, w_a, No, Ni, tiles_i, tile_base, vec_dz, vec_a;
};
struct PgDwArgs {
    PgJob job[kPgJobs];
    int32_t n_jobs, n_slabs;
    int64_t rows, slab_rows;
    float* partials;                // [tiles][n_slabs][kPgPartial]
};

static int64_t pg_grad_floats(const PolicyNet& n) {
    return (int64_t)n.H * (n.S + 1) + (int64_t)(n.nh - 1) * n.H * (n.H + 1) + (int64_t)n.O * (n.H + 1);
}
static int64_t pg_tiles(const PolicyNet& n) {
    const int64_t th = n.H / kPgTile;
    return th + (n.nh - 1) * th * th + th;                           // first layer (S <= 32: one column tile), H x H layers, head
}
static void pg_slabs(int64_t m, int64_t& slab_rows, int32_t& n_slabs) {
    const int64_t chunks = ceil_div(m, kPgTile), per = ceil_div(chunks, kPgMaxSlabs);
    slab_rows = per * kPgTile;
    n_slabs = (int32_t)ceil_div(chunks, per);
}

// the jobs of one net, layer by layer, behind those already in `d`: its input rows x [m][n.S], its stored activations and dZ
// [nh][m][H], its head gradient rows dout [m][ld_dout], and where its gradient goes (torch's layout, layers back to back);
// `with_head` false: the head layer is the caller's own (its gradient lies behind the hidden layers' all the same)
static void pg_add_net_jobs(PgDwArgs& d, int& tiles, const PolicyNet& n, int64_t m, const float* x, const float* acts, const float* dz,
                            const float* dout, int ld_dout, float* grad, bool with_head = true) {
    float* gp = grad;
    for (int l = 0; l <= (with_head ? n.nh : n.nh - 1); ++l) {
        PgJob& jb = d.job[d.n_jobs++];
        const bool first = l == 0, head = l == n.nh;
        jb.dz = head ? dout : dz + (int64_t)l * m * n.H;
        jb.ld_dz = jb.w_dz = head ? ld_dout : n.H;
        jb.No = head ? n.O : n.H;
        jb.a = first ? x : acts + (int64_t)(l - 1) * m * n.H;
        jb.ld_a = jb.w_a = jb.Ni = first ? n.S : n.H;
        jb.vec_dz = 1;
        jb.vec_a = !first || (n.S % 4 == 0 && ((uintptr_t)x & 15) == 0);
        jb.gw = gp; jb.gb = gp + (int64_t)jb.No * jb.Ni;
        gp = jb.gb + jb.No;
        jb.tiles_i = (int32_t)ceil_div(jb.Ni, kPgTile);
        jb.tile_base = tiles;
        tiles += (int)ceil_div(jb.No, kPgTile) * jb.tiles_i;
    }
}

// the two launches over `d`'s jobs (rows, slabs and partials are filled in here); defined in policy_grad.hip beside the kernels
__attribute__((visibility("hidden"))) int policy_weight_grad_launch(const char* who, PgDwArgs& d, int tiles, int64_t m, float* partials,
                                                                    hipStream_t st);

}  // namespace tg
