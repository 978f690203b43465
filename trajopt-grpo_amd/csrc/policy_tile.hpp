// The float32 row-tile forward core of the DeviceActor kernels (policy_step.hip, policy_q.hip, policy_grad.hip): the ONE definition
// of the arithmetic whose bits the three advertise as equal -- sac_target's action and logp are act()'s, evaluate()'s mean and value
// are act()'s and values()'.  Everything here is a primitive that does not know its caller and is inlined into the caller's kernel
// (no device symbol crosses a translation unit).  Where the callers differ -- which block the ring fetches next, what becomes of a
// finished tile, where the action comes from -- the difference is an argument or stays in the caller.
//
// Layout (mlp_f32_wide.hip's 16-row tile, on v_mfma_f32_16x16x4_f32): a wave owns 16 rows; lane (j = lane & 15, g = lane >> 4) of
// accumulator tile t holds features 16 t + 4 g + r (r = 0..3) of row j, and register r of the four lane groups IS the B operand of
// MFMA step (t, r) of the next layer.  The A operand of that step, lane (i, g), is W[out i][16 t + 4 g + r]: four consecutive floats
// of a weight ROW of torch's own `nn.Linear.weight` storage, row-major [out][in].  The 16 output features of a block are one
// contiguous 16 x H float region of it; piece t of the block (1 KiB in LDS, lane (i, g) at byte 16 lane) is lane (i, g)'s 16 bytes
// at W + (16 mo + i) H + 16 t + 4 g: an LDS-DMA whose 64 lane addresses are 16 runs of 64 B.
//
// Ring: 3 slots of one 16-feature block (H / 16 KiB), two blocks in flight, a counted vmcnt wait and one raw s_barrier per block
// (mfma_ring.hpp's discipline).  A caller keeps the prefetch cursor and hands it over as `dma_next`, which tile_products issues
// behind its first two reads.
//
// Tables: a net's first layer (K <= 32 inputs, rows of K floats: not 16-byte aligned in general) is staged once per workgroup as
// zero-padded scalars in operand order, with the hidden biases, the head rows and the head bias (NetTables).
#pragma once
#include <type_traits>

#include "mfma_ring.hpp"
#include "act_f32.hpp"

namespace tg {

constexpr int kPolicyLinear = TG_POLICY_MAX_LAYERS;     // Linear layers of a net: up to 5 hidden layers and the head
constexpr int kTileWaves = 4;                           // waves per workgroup: 64 rows per round
constexpr int kTileD = 3, kTileP = kTileD - 1;          // ring slots, blocks in flight
constexpr int kTileMaxIn = 32;                          // inputs of a first layer
constexpr int kTileHeadBias = 8;                        // staged head-bias floats (the squashed head: 2 x 4 outputs)

struct PolicyNet {
    const float* w[kPolicyLinear];
    const float* b[kPolicyLinear];
    int32_t S, H, nh, O, act;                           // input width, hidden width, hidden layers, head outputs, TG_ACT_*
};

__device__ static inline uint4 lds_u4(const uint4* __restrict__ p) { return *p; }
__device__ static inline float4 lds_f4(const float* __restrict__ p) { return *reinterpret_cast<const float4*>(p); }
__device__ static inline float lds_f(const float* __restrict__ p) { return *p; }

// Layer l's weight / bias pointer of the workgroup's net, for kernel arguments that lead with `PolicyNet net[2]` (actor, critic).
// A run-time index into a local copy of the tables puts it into scratch: uniform selects over the kernel arguments themselves
// instead (l and `critic` are workgroup-uniform).
template <typename Args>
__device__ static inline const float* net_weight(const Args& a, bool critic, int l) {
    const float* r = critic ? a.net[1].w[0] : a.net[0].w[0];
#pragma unroll
    for (int q = 1; q < kPolicyLinear; ++q) r = l == q ? (critic ? a.net[1].w[q] : a.net[0].w[q]) : r;
    return r;
}
template <typename Args>
__device__ static inline const float* net_bias(const Args& a, bool critic, int l) {
    const float* r = critic ? a.net[1].b[0] : a.net[0].b[0];
#pragma unroll
    for (int q = 1; q < kPolicyLinear; ++q) r = l == q ? (critic ? a.net[1].b[q] : a.net[0].b[q]) : r;
    return r;
}

// f(width, activation) with both as std::integral_constant: the six (H, activation) bodies of a kernel behind one
// workgroup-uniform switch
template <typename F>
__device__ __attribute__((always_inline)) static inline void dispatch_width_act(int H, int act, F&& f) {
    using Relu = std::integral_constant<int, TG_ACT_RELU>;
    using Tanh = std::integral_constant<int, TG_ACT_TANH>;
    const bool tanh_net = act == TG_ACT_TANH;
    if (H == 64) {
        if (tanh_net) f(std::integral_constant<int, 64>{}, Tanh{}); else f(std::integral_constant<int, 64>{}, Relu{});
    } else if (H == 128) {
        if (tanh_net) f(std::integral_constant<int, 128>{}, Tanh{}); else f(std::integral_constant<int, 128>{}, Relu{});
    } else {
        if (tanh_net) f(std::integral_constant<int, 256>{}, Tanh{}); else f(std::integral_constant<int, 256>{}, Relu{});
    }
}

// a net's resident tables in LDS, in the order they are staged; K4 = ceil(K / 4) first-layer steps
template <int H>
struct NetTables {
    float* w0;                                          // [H / 16][K4][64 lanes]: lane (i, g) of step s holds W0[16 mo + i][4 s + g]
    float* bias;                                        // [nh][H]
    float* wh;                                          // [O][H]
    float* bh;                                          // [kTileHeadBias]
    __device__ NetTables(float* base, int K4, int nh, int O) : w0(base), bias(w0 + H / 16 * K4 * 64), wh(bias + nh * H), bh(wh + O * H) {}
};

// staged by the whole workgroup: the first layer (K inputs) in operand order, zero-padded to K4 steps; the biases (`bias_of(l)`:
// layer l's); the head.  The caller's barrier follows.
template <int H, typename BiasOf>
__device__ __attribute__((always_inline)) static inline void stage_net_tables(const float* w0, const int K, const int nh, const int O,
                                                                              BiasOf&& bias_of, const float* Wh, const float* Bh,
                                                                              float* dst, const int tid) {
    constexpr int NT = H / 16, WPW = kTileWaves;
    const int K4 = (K + 3) >> 2;
    const NetTables<H> tb(dst, K4, nh, O);
    for (int q = tid; q < NT * K4 * 64; q += 64 * WPW) {
        const int ln = q & 63, ps = q >> 6, mo = ps / K4, s = ps - mo * K4;
        const int k = 4 * s + (ln >> 4);
        const bool in = k < K;
        const float v = w0[(16 * mo + (ln & 15)) * K + (in ? k : 0)];
        tb.w0[q] = in ? v : 0.f;
    }
    for (int l = 0; l < nh; ++l) {
        const float* bl = bias_of(l);
        for (int q = tid; q < H; q += 64 * WPW) tb.bias[l * H + q] = bl[q];
    }
    for (int q = tid; q < O * H; q += 64 * WPW) tb.wh[q] = Wh[q];
    const float bv = Bh[tid < O ? tid : 0];
    if (tid < kTileHeadBias) tb.bh[tid] = tid < O ? bv : 0.f;
}

// the wave's pieces of one forward ring block; `src`: the lane's 16 bytes of piece 0, W + (16 mo + j) H + 4 g
template <int NT>
__device__ __attribute__((always_inline)) static inline void ring_dma_rows(const float* src, uint4* slot, const int wave) {
#pragma unroll
    for (int q = 0; q < NT / kTileWaves; ++q) {
        const int piece = q * kTileWaves + wave;
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint4*>(src + 16 * piece), (lds_void*)(slot + piece * 64), 16, 0, 0);
    }
}

template <int kAct>
__device__ static inline void act4(f32x4& v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = act_f32<kAct>(v[r]);
}

// one 16-feature output tile against a whole H-wide operand (mlp_f32_wide.hip's tile_products): two accumulator chains, the A
// operands of pieces t + 2, t + 3 requested before the products of pieces t, t + 1; the block's DMA successor is issued behind
// the first reads
template <int NT, typename DmaNext>
__device__ __attribute__((always_inline)) static inline f32x4 tile_products(const uint4* __restrict__ cur, const int lane,
                                                                            const f32x4 (&xin)[NT], f32x4 acc, DmaNext&& dma_next) {
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
    return acc + acc1;                                                // (a fixed order: deterministic)
}

// layer 0 from the staged first layer: lane group g's xr[s] is input 4 s + g of the lane's row, zero past the width.
// on_tile(0, mo, acc) sees every finished tile.
template <int H, int kAct, typename OnTile>
__device__ __attribute__((always_inline)) static inline void first_layer(const float* w0_s, const float* bias_s, const int K4, const int lane,
                                                                         const float (&xr)[kTileMaxIn / 4], f32x4 (&xin)[H / 16],
                                                                         OnTile&& on_tile) {
    constexpr int NT = H / 16;
    const int g = lane >> 4;
#pragma unroll
    for (int mo = 0; mo < NT; ++mo) {
        const float4 b4 = lds_f4(bias_s + 16 * mo + 4 * g);
        f32x4 acc = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int s = 0; s < kTileMaxIn / 4; ++s)
            if (s < K4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(lds_f(w0_s + (mo * K4 + s) * 64 + lane), xr[s], acc, 0, 0, 0);
        act4<kAct>(acc);
        xin[mo] = acc;
        on_tile(0, mo, acc);
    }
}

// the n_hh hidden H x H layers, one ring block per 16 output features; xin: layer 0's output in, the top hidden layer's out.
// on_tile(l, mo, acc) sees every finished tile.
template <int H, int kAct, typename DmaNext, typename OnTile>
__device__ __attribute__((always_inline)) static inline void hidden_layers(const uint4* ring, int& cur_slot, const float* bias_s, const int n_hh,
                                                                           const int lane, f32x4 (&xin)[H / 16], DmaNext&& dma_next,
                                                                           OnTile&& on_tile) {
    constexpr int NT = H / 16, D = kTileD, P = kTileP, SLOT = NT * 64;
    // counted wait for the block about to be consumed: behind its DMA there are always the pieces of the P - 1 later blocks.  The
    // loads and stores of a round (inputs, outputs, on_tile's) are issued behind them too and are NOT counted: stricter, never weaker.
    constexpr int kWait = (P - 1) * (NT / kTileWaves);
    const int g = lane >> 4;
    f32x4 xout[NT];
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
            f32x4 acc = tile_products<NT>(cur, lane, xin, f32x4{b4.x, b4.y, b4.z, b4.w}, dma_next);
            act4<kAct>(acc);
            xout[mo] = acc;
            on_tile(l, mo, acc);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) xin[t] = xout[t];
    }
}

// head output k: an fp32 dot product over the lane's features, the four lane groups added in a fixed order (mlp_f32_wide.hip's).
// A head row is addressed in LDS by a uniform run-time index: the squashed head's log-std rows A .. 2 A - 1 need no run-time
// index into a register array.
template <int NT>
__device__ __attribute__((always_inline)) static inline float head_out(const float* wh_s, const float* bh_s, const f32x4 (&xin)[NT],
                                                                       const int k, const int g) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float4 w = lds_f4(wh_s + k * (16 * NT) + 16 * t + 4 * g);
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
}

// The whole forward of a workgroup on one net of `a` (`second`: a.net[1]) with K inputs: the ring's prefetch cursor, the resident
// tables, and per round of 64 rows
//   inputs(row, rowc, valid, xr)          fills the lane's first-layer operands: xr[s] = input 4 s + g of its row, zero past K
//   on_tile(row, valid, l, mo, acc)       sees every finished hidden tile (the activation stores)
//   epilogue(row, rowc, valid, xin, tb)   the head and what follows it, on the top hidden layer's tiles
// rowc is the row clamped into the batch (no load under a branch), valid says whether the lane's row exists.
template <int H, int kAct, typename Args, typename Inputs, typename OnTile, typename Epilogue>
__device__ __attribute__((always_inline)) static inline void forward_tiles(const Args& a, const bool second, const int K, const int nh,
                                                                           const int O, uint4* lds, Inputs&& inputs, OnTile&& on_tile,
                                                                           Epilogue&& epilogue) {
    constexpr int NT = H / 16, D = kTileD, P = kTileP, SLOT = NT * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int n_hh = nh - 1, K4 = (K + 3) >> 2;
    uint4* ring = lds;
    const NetTables<H> tb(reinterpret_cast<float*>(ring + D * SLOT), K4, nh, O);
    const int64_t rows = a.rows;
    const int64_t n_rounds = (rows + 63) / 64;

    int pre_l = 1, pre_mo = 0, pre_slot = 0, cur_slot = 0;
    auto dma_next = [&]() {
        ring_dma_rows<NT>(net_weight(a, second, pre_l) + ((16 * pre_mo + j) * H + 4 * g), ring + pre_slot * SLOT, wave);
        pre_mo = (pre_mo + 1 == NT) ? 0 : pre_mo + 1;
        pre_l = pre_mo != 0 ? pre_l : (pre_l == n_hh ? 1 : pre_l + 1);
        pre_slot = (pre_slot + 1 == D) ? 0 : pre_slot + 1;
    };
    if (n_hh > 0) {
#pragma unroll
        for (int b = 0; b < P; ++b) dma_next();
    }
    stage_net_tables<H>(net_weight(a, second, 0), K, nh, O, [&](int l) { return net_bias(a, second, l); }, net_weight(a, second, nh),
                        net_bias(a, second, nh), tb.w0, tid);
    __syncthreads();                                                  // (the tables; drains the prologue's DMA too: once)

    for (int64_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const int64_t row = round * 64 + wave * 16 + j;
        const bool valid = row < rows;
        const int64_t rowc = valid ? row : rows - 1;
        f32x4 xin[NT];
        float xr[kTileMaxIn / 4];
        inputs(row, rowc, valid, xr);
        auto tile = [&](int l, int mo, const f32x4& v) { on_tile(row, valid, l, mo, v); };
        first_layer<H, kAct>(tb.w0, tb.bias, K4, lane, xr, xin, tile);
        hidden_layers<H, kAct>(ring, cur_slot, tb.bias, n_hh, lane, xin, dma_next, tile);
        epilogue(row, rowc, valid, xin, tb);
    }
    // the ring's prefetches of a round that never came: let them land before the workgroup's LDS goes away
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- sampling and density: the rollout kernels' float32 Box-Muller (fused_rollout_f32.hip) on one Philox draw, and the terms of
//      logp, one float32 rounding per operation -----------------------------------------------------------------------------------
__device__ static inline void box_muller_eps(const uint32_t (&rnd)[4], const int A, float (&eps)[4]) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        eps[2 * hh] = eps[2 * hh + 1] = 0.f;
        if (2 * hh < A) {
            const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(Philox::u01(rnd[2 * hh])));
            const float rev = Philox::u01(rnd[2 * hh + 1]);
            eps[2 * hh] = rad * __builtin_amdgcn_cosf(rev);
            eps[2 * hh + 1] = rad * __builtin_amdgcn_sinf(rev);
        }
    }
}
// log N(mu + exp(ls) e; mu, exp(ls)) of one dimension: -0.5 e^2 - ls - 0.5 log 2 pi
__device__ static inline float gaussian_logp_term(float e, float ls) {
    return rn_sub(rn_sub(rn_mul(-0.5f, rn_mul(e, e)), ls), 0.91893853320467274f);
}
// what a = tanh(u) takes off it: log(1 - a^2 + 1e-6)
__device__ static inline float squash_logp_term(float act) { return logf(rn_add(rn_sub(1.0f, rn_mul(act, act)), 1e-6f)); }

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// what every entry refuses about a net; `outs`: the head outputs the caller expects; `pointers`: the launches (the entries that
// only size things read the widths alone)
static int policy_net_check(const char* who, const char* name, const tg_policy_net* n, int outs, bool pointers, PolicyNet& out) {
    TG_REQUIRE(n != nullptr, "%s: the %s table is null", who, name);
    TG_REQUIRE(n->n_layers >= 2 && n->n_layers <= kPolicyLinear, "%s: %s has %d Linear layers, outside 2..%d (1..%d hidden layers)", who,
               name, n->n_layers, kPolicyLinear, kPolicyLinear - 1);
    TG_REQUIRE(n->activation == TG_ACT_RELU || n->activation == TG_ACT_TANH, "%s: %s has an unknown hidden activation %d", who, name,
               n->activation);
    const int L = n->n_layers, S = n->in_dim[0], H = n->out_dim[0], O = n->out_dim[L - 1];
    TG_REQUIRE(S >= 1 && S <= kTileMaxIn, "%s: %s has input width %d outside [1, %d]", who, name, S, kTileMaxIn);
    TG_REQUIRE(H == 64 || H == 128 || H == 256, "%s: %s has hidden width %d (64, 128 or 256)", who, name, H);
    for (int l = 0; l < L; ++l) {
        TG_REQUIRE((l == 0 || n->in_dim[l] == H) && (l == L - 1 || n->out_dim[l] == H), "%s: %s layer %d is %d -> %d, hidden width %d", who,
                   name, l, n->in_dim[l], n->out_dim[l], H);
        if (pointers) {
            TG_REQUIRE(n->w[l] && n->b[l], "%s: %s layer %d has a null weight or bias", who, name, l);
            // the H x H layers are read 16 bytes at a time, everything else as floats
            const uintptr_t mask = (l > 0 && l < L - 1) ? 15 : 3;
            TG_REQUIRE(((uintptr_t)n->w[l] & mask) == 0 && ((uintptr_t)n->b[l] & 3) == 0,
                       "%s: %s layer %d has a misaligned weight or bias pointer", who, name, l);
        }
        out.w[l] = n->w[l];
        out.b[l] = n->b[l];
    }
    for (int l = L; l < kPolicyLinear; ++l) { out.w[l] = n->w[0]; out.b[l] = n->b[0]; }
    TG_REQUIRE(O == outs, "%s: %s has %d head outputs, %d expected", who, name, O, outs);
    out.S = S; out.H = H; out.nh = L - 1; out.O = O; out.act = n->activation;
    return TG_OK;
}

// LDS of a workgroup that runs one net: the ring and the net's tables
static size_t ring_tables_lds_bytes(const PolicyNet& n) {
    const int NT = n.H / 16, K4 = (n.S + 3) / 4;
    return (size_t)kTileD * NT * 1024 + (size_t)NT * K4 * 256 + (size_t)(n.nh + n.O) * n.H * 4 + kTileHeadBias * 4;
}

// one workgroup per 64 rows, at most `grid_limit` of them (<= 0: per_cu workgroups per CU), `nets` as grid dimension y
template <typename K, typename Args>
static int launch_row_tiles(const char* who, K kernel, LdsOptIn& opt_in, const Args& args, int nets, size_t shmem, int32_t grid_limit,
                            int per_cu, hipStream_t st) {
    if (int rc = reserve_dynamic_lds((const void*)kernel, shmem, opt_in, who)) return rc;
    const int64_t tiles = ceil_div(args.rows, 64);
    const int64_t cap = grid_limit > 0 ? grid_limit : (int64_t)per_cu * device_cus();
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles < cap ? tiles : cap), (unsigned)nets), dim3(64 * kTileWaves), shmem, st, args);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

}  // namespace tg
