// Rollout storage for gfx950 (tg_segment_push, tg_segment_gae, tg_segment_permute, tg_segment_gather): fixed-length on-policy segments
// of a vector env -- one launch per stored step, one for GAE over the segment, one for a fresh permutation of its rows, one per
// gathered minibatch.  The rule is stated in include/trajopt_grpo_hip.h (tg_segment) and, element by element, in
// tests/segment_ref.py; every float32 operation is rounded on its own, so the NumPy restatement is bit for bit.
//
// Push and gather: ONE WAVE PER WORKGROUP, 64 slots (rows) per wave.  A wave's piece of an [n][W] array is one run of 64 W
// consecutive floats.  On the caller's side that run starts 16-byte aligned (the wave's first slot is a multiple of 64); on the
// storage side it starts at float (t n + s0) W, which need not be a multiple of 4.  The shift happens in LDS: 16-byte loads from
// the caller's side land at lds[phase + .], and the run leaves as 16-byte loads from lds[4 j] to 16-byte aligned stores -- whole
// lines on both global sides, the ragged first and last group float by float.  Only wave_lds_sync (row_store.hpp) orders the two
// halves: no workgroup barrier anywhere in this file but the permutation's counter.
// GAE: one lane per slot walks its column backwards; the loads of time steps t - kGaePrefetch .. t - 1 are in flight while the
// recurrence of steps t .. t + kGaePrefetch - 1 runs, so the dependent chain is four float32 operations per step and no memory
// round trip.  Lanes of a wave read 64 consecutive floats of a time row.
// Byte offsets into the storage are 64-bit throughout.
#include "tg_common.hpp"
#include "row_store.hpp"

#include <stdint.h>

namespace tg {

constexpr int kSegSlots = TG_SEGMENT_SLOTS;            // slots of a push / GAE / gather workgroup: one wave
constexpr int kSegMaxObs = 32, kSegMaxAct = 8;
constexpr int kSegLds = 64 * kSegMaxObs + 4;           // floats: a wave's widest run and the shift
constexpr int kGaePrefetch = TG_SEGMENT_GAE_PREFETCH;
constexpr int kPermBlock = TG_SEGMENT_PERMUTE_BLOCK;
static_assert(kSegSlots == kWave, "a push workgroup is one wave: wave_lds_sync is its only barrier");

// dst[d0 .. d0 + len) = src[0 .. len) through the wave's LDS region.  src and dst are 16-byte aligned, d0 is any float offset.
__device__ static inline void run_copy_staged(float* __restrict__ dst, int64_t d0, const float* __restrict__ src, int len, float* lds) {
    const int lane = threadIdx.x;
    const int phase = (int)(d0 & 3);
    for (int g = lane; 4 * g < len; g += kSegSlots) {
        if (4 * g + 4 <= len) {
            const float4 v = *reinterpret_cast<const float4*>(src + 4 * g);
            float* p = lds + phase + 4 * g;
            p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        } else {
            for (int k = 4 * g; k < len; ++k) lds[phase + k] = src[k];
        }
    }
    wave_lds_sync();
    float* __restrict__ out = dst + (d0 - phase);                          // 16-byte aligned
    const int end = phase + len;
    for (int j = lane; 4 * j < end; j += kSegSlots) {
        if (4 * j >= phase && 4 * j + 4 <= end) {
            *reinterpret_cast<float4*>(out + 4 * j) = *reinterpret_cast<const float4*>(lds + 4 * j);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = 4 * j + k;
                if (e >= phase && e < end) out[e] = lds[e];
            }
        }
    }
    wave_lds_sync();                                                        // (the region is free for the next run)
}

__global__ __launch_bounds__(kSegSlots) void segment_push_kernel(tg_segment s, const float* __restrict__ actions,
                                                                  const float* __restrict__ logp, const float* __restrict__ value,
                                                                  const float* __restrict__ obs, const float* __restrict__ reward,
                                                                  const uint8_t* __restrict__ terminated,
                                                                  const uint8_t* __restrict__ truncated,
                                                                  const float* __restrict__ final_value) {
    __shared__ float4 seg_lds[kSegLds / 4];
    float* lds = reinterpret_cast<float*>(seg_lds);
    const int lane = threadIdx.x;
    const int64_t n = s.n;
    const int64_t s0 = (int64_t)blockIdx.x * kSegSlots;                    // the wave's first slot
    const int slots = (int)(n - s0 < kSegSlots ? n - s0 : kSegSlots);
    const int S = s.obs_dim, A = s.act_dim, L = s.steps;
    int t = s.d_step[s0];                                                   // every store below depends on it: read before any write
    t = (uint32_t)t < (uint32_t)L ? t : 0;                                  // (a counter outside the segment never becomes an address)

    // ---- row 0 is the one row a segment's own last push overwrites: step 0 keeps a copy of it for the minibatches ----
    if (t == 0) run_copy_staged(s.d_first_obs, s0 * S, s.d_obs + s0 * S, slots * S, lds);
    // ---- obs -> row t + 1 (and the last push of a segment also -> row 0: the next segment starts with no launch), act -> row t ----
    run_copy_staged(s.d_obs, ((int64_t)(t + 1) * n + s0) * S, obs + s0 * S, slots * S, lds);
    if (t + 1 == L) run_copy_staged(s.d_obs, s0 * S, obs + s0 * S, slots * S, lds);
    run_copy_staged(s.d_act, ((int64_t)t * n + s0) * A, actions + s0 * A, slots * A, lds);

    // ---- per slot: logp, val, the flags and the effective reward, then the slot's step counter ----
    if (lane < slots) {
        const int64_t i = s0 + lane, row = (int64_t)t * n + i;
        const bool term = terminated[i] != 0, trunc = truncated[i] != 0;
        const float rw = reward[i];
        float eff = rw;
        if (trunc && !term) eff = rn_add(rw, rn_mul(s.gamma, final_value[i]));   // a select: final_value is garbage elsewhere
        s.d_logp[row] = logp[i];
        s.d_val[row] = value[i];
        s.d_rew[row] = eff;
        s.d_flags[row] = (uint8_t)((term ? 1 : 0) | (trunc ? 2 : 0));
        s.d_step[i] = t + 1 == L ? 0 : t + 1;
    }
}

// One step of the recurrence (the arithmetic of tools/vec_env_ppo.py's torch loop, operation by operation).
__device__ static inline void gae_step(float g, float c, float rew, float val, uint8_t flags, float& nxt, float& adv, float& ret) {
    const float live = flags ? 0.0f : 1.0f;
    const float delta = rn_sub(rn_add(rew, rn_mul(rn_mul(g, nxt), live)), val);
    adv = rn_add(delta, rn_mul(rn_mul(c, live), adv));
    ret = rn_add(adv, val);
    nxt = val;
}

struct GaeOperands { float rew[kGaePrefetch], val[kGaePrefetch]; uint8_t flags[kGaePrefetch]; };

// the operands of steps top - 1, top - 2, .., top - kGaePrefetch, all of them inside the segment: loads without a branch, so the
// wait in front of their first use counts exactly the memory operations issued behind them
__device__ static inline void gae_request(const tg_segment& s, int64_t i, int top, GaeOperands& o) {
#pragma unroll
    for (int k = 0; k < kGaePrefetch; ++k) {
        const int64_t row = (int64_t)(top - 1 - k) * s.n + i;
        o.rew[k] = s.d_rew[row];
        o.val[k] = s.d_val[row];
        o.flags[k] = s.d_flags[row];
    }
}

__global__ __launch_bounds__(kSegSlots) void segment_gae_kernel(tg_segment s, const float* __restrict__ last_value) {
    const int64_t i = (int64_t)blockIdx.x * kSegSlots + threadIdx.x;
    if (i >= s.n) return;
    const float g = s.gamma, c = s.gamma_lam;
    float nxt = last_value[i], adv = 0.0f, ret;
    int top = s.steps;
    // the ragged head, steps % kGaePrefetch steps one at a time: what is left is whole groups of kGaePrefetch
    for (int k = top % kGaePrefetch; k > 0; --k) {
        const int64_t row = (int64_t)--top * s.n + i;
        gae_step(g, c, s.d_rew[row], s.d_val[row], s.d_flags[row], nxt, adv, ret);
        s.d_adv[row] = adv;
        s.d_ret[row] = ret;
    }
    if (top == 0) return;
    GaeOperands cur, ahead;
    gae_request(s, i, top, cur);
    // The first group is waited for HERE, once (vmcnt(0); expcnt and lgkmcnt untouched).  Entered with loads pending, the loop's head
    // would need a wait that the back edge inherits -- there it waits for the previous trip's stores, a round trip per group.
    // gfx9 S_WAITCNT immediate: vmcnt = bits [3:0] and [15:14], expcnt = [6:4], lgkmcnt = [11:8]; 0x0F70 is vmcnt 0 with expcnt 7 and
    // lgkmcnt 15 (their maxima: no wait).  Results do not depend on it, only the schedule: with the compiler this was written on,
    // the loop's own waits are vmcnt(32) / (17) / (16) at the end of a trip (profiles/r23_segment_probe.md).  That figure is one
    // compiler's output: after a compiler change read it again from the assembly (--save-temps) before quoting it.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    for (; top > 0; top -= kGaePrefetch) {
        // the group behind this one is in flight while this one is consumed (the last trip asks for its own group again: no branch)
        gae_request(s, i, top > kGaePrefetch ? top - kGaePrefetch : top, ahead);
#pragma unroll
        for (int k = 0; k < kGaePrefetch; ++k) {
            gae_step(g, c, cur.rew[k], cur.val[k], cur.flags[k], nxt, adv, ret);
            const int64_t row = (int64_t)(top - 1 - k) * s.n + i;
            s.d_adv[row] = adv;
            s.d_ret[row] = ret;
        }
        cur = ahead;
    }
}

// The permutation of [0, rows): a balanced Feistel network on `bits` bits (even, the smallest with 2^bits >= rows), four rounds,
// round function = word 0 of Philox(key = seed, counter = (half, round, ordinal lo, ordinal hi)) masked to bits / 2 bits, and a
// cycle walk back into [0, rows).  The network is a bijection of [0, 2^bits) and the walk starts inside [0, rows), so the walk
// returns there: the loop ends, and the map restricted to [0, rows) is a bijection of it.
__device__ static inline uint32_t feistel(uint32_t x, int half, uint64_t seed, uint64_t ordinal) {
    const uint32_t mask = (1u << half) - 1u;
    uint32_t l = x >> half, r = x & mask;
#pragma unroll
    for (uint32_t round = 0; round < 4; ++round) {
        uint32_t w[4];
        Philox::draw(seed, ((uint64_t)round << 32) | r, (uint32_t)ordinal, (uint32_t)(ordinal >> 32), w);
        const uint32_t nr = l ^ (w[0] & mask);
        l = r;
        r = nr;
    }
    return (l << half) | r;
}

__global__ __launch_bounds__(kPermBlock) void segment_permute_kernel(tg_segment s, int64_t rows, int half) {
    const uint64_t ordinal = s.d_shuffles[blockIdx.x];                      // a workgroup's own copy of the counter: no other reads it
    const int64_t i = (int64_t)blockIdx.x * kPermBlock + threadIdx.x;
    if (i < rows) {
        uint32_t y = (uint32_t)i;
        do { y = feistel(y, half, s.seed, ordinal); } while ((int64_t)y >= rows);
        s.d_idx[i] = (int64_t)y;
    }
    __syncthreads();                                                        // every lane holds the ordinal: now it may move on
    if (threadIdx.x == 0) s.d_shuffles[blockIdx.x] = ordinal + 1;
}

struct SegBatch {
    float* obs;              // [B][S]
    float* act;              // [B][A]
    float* logp;
    float* adv;
    float* ret;
    float* val;
};

// Rows rows_lds[0 .. count) of a row-major [.][W] array (-1: a row of NaNs) -> dst[0 .. count W), 16-byte aligned: gathered into the
// wave's LDS region, 16 bytes per lane where a row is a whole number of them, and left as in run_copy_staged.  Rows below `head_rows`
// are read from `head` instead of `src` (the observations of step 0: see the push).
__device__ static inline void gather_rows_staged(float* __restrict__ dst, const float* __restrict__ src, const float* __restrict__ head,
                                                 int64_t head_rows, int W, int count, const int64_t* rows_lds, float* lds) {
    const int lane = threadIdx.x;
    const float nan = __builtin_nanf("");
    const int len = count * W;
    if ((W & 3) == 0) {
        const int per = W >> 2;
        for (int q = lane; 4 * q < len; q += kSegSlots) {
            const int r = (int)((uint32_t)q / (uint32_t)per), k = q - r * per;
            const int64_t from = rows_lds[r];
            float4 v = make_float4(nan, nan, nan, nan);
            if (from >= 0) v = *reinterpret_cast<const float4*>((from < head_rows ? head : src) + from * W + 4 * k);
            *reinterpret_cast<float4*>(lds + 4 * q) = v;
        }
    } else {
        for (int e = lane; e < len; e += kSegSlots) {
            const int r = (int)((uint32_t)e / (uint32_t)W);
            const int64_t from = rows_lds[r];
            lds[e] = from >= 0 ? (from < head_rows ? head : src)[from * W + (e - r * W)] : nan;
        }
    }
    wave_lds_sync();
    for (int j = lane; 4 * j < len; j += kSegSlots) {
        if (4 * j + 4 <= len) {
            *reinterpret_cast<float4*>(dst + 4 * j) = *reinterpret_cast<const float4*>(lds + 4 * j);
        } else {
            for (int e = 4 * j; e < len; ++e) dst[e] = lds[e];
        }
    }
    wave_lds_sync();
}

__global__ __launch_bounds__(kSegSlots) void segment_gather_kernel(tg_segment s, int64_t rows, int64_t first, int64_t count, SegBatch out) {
    __shared__ float4 seg_lds[kSegLds / 4];
    float* lds = reinterpret_cast<float*>(seg_lds);
    const int lane = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * kSegSlots;                    // the wave's first row of the minibatch
    const int here = (int)(count - b0 < kSegSlots ? count - b0 : kSegSlots);
    __shared__ int64_t seg_rows[kSegSlots];
    int64_t row = -1;
    if (lane < here) {
        row = s.d_idx[first + b0 + lane];
        if ((uint64_t)row >= (uint64_t)rows) row = -1;                      // (an index outside the segment is not read)
    }
    seg_rows[lane] = row;
    wave_lds_sync();
    const int S = s.obs_dim, A = s.act_dim;
    gather_rows_staged(out.obs + b0 * S, s.d_obs, s.d_first_obs, s.n, S, here, seg_rows, lds);
    gather_rows_staged(out.act + b0 * A, s.d_act, s.d_act, 0, A, here, seg_rows, lds);
    if (lane < here) {
        const float nan = __builtin_nanf("");
        const bool ok = row >= 0;
        out.logp[b0 + lane] = ok ? s.d_logp[row] : nan;
        out.adv[b0 + lane] = ok ? s.d_adv[row] : nan;
        out.ret[b0 + lane] = ok ? s.d_ret[row] : nan;
        out.val[b0 + lane] = ok ? s.d_val[row] : nan;
    }
}

// what the four entries refuse about the object itself
static int segment_check(const char* who, const tg_segment* s) {
    TG_REQUIRE(s && s->d_obs && s->d_act && s->d_logp && s->d_val && s->d_rew && s->d_flags && s->d_adv && s->d_ret && s->d_idx &&
               s->d_step && s->d_shuffles && s->d_first_obs, "%s: null pointer", who);
    TG_REQUIRE(s->n > 0 && s->steps > 0, "%s: bad sizes n=%lld steps=%d", who, (long long)s->n, s->steps);
    TG_REQUIRE(((int64_t)s->steps + 1) * s->n < ((int64_t)1 << 31), "%s: (steps %d + 1) x n %lld rows >= 2^31", who, s->steps,
               (long long)s->n);
    TG_REQUIRE(s->gamma > 0.0f && s->gamma <= 1.0f && s->gamma_lam > 0.0f && s->gamma_lam <= 1.0f,
               "%s: gamma=%g or gamma_lam=%g outside (0, 1]", who, (double)s->gamma, (double)s->gamma_lam);
    if (s->obs_dim < 1 || s->obs_dim > kSegMaxObs || s->act_dim < 1 || s->act_dim > kSegMaxAct)
        return set_error(TG_ERR_UNSUPPORTED, "%s: obs_dim=%d outside [1, %d] or act_dim=%d outside [1, %d]", who, s->obs_dim, kSegMaxObs,
                         s->act_dim, kSegMaxAct);
    TG_REQUIRE((((uintptr_t)s->d_obs | (uintptr_t)s->d_act | (uintptr_t)s->d_first_obs) & 15) == 0,
               "%s: d_obs, d_act and d_first_obs must be 16-byte aligned", who);
    return TG_OK;
}

// the width of the Feistel network for `rows` rows: even, at least 2, the smallest with 2^bits >= rows
static int permute_bits(int64_t rows) {
    int bits = 2;
    while (((int64_t)1 << bits) < rows) bits += 2;
    return bits;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_segment_push(const tg_segment* s, const float* d_actions, const float* d_logp, const float* d_value, const float* d_obs_in,
                    const float* d_reward, const uint8_t* d_terminated, const uint8_t* d_truncated, const float* d_final_value,
                    void* stream) {
    const char* who = "tg_segment_push";
    if (int rc = segment_check(who, s)) return rc;
    TG_REQUIRE(d_actions && d_logp && d_value && d_obs_in && d_reward && d_terminated && d_truncated && d_final_value,
               "%s: null pointer", who);
    TG_REQUIRE((((uintptr_t)d_actions | (uintptr_t)d_obs_in) & 15) == 0, "%s: d_actions and d_obs_in must be 16-byte aligned", who);
    hipLaunchKernelGGL(segment_push_kernel, dim3((unsigned)ceil_div(s->n, kSegSlots)), dim3(kSegSlots), 0, (hipStream_t)stream, *s,
                       d_actions, d_logp, d_value, d_obs_in, d_reward, d_terminated, d_truncated, d_final_value);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

int tg_segment_gae(const tg_segment* s, const float* d_last_value, void* stream) {
    const char* who = "tg_segment_gae";
    if (int rc = segment_check(who, s)) return rc;
    TG_REQUIRE(d_last_value != nullptr, "%s: null pointer", who);
    hipLaunchKernelGGL(segment_gae_kernel, dim3((unsigned)ceil_div(s->n, kSegSlots)), dim3(kSegSlots), 0, (hipStream_t)stream, *s,
                       d_last_value);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

int tg_segment_permute(const tg_segment* s, void* stream) {
    const char* who = "tg_segment_permute";
    if (int rc = segment_check(who, s)) return rc;
    const int64_t rows = (int64_t)s->steps * s->n;
    hipLaunchKernelGGL(segment_permute_kernel, dim3((unsigned)ceil_div(rows, kPermBlock)), dim3(kPermBlock), 0, (hipStream_t)stream, *s,
                       rows, permute_bits(rows) / 2);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

int tg_segment_gather(const tg_segment* s, int64_t first, int64_t count, float* o_obs, float* o_act, float* o_logp, float* o_adv,
                      float* o_ret, float* o_val, void* stream) {
    const char* who = "tg_segment_gather";
    if (int rc = segment_check(who, s)) return rc;
    TG_REQUIRE(o_obs && o_act && o_logp && o_adv && o_ret && o_val, "%s: null pointer", who);
    const int64_t rows = (int64_t)s->steps * s->n;
    TG_REQUIRE(first >= 0 && count > 0 && first + count <= rows, "%s: rows [%lld, %lld + %lld) outside the segment's %lld", who,
               (long long)first, (long long)first, (long long)count, (long long)rows);
    TG_REQUIRE((((uintptr_t)o_obs | (uintptr_t)o_act) & 15) == 0, "%s: o_obs and o_act must be 16-byte aligned", who);
    const SegBatch out{o_obs, o_act, o_logp, o_adv, o_ret, o_val};
    hipLaunchKernelGGL(segment_gather_kernel, dim3((unsigned)ceil_div(count, kSegSlots)), dim3(kSegSlots), 0, (hipStream_t)stream, *s,
                       rows, first, count, out);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

}  // extern "C"
