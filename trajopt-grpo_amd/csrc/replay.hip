// Replay buffer for gfx950 (tg_replay_start, tg_replay_push, tg_replay_sample): n-step transitions of a vector env, one streaming
// launch per push and one gather launch per sampled batch.  The rule is stated in include/trajopt_grpo_hip.h (tg_replay) and, element
// by element, in tests/replay_ref.py; the arithmetic is one float32 multiply and one float32 add per extended row, each rounded on its
// own, so the NumPy restatement is bit for bit.
//
// Push: a block owns kReplaySlots consecutive env slots and everything of them -- their piece of the time slot's contiguous [n][.]
// blocks, their rows of rew / disc / nstep, their entries of cursor / filled / open / last_obs -- so no two blocks touch the same
// address and one barrier (between reading the per-slot state and writing it) orders a block's own accesses.  The storage side of the
// block copies is written as aligned 16-byte stores; a time slot starts at float c n S, which need not be a multiple of 4, so the
// caller's side of a group of four is a 4-byte-aligned 16-byte access and the ragged ends of a block's piece go float by float.
// Byte offsets into the storage are 64-bit throughout: [K n][S] passes 2^31 bytes at realistic sizes.
#include "tg_common.hpp"

#include <stdint.h>

namespace tg {

constexpr int kReplaySlots = 64;       // env slots of a push block (a multiple of 4: a block's piece of an [n][.] array starts 16-byte aligned)
constexpr int kReplayBlock = 256;
constexpr int kReplayMaxNStep = 16, kReplayMaxObs = 32, kReplayMaxAct = 8;

struct F4 { float v[4]; };
// 16 bytes at a 4-byte aligned address / at a 16-byte aligned one
__device__ static inline F4 load4_any(const float* p) { F4 r; __builtin_memcpy(r.v, p, 16); return r; }
__device__ static inline void store4_any(float* p, const F4& x) { __builtin_memcpy(p, x.v, 16); }
__device__ static inline void store4_aligned(float* p, const F4& x) {
    *reinterpret_cast<float4*>(p) = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
}

// dst[d0 .. d0 + len) = src[0 .. len): dst + (d0 & ~3) is 16-byte aligned, src is a float pointer
__device__ static inline void block_copy(float* __restrict__ dst, int64_t d0, const float* __restrict__ src, int len, int tid) {
    const int phase = (int)(d0 & 3);
    const int groups = (phase + len + 3) >> 2;
    for (int g = tid; g < groups; g += kReplayBlock) {
        const int le = 4 * g - phase;                                       // the group's first float within the piece
        if (le >= 0 && le + 4 <= len) {
            store4_aligned(dst + d0 + le, load4_any(src + le));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (le + k >= 0 && le + k < len) dst[d0 + le + k] = src[le + k];
        }
    }
}

__global__ __launch_bounds__(kReplayBlock) void replay_push_kernel(tg_replay r, const float* __restrict__ actions,
                                                                    const float* __restrict__ obs, const float* __restrict__ reward,
                                                                    const uint8_t* __restrict__ terminated,
                                                                    const uint8_t* __restrict__ truncated,
                                                                    const float* __restrict__ final_obs) {
#pragma clang fp contract(off)                                             // rew grows by one multiply and one add, each rounded on its own
    __shared__ uint8_t s_open[kReplaySlots], s_flag[kReplaySlots];        // per slot: open rows; bit 0 terminated, bit 1 truncated
    const int tid = threadIdx.x;
    const int64_t n = r.n;
    const int64_t s0 = (int64_t)blockIdx.x * kReplaySlots;                 // the block's first slot
    const int slots = (int)(n - s0 < kReplaySlots ? n - s0 : kReplaySlots);
    const int S = r.obs_dim, A = r.act_dim, K = r.capacity_steps, N = r.n_step;
    int c = r.d_cursor[s0];
    c = (uint32_t)c < (uint32_t)K ? c : 0;                                  // (a cursor outside the ring never becomes an address)
    int32_t filled_in = 0;
    if (tid < slots) {
        const int32_t o = r.d_open[s0 + tid];
        s_open[tid] = (uint8_t)(o < 0 ? 0 : o > N - 1 ? N - 1 : o);
        s_flag[tid] = (uint8_t)((terminated[s0 + tid] ? 1 : 0) | (truncated[s0 + tid] ? 2 : 0));
        filled_in = r.d_filled[s0 + tid];
    }
    __syncthreads();                                                        // the per-slot state is read; from here on it may be written

    const int64_t row0 = (int64_t)c * n + s0;                               // the block's first row of the time slot
    // ---- the new rows' obs / next_obs, and last_obs: the block's piece is `len` consecutive floats of every [n][S] array ----
    {
        const int len = slots * S;
        const int64_t d0 = row0 * S, l0 = s0 * S;
        float* __restrict__ last = r.d_last_obs + l0;
        const float* __restrict__ ob = obs + l0;
        const float* __restrict__ fo = final_obs + l0;
        const int phase = (int)(d0 & 3);
        const int groups = (phase + len + 3) >> 2;
        for (int g = tid; g < groups; g += kReplayBlock) {
            const int le = 4 * g - phase;
            if (le >= 0 && le + 4 <= len) {
                int slot = (int)((uint32_t)le / (uint32_t)S), rem = le - slot * S;
                bool take[4], any = false;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    take[k] = s_flag[slot] != 0;
                    any = any || take[k];
                    if (++rem == S) { rem = 0; ++slot; }
                }
                const F4 prev = load4_any(last + le), now = load4_any(ob + le);
                F4 nx = now;
                if (any) {                                                  // final_obs is read only where an episode ended
                    const F4 fin = load4_any(fo + le);
#pragma unroll
                    for (int k = 0; k < 4; ++k) nx.v[k] = take[k] ? fin.v[k] : now.v[k];
                }
                store4_aligned(r.d_obs + d0 + le, prev);
                store4_aligned(r.d_next_obs + d0 + le, nx);
                store4_any(last + le, now);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = le + k;
                    if (e >= 0 && e < len) {
                        const float now = ob[e];
                        r.d_obs[d0 + e] = last[e];
                        r.d_next_obs[d0 + e] = s_flag[(uint32_t)e / (uint32_t)S] ? fo[e] : now;
                        last[e] = now;
                    }
                }
            }
        }
        // ---- next_obs of the rows still open: rows ((c - j) mod K) n + i, j = 1 .. open[i], one float per lane, coalesced ----
        if (N > 1) {
            for (int e = tid; e < len; e += kReplayBlock) {
                const int slot = (int)((uint32_t)e / (uint32_t)S), o = s_open[slot];
                if (o > 0) {
                    const float nx = s_flag[slot] ? fo[e] : ob[e];
                    int cj = c;
                    for (int j = 1; j <= o; ++j) {
                        cj = cj == 0 ? K - 1 : cj - 1;
                        r.d_next_obs[((int64_t)cj * n + s0) * S + e] = nx;
                    }
                }
            }
        }
    }
    // ---- the new rows' actions ----
    block_copy(r.d_act, row0 * A, actions + s0 * A, slots * A, tid);

    // ---- per slot: rew / disc / nstep of the new row and of the open ones, then the slot's state ----
    if (tid < slots) {
        const int64_t i = s0 + tid;
        const int o = s_open[tid], flag = s_flag[tid];
        const bool term = (flag & 1) != 0;
        const float rw = reward[i];
        int64_t row = row0 + tid;
        r.d_rew[row] = rw;
        r.d_disc[row] = term ? 0.0f : r.discount[1];
        r.d_nstep[row] = 1;
        int cj = c;
        for (int j = 1; j <= o; ++j) {
            cj = cj == 0 ? K - 1 : cj - 1;
            row = (int64_t)cj * n + i;
            r.d_rew[row] = r.d_rew[row] + r.discount[j] * rw;              // (not contracted: the pragma above)
            r.d_disc[row] = term ? 0.0f : r.discount[j + 1];
            r.d_nstep[row] = (uint8_t)(j + 1);
        }
        r.d_open[i] = flag ? 0 : (o + 1 < N - 1 ? o + 1 : N - 1);
        r.d_cursor[i] = c + 1 == K ? 0 : c + 1;
        const int32_t f = filled_in < 0 ? 0 : filled_in;
        r.d_filled[i] = f + 1 < K ? f + 1 : K;
    }
}

__global__ __launch_bounds__(kReplayBlock) void replay_start_kernel(tg_replay r, const float* __restrict__ obs) {
    const int64_t gid = (int64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    const int64_t total = r.n * r.obs_dim, e = gid * 4;
    if (e + 4 <= total) {
        store4_aligned(r.d_last_obs + e, load4_any(obs + e));
    } else {
        for (int64_t k = e; k < total; ++k) r.d_last_obs[k] = obs[k];
    }
    for (int64_t i = gid; i < r.n; i += (int64_t)gridDim.x * kReplayBlock) r.d_open[i] = 0;
}

struct ReplayBatch {
    float* obs;              // [B][S]
    float* act;              // [B][A]
    float* rew;
    float* next_obs;         // [B][S]
    float* disc;
    int64_t* idx;
};

// L lanes per sampled row (a power of two): lane k of the group reads floats k, k + L, ... of the row, so a group reads the random row
// with adjacent lanes on adjacent floats, and adjacent groups write adjacent rows of the batch-major outputs.  Every lane of a group
// computes the group's draw itself: the lanes run in lockstep, so that costs what one lane's draw costs.
template <int L>
__global__ __launch_bounds__(kReplayBlock) void replay_sample_kernel(tg_replay r, int64_t batch, const int64_t* __restrict__ indices,
                                                                      uint64_t seed, uint64_t ordinal, ReplayBatch out) {
    const int64_t t = (int64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    const int64_t b = t / L;
    const int lane = (int)(t % L);
    if (b >= batch) return;
    const int S = r.obs_dim, A = r.act_dim;
    int32_t filled = r.d_filled[0];
    filled = filled < 0 ? 0 : filled > r.capacity_steps ? r.capacity_steps : filled;
    const uint64_t R = (uint64_t)filled * (uint64_t)r.n;                    // rows stored: < 2^31
    int64_t row;
    if (indices != nullptr) {
        row = indices[b];
    } else {
        uint32_t w[4];
        Philox::draw(seed, (uint64_t)b, (uint32_t)(ordinal >> 32), (uint32_t)ordinal, w);
        row = (int64_t)(((uint64_t)w[0] * R) >> 32);
    }
    const bool ok = (uint64_t)row < R;                                      // (a negative index is a huge unsigned one)
    const float nan = __builtin_nanf("");
    const float* __restrict__ so = r.d_obs + row * S;
    const float* __restrict__ sn = r.d_next_obs + row * S;
    const float* __restrict__ sa = r.d_act + row * A;
    for (int k = lane; k < S; k += L) {
        float x = nan, y = nan;
        if (ok) { x = so[k]; y = sn[k]; }
        out.obs[b * S + k] = x;
        out.next_obs[b * S + k] = y;
    }
    for (int k = lane; k < A; k += L) {
        float x = nan;
        if (ok) x = sa[k];
        out.act[b * A + k] = x;
    }
    if (lane == 0) {
        float x = nan, y = nan;
        if (ok) { x = r.d_rew[row]; y = r.d_disc[row]; }
        out.rew[b] = x;
        out.disc[b] = y;
        out.idx[b] = row;
    }
}

// what the three entries refuse about the object itself
static int replay_check(const char* who, const tg_replay* r) {
    TG_REQUIRE(r && r->d_obs && r->d_act && r->d_next_obs && r->d_rew && r->d_disc && r->d_nstep && r->d_last_obs && r->d_cursor &&
               r->d_filled && r->d_open, "%s: null pointer", who);
    TG_REQUIRE(r->n > 0 && r->capacity_steps > 0, "%s: bad sizes n=%lld capacity_steps=%d", who, (long long)r->n, r->capacity_steps);
    TG_REQUIRE(r->n_step >= 1 && r->n_step <= kReplayMaxNStep, "%s: n_step=%d outside [1, %d]", who, r->n_step, kReplayMaxNStep);
    TG_REQUIRE(r->capacity_steps >= r->n_step, "%s: capacity_steps=%d < n_step=%d (a row must not be extended after the ring took it back)",
               who, r->capacity_steps, r->n_step);
    TG_REQUIRE((int64_t)r->capacity_steps * r->n < ((int64_t)1 << 31), "%s: capacity_steps %d x n %lld rows >= 2^31", who,
               r->capacity_steps, (long long)r->n);
    if (r->obs_dim < 1 || r->obs_dim > kReplayMaxObs || r->act_dim < 1 || r->act_dim > kReplayMaxAct)
        return set_error(TG_ERR_UNSUPPORTED, "%s: obs_dim=%d outside [1, %d] or act_dim=%d outside [1, %d]", who, r->obs_dim,
                         kReplayMaxObs, r->act_dim, kReplayMaxAct);
    TG_REQUIRE((((uintptr_t)r->d_obs | (uintptr_t)r->d_act | (uintptr_t)r->d_next_obs | (uintptr_t)r->d_last_obs) & 15) == 0,
               "%s: d_obs, d_act, d_next_obs and d_last_obs must be 16-byte aligned", who);
    return TG_OK;
}

template <int L> static void replay_sample_launch(const tg_replay* r, int64_t batch, const int64_t* indices, uint64_t seed,
                                                  uint64_t ordinal, const ReplayBatch& out, hipStream_t st) {
    const int64_t blocks = (batch * L + kReplayBlock - 1) / kReplayBlock;
    hipLaunchKernelGGL((replay_sample_kernel<L>), dim3((unsigned)blocks), dim3(kReplayBlock), 0, st, *r, batch, indices, seed, ordinal, out);
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_replay_start(const tg_replay* r, const float* d_obs_in, void* stream) {
    const char* who = "tg_replay_start";
    if (int rc = replay_check(who, r)) return rc;
    TG_REQUIRE(d_obs_in != nullptr, "%s: null pointer", who);
    const int64_t groups = (r->n * r->obs_dim + 3) / 4;
    hipLaunchKernelGGL(replay_start_kernel, dim3((unsigned)((groups + kReplayBlock - 1) / kReplayBlock)), dim3(kReplayBlock), 0,
                       (hipStream_t)stream, *r, d_obs_in);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

int tg_replay_push(const tg_replay* r, const float* d_actions, const float* d_obs_in, const float* d_reward, const uint8_t* d_terminated,
                   const uint8_t* d_truncated, const float* d_final_obs, void* stream) {
    const char* who = "tg_replay_push";
    if (int rc = replay_check(who, r)) return rc;
    TG_REQUIRE(d_actions && d_obs_in && d_reward && d_terminated && d_truncated && d_final_obs, "%s: null pointer", who);
    hipLaunchKernelGGL(replay_push_kernel, dim3((unsigned)((r->n + kReplaySlots - 1) / kReplaySlots)), dim3(kReplayBlock), 0,
                       (hipStream_t)stream, *r, d_actions, d_obs_in, d_reward, d_terminated, d_truncated, d_final_obs);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

int tg_replay_sample(const tg_replay* r, int64_t batch, const int64_t* d_indices, uint64_t seed, uint64_t ordinal, float* o_obs,
                     float* o_act, float* o_rew, float* o_next_obs, float* o_disc, int64_t* o_idx, void* stream) {
    const char* who = "tg_replay_sample";
    if (int rc = replay_check(who, r)) return rc;
    TG_REQUIRE(o_obs && o_act && o_rew && o_next_obs && o_disc && o_idx, "%s: null pointer", who);
    TG_REQUIRE(batch > 0 && batch < ((int64_t)1 << 31), "%s: batch=%lld outside [1, 2^31)", who, (long long)batch);
    TG_REQUIRE((((uintptr_t)o_obs | (uintptr_t)o_act | (uintptr_t)o_rew | (uintptr_t)o_next_obs | (uintptr_t)o_disc | (uintptr_t)o_idx) & 15) == 0,
               "%s: the outputs must be 16-byte aligned", who);
    const ReplayBatch out{o_obs, o_act, o_rew, o_next_obs, o_disc, o_idx};
    const hipStream_t st = (hipStream_t)stream;
    const int S = r->obs_dim;
    if (S <= 4) replay_sample_launch<4>(r, batch, d_indices, seed, ordinal, out, st);
    else if (S <= 8) replay_sample_launch<8>(r, batch, d_indices, seed, ordinal, out, st);
    else if (S <= 16) replay_sample_launch<16>(r, batch, d_indices, seed, ordinal, out, st);
    else replay_sample_launch<32>(r, batch, d_indices, seed, ordinal, out, st);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

}  // extern "C"
