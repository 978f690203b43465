// Proportional prioritised replay for gfx950 (tg_replay_prio_push / _update / _sample / _rebuild): a sum tree of fan-out 64 over the
// rows of a tg_replay, one tree node per wavefront lane.  The rule is stated in include/trajopt_grpo_hip.h (tg_replay_prio) and, level
// by level, in tests/replay_prio_ref.py; node sums and prefix scans are float32 adds in one fixed order, so the NumPy restatement of
// the tree and of the descent is bit for bit.  Only the two pow() results (a new leaf, a raw importance weight) are not restated: they
// are formed in float64 and rounded once.
//
// Work split.  A wavefront is the unit everywhere: lane j holds child j of one node, the node's sum is five-plus-one __shfl_down adds
// (the butterfly s[i] += s[i + 32], 16, .., 1; lane 0 ends with the sum), the descent's inclusive prefix is six __shfl_up adds
// (Kogge-Stone), the chosen child comes out of one __ballot.  Nothing goes through LDS.  Blocks are four independent waves.
//   prio_push_kernel     one wave per level-1 node that the new time slot's leaves touch: it writes the slot's leaves of that node
//                        (*d_max), reads the node's other leaves as they are, and stores the node.  Every leaf belongs to exactly one
//                        node, so no two waves write one address, and the first / last node, shared with neighbouring slots, are
//                        recomputed whole.  The slot is (d_cursor[0] - 1) mod K, read on the device: nothing changes by value.
//   prio_nodes_kernel    one wave per node of ONE level > 0, from one of three sources: a contiguous range given by value (rebuild),
//                        the range above the pushed slot (push), or the list d_idx[b] >> 6 l (update; duplicates store the same bits).
//   prio_crown_kernel    one workgroup of 16 waves: every level of at most 64 nodes, bottom up to the root, a barrier between levels.
//   prio_zero_kernel /   update_priorities' duplicate rule, the scheme the header names: one launch stores 0 to every named leaf, the
//   prio_max_kernel      next integer-atomicMaxes the new priority's bits into the leaf (and a wave's largest into *d_max).  Leaves are
//                        >= 0, so their bits order as unsigned integers and the result is the same for every launch order.
//   prio_sample_kernel   one wave per sampled row: the descent (one 256-byte node per level) and the gather of the row's 2 S + A <= 72
//                        floats by the same wave; lane 0 writes rew, disc, idx and the raw weight.
//   prio_norm_kernel     one workgroup: the batch maximum of the raw weights, then weight = raw / max.
// Levels are ordered by separate launches on the stream: no cooperative launch, no spin-wait, no grid barrier, no float atomic.
#include "tg_common.hpp"

#include <stdint.h>

namespace tg {

constexpr int kPrioBlock = 256, kPrioWaves = kPrioBlock / kWave;
constexpr int kPrioCrownBlock = 1024;
constexpr int kPrioMaxLevels = 7;                                          // the leaves and at most 6 levels above them
constexpr int kPrioMaxObs = 32, kPrioMaxAct = 8, kPrioMaxNStep = 16;
// the cap of a new priority: fewer than 2^31 leaves of at most 2^96 sum to less than 2^127, so no node, prefix or root leaves float32
constexpr float kPrioMaxPriority = 0x1p96f;

// the sum of a node's 64 children, one per lane, in the fixed butterfly order; lane 0 holds it (the other lanes hold partial sums)
__device__ static inline float node_sum(float x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = rn_add(x, __shfl_down(x, d));
    return x;
}
// the inclusive prefix of the 64 children by the Kogge-Stone scan
__device__ static inline float node_scan(float x, int lane) {
#pragma unroll
    for (int d = 1; d <= 32; d <<= 1) {
        const float y = __shfl_up(x, d);
        if (lane >= d) x = rn_add(x, y);
    }
    return x;
}
__device__ static inline uint32_t stored_rows(const tg_replay& r) {
    int32_t filled = r.d_filled[0];
    filled = filled < 0 ? 0 : filled > r.capacity_steps ? r.capacity_steps : filled;
    return (uint32_t)((int64_t)filled * r.n);                               // < 2^31
}
// the leaves [lo, hi] of the time slot the last push wrote
__device__ static inline void pushed_slot(const tg_replay& r, int64_t& lo, int64_t& hi) {
    int c = r.d_cursor[0];
    c = (uint32_t)c < (uint32_t)r.capacity_steps ? c : 0;
    c = c == 0 ? r.capacity_steps - 1 : c - 1;
    lo = (int64_t)c * r.n;
    hi = lo + r.n - 1;
}
// node `node` of level l (1 <= l < levels, node < size[l]) from its children: wave-uniform arguments
__device__ static inline void recompute_node(const tg_replay_prio& p, int l, int64_t node, int lane) {
    const float s = node_sum(p.d_tree[p.offset[l - 1] + node * 64 + lane]);  // (the level below is zero-padded to a multiple of 64)
    if (lane == 0) p.d_tree[p.offset[l] + node] = s;
}

__global__ __launch_bounds__(kPrioBlock) void prio_push_kernel(tg_replay r, tg_replay_prio p) {
    const int lane = threadIdx.x & 63;
    int64_t lo, hi;
    pushed_slot(r, lo, hi);
    const int64_t node = (lo >> 6) + (int64_t)blockIdx.x * kPrioWaves + (threadIdx.x >> 6);
    if (node > (hi >> 6)) return;                                           // (wave-uniform)
    const float top = __uint_as_float(*p.d_max);
    const int64_t leaf = node * 64 + lane;                                  // < size[0] rounded up to 64: inside the padded level
    float x;
    if (leaf >= lo && leaf <= hi) {
        x = top;
        p.d_tree[leaf] = x;
    } else {
        x = p.d_tree[leaf];
    }
    const float s = node_sum(x);
    if (lane == 0) p.d_tree[p.offset[1] + node] = s;
}

enum { kNodesRange = 0, kNodesPushed = 1, kNodesList = 2 };
template <int SRC>
__global__ __launch_bounds__(kPrioBlock) void prio_nodes_kernel(tg_replay r, tg_replay_prio p, int l, int64_t first, int64_t count,
                                                                 const int64_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kPrioWaves + (threadIdx.x >> 6);
    int64_t node;
    if (SRC == kNodesRange) {
        if (w >= count) return;
        node = first + w;
    } else if (SRC == kNodesPushed) {
        int64_t lo, hi;
        pushed_slot(r, lo, hi);
        node = (lo >> (6 * l)) + w;
        if (node > (hi >> (6 * l))) return;
    } else {
        if (w >= count) return;
        const int64_t row = idx[w];
        if ((uint64_t)row >= (uint64_t)stored_rows(r)) return;
        node = row >> (6 * l);
    }
    recompute_node(p, l, node, lane);
}

// levels l0 .. levels - 1, each of at most 64 nodes
__global__ __launch_bounds__(kPrioCrownBlock) void prio_crown_kernel(tg_replay_prio p, int l0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int l = l0; l < p.levels; ++l) {
        for (int64_t node = wave; node < p.size[l]; node += kPrioCrownBlock / kWave) recompute_node(p, l, node, lane);
        __threadfence_block();
        __syncthreads();                                                    // the level is in memory before the next one reads it
    }
}

// the new priority of an error, or a negative number where the element is ignored
__device__ static inline float new_priority(float td, float alpha, float eps) {
    if (!(__builtin_fabsf(td) <= 3.4028235e38f)) return -1.0f;              // NaN or infinite
    const double v = pow((double)__builtin_fabsf(td) + (double)eps, (double)alpha);
    return v < (double)kPrioMaxPriority ? (float)v : kPrioMaxPriority;
}
__global__ __launch_bounds__(kPrioBlock) void prio_zero_kernel(tg_replay r, tg_replay_prio p, int64_t batch,
                                                                const int64_t* __restrict__ idx, const float* __restrict__ td) {
    const int64_t b = (int64_t)blockIdx.x * kPrioBlock + threadIdx.x;
    if (b >= batch) return;
    const int64_t row = idx[b];
    const float e = td[b];
    if ((uint64_t)row < (uint64_t)stored_rows(r) && __builtin_fabsf(e) <= 3.4028235e38f) p.d_tree[row] = 0.0f;
}
__global__ __launch_bounds__(kPrioBlock) void prio_max_kernel(tg_replay r, tg_replay_prio p, int64_t batch,
                                                               const int64_t* __restrict__ idx, const float* __restrict__ td, float alpha,
                                                               float eps) {
    const int64_t b = (int64_t)blockIdx.x * kPrioBlock + threadIdx.x;
    uint32_t bits = 0;
    if (b < batch) {
        const int64_t row = idx[b];
        const float v = new_priority(td[b], alpha, eps);
        if ((uint64_t)row < (uint64_t)stored_rows(r) && v >= 0.0f) {
            bits = __float_as_uint(v);
            atomicMax(reinterpret_cast<uint32_t*>(p.d_tree) + row, bits);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {                                     // the wave's largest: one atomic per wave on the shared word
        const uint32_t o = (uint32_t)__shfl_xor((int)bits, d);
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits != 0) atomicMax(p.d_max, bits);
}

struct PrioBatch {
    float* obs;              // [B][S]
    float* act;              // [B][A]
    float* rew;
    float* next_obs;         // [B][S]
    float* disc;
    int64_t* idx;
    float* raw;              // [B] the importance weight before the division by the batch maximum
};

__global__ __launch_bounds__(kPrioBlock) void prio_sample_kernel(tg_replay r, tg_replay_prio p, int64_t batch,
                                                                  const int64_t* __restrict__ indices, uint64_t seed, uint64_t ordinal,
                                                                  float beta, PrioBatch out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * kPrioWaves + (threadIdx.x >> 6);
    if (b >= batch) return;                                                 // (wave-uniform)
    const int S = r.obs_dim, A = r.act_dim;
    const uint32_t R = stored_rows(r);
    const float root = p.d_tree[p.offset[p.levels - 1]];
    int64_t row;
    float leaf = 0.0f;
    if (indices != nullptr) {
        row = indices[b];
        if ((uint64_t)row < (uint64_t)R) leaf = p.d_tree[row];
    } else if (root > 0.0f) {
        uint32_t w[4];
        Philox::draw(seed, (uint64_t)b, (uint32_t)(ordinal >> 32), (uint32_t)ordinal, w);
        double t = ((double)b + Philox::u01d(w[0], w[1])) / (double)batch * (double)root;
        int64_t node = 0;
        for (int l = p.levels - 2; l >= 0; --l) {
            const float child = p.d_tree[p.offset[l] + node * 64 + lane];
            const float prefix = node_scan(child, lane);
            const unsigned long long positive = __ballot(child > 0.0f);
            const unsigned long long over = __ballot(child > 0.0f && (double)prefix > t);
            int chosen = 0;
            if (over != 0ull) chosen = __builtin_ctzll(over);
            else if (positive != 0ull) chosen = 63 - __builtin_clzll(positive);
            const float before = __shfl(prefix, chosen > 0 ? chosen - 1 : 0);
            if (chosen > 0) t -= (double)before;
            leaf = __shfl(child, chosen);
            node = node * 64 + chosen;
        }
        row = node;
    } else {
        row = -1;
    }
    const bool ok = (uint64_t)row < (uint64_t)R && leaf > 0.0f && root > 0.0f;
    const float nan = __builtin_nanf("");
    const float* __restrict__ so = r.d_obs + row * S;
    const float* __restrict__ sn = r.d_next_obs + row * S;
    const float* __restrict__ sa = r.d_act + row * A;
    for (int e = lane; e < 2 * S + A; e += kWave) {                         // obs | next_obs | act: adjacent lanes on adjacent floats
        float x = nan;
        if (e < S) {
            if (ok) x = so[e];
            out.obs[b * S + e] = x;
        } else if (e < 2 * S) {
            if (ok) x = sn[e - S];
            out.next_obs[b * S + e - S] = x;
        } else {
            if (ok) x = sa[e - 2 * S];
            out.act[b * A + e - 2 * S] = x;
        }
    }
    if (lane == 0) {
        float x = nan, y = nan, wt = nan;
        if (ok) {
            x = r.d_rew[row];
            y = r.d_disc[row];
            wt = (float)pow((double)R * (double)leaf / (double)root, -(double)beta);
        }
        out.rew[b] = x;
        out.disc[b] = y;
        out.idx[b] = row;
        out.raw[b] = wt;
    }
}

__global__ __launch_bounds__(kPrioCrownBlock) void prio_norm_kernel(const float* __restrict__ raw, float* __restrict__ weight, int64_t batch) {
    __shared__ float s_max[kPrioCrownBlock / kWave];
    float m = 0.0f;                                                         // raw weights are > 0; a NaN loses every comparison
    for (int64_t b = threadIdx.x; b < batch; b += kPrioCrownBlock) {
        const float x = raw[b];
        m = x > m ? x : m;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_xor(m, d);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s_max[0];
#pragma unroll
    for (int k = 1; k < kPrioCrownBlock / kWave; ++k) m = s_max[k] > m ? s_max[k] : m;
    for (int64_t b = threadIdx.x; b < batch; b += kPrioCrownBlock) weight[b] = rn_div(raw[b], m);
}

// ---- host side ----
static int64_t prio_levels(int64_t rows, tg_replay_prio* p) {
    int64_t n = rows, off = 0;
    int l = 0;
    for (;;) {
        p->size[l] = n;
        p->offset[l] = off;
        off += (n + 63) / 64 * 64;
        ++l;
        if (n == 1 && l > 1) break;
        n = (n + 63) / 64;
    }
    p->levels = l;
    for (; l < 8; ++l) p->size[l] = p->offset[l] = 0;
    p->reserved = 0;
    return off;
}

// what the entries refuse about the two objects (the first part states tg_replay's own rules again: replay.hip keeps its check to itself)
static int prio_check(const char* who, const tg_replay* r, const tg_replay_prio* p) {
    TG_REQUIRE(r && r->d_obs && r->d_act && r->d_next_obs && r->d_rew && r->d_disc && r->d_nstep && r->d_last_obs && r->d_cursor &&
               r->d_filled && r->d_open && p && p->d_tree && p->d_max, "%s: null pointer", who);
    TG_REQUIRE(r->n > 0 && r->capacity_steps > 0, "%s: bad sizes n=%lld capacity_steps=%d", who, (long long)r->n, r->capacity_steps);
    TG_REQUIRE(r->n_step >= 1 && r->n_step <= kPrioMaxNStep, "%s: n_step=%d outside [1, %d]", who, r->n_step, kPrioMaxNStep);
    TG_REQUIRE(r->capacity_steps >= r->n_step, "%s: capacity_steps=%d < n_step=%d", who, r->capacity_steps, r->n_step);
    TG_REQUIRE((int64_t)r->capacity_steps * r->n < ((int64_t)1 << 31), "%s: capacity_steps %d x n %lld rows >= 2^31", who,
               r->capacity_steps, (long long)r->n);
    if (r->obs_dim < 1 || r->obs_dim > kPrioMaxObs || r->act_dim < 1 || r->act_dim > kPrioMaxAct)
        return set_error(TG_ERR_UNSUPPORTED, "%s: obs_dim=%d outside [1, %d] or act_dim=%d outside [1, %d]", who, r->obs_dim, kPrioMaxObs,
                         r->act_dim, kPrioMaxAct);
    TG_REQUIRE((((uintptr_t)r->d_obs | (uintptr_t)r->d_act | (uintptr_t)r->d_next_obs | (uintptr_t)r->d_last_obs) & 15) == 0,
               "%s: d_obs, d_act, d_next_obs and d_last_obs must be 16-byte aligned", who);
    return TG_OK;
}
static int tree_check(const char* who, const tg_replay_prio* p, int64_t rows) {
    TG_REQUIRE(p && p->d_tree && p->d_max, "%s: null pointer", who);
    TG_REQUIRE(((uintptr_t)p->d_tree & 15) == 0 && ((uintptr_t)p->d_max & 3) == 0, "%s: d_tree must be 16-byte aligned, d_max 4-byte", who);
    TG_REQUIRE(p->levels >= 2 && p->levels <= kPrioMaxLevels && p->size[0] >= 1 && p->size[0] < ((int64_t)1 << 31) &&
               (rows == 0 || p->size[0] == rows), "%s: the tree's levels=%d size[0]=%lld do not fit %lld rows", who, p->levels,
               (long long)p->size[0], (long long)rows);
    tg_replay_prio want;
    prio_levels(p->size[0], &want);
    bool same = want.levels == p->levels;
    for (int l = 0; l < 8; ++l) same = same && want.size[l] == p->size[l] && want.offset[l] == p->offset[l];
    TG_REQUIRE(same, "%s: levels / size / offset are not tg_replay_prio_levels' for %lld rows", who, (long long)p->size[0]);
    return TG_OK;
}
static inline bool nonneg_finite(float x) { return x >= 0.0f && x <= 3.4028235e38f; }
static inline unsigned wave_blocks(int64_t waves) { return (unsigned)((waves + kPrioWaves - 1) / kPrioWaves); }
// the first level of at most 64 nodes: the crown starts there
static inline int crown_level(const tg_replay_prio* p) {
    int l = 1;
    while (p->size[l] > 64) ++l;
    return l;
}

}  // namespace tg

using namespace tg;

extern "C" {

int64_t tg_replay_prio_levels(int64_t rows, tg_replay_prio* p) {
    const char* who = "tg_replay_prio_levels";
    TG_REQUIRE(p != nullptr, "%s: null pointer", who);
    TG_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31), "%s: rows=%lld outside [1, 2^31)", who, (long long)rows);
    return prio_levels(rows, p);
}

int tg_replay_prio_rebuild(const tg_replay_prio* p, void* stream) {
    const char* who = "tg_replay_prio_rebuild";
    if (int rc = tree_check(who, p, 0)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int lc = crown_level(p);
    const tg_replay none{};
    for (int l = 1; l < lc; ++l)
        hipLaunchKernelGGL((prio_nodes_kernel<kNodesRange>), dim3(wave_blocks(p->size[l])), dim3(kPrioBlock), 0, st, none, *p, l,
                           (int64_t)0, p->size[l], (const int64_t*)nullptr);
    hipLaunchKernelGGL(prio_crown_kernel, dim3(1), dim3(kPrioCrownBlock), 0, st, *p, lc);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

int tg_replay_prio_push(const tg_replay* r, const tg_replay_prio* p, void* stream) {
    const char* who = "tg_replay_prio_push";
    if (int rc = prio_check(who, r, p)) return rc;
    if (int rc = tree_check(who, p, (int64_t)r->capacity_steps * r->n)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int lc = crown_level(p);
    // n consecutive leaves touch at most ceil((n - 1) / 64^l) + 1 nodes of level l, wherever they start
    hipLaunchKernelGGL(prio_push_kernel, dim3(wave_blocks((r->n + 62) / 64 + 1)), dim3(kPrioBlock), 0, st, *r, *p);
    for (int l = 2; l < lc; ++l) {
        const int64_t span = (int64_t)1 << (6 * l);
        hipLaunchKernelGGL((prio_nodes_kernel<kNodesPushed>), dim3(wave_blocks((r->n - 2 + span) / span + 1)), dim3(kPrioBlock), 0, st, *r,
                           *p, l, (int64_t)0, (int64_t)0, (const int64_t*)nullptr);
    }
    const int l0 = lc > 1 ? lc : 2;                                         // (level 1 is the push kernel's)
    if (l0 < p->levels) hipLaunchKernelGGL(prio_crown_kernel, dim3(1), dim3(kPrioCrownBlock), 0, st, *p, l0);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

int tg_replay_prio_update(const tg_replay* r, const tg_replay_prio* p, int64_t batch, const int64_t* d_idx, const float* d_td, float alpha,
                          float eps, void* stream) {
    const char* who = "tg_replay_prio_update";
    if (int rc = prio_check(who, r, p)) return rc;
    if (int rc = tree_check(who, p, (int64_t)r->capacity_steps * r->n)) return rc;
    TG_REQUIRE(d_idx && d_td, "%s: null pointer", who);
    TG_REQUIRE(batch > 0 && batch < ((int64_t)1 << 31), "%s: batch=%lld outside [1, 2^31)", who, (long long)batch);
    TG_REQUIRE(nonneg_finite(alpha) && nonneg_finite(eps), "%s: alpha=%g and eps=%g must be finite and >= 0", who, alpha, eps);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((batch + kPrioBlock - 1) / kPrioBlock);
    hipLaunchKernelGGL(prio_zero_kernel, dim3(blocks), dim3(kPrioBlock), 0, st, *r, *p, batch, d_idx, d_td);
    hipLaunchKernelGGL(prio_max_kernel, dim3(blocks), dim3(kPrioBlock), 0, st, *r, *p, batch, d_idx, d_td, alpha, eps);
    const int lc = crown_level(p);
    for (int l = 1; l < lc; ++l)
        hipLaunchKernelGGL((prio_nodes_kernel<kNodesList>), dim3(wave_blocks(batch)), dim3(kPrioBlock), 0, st, *r, *p, l, (int64_t)0, batch,
                           d_idx);
    hipLaunchKernelGGL(prio_crown_kernel, dim3(1), dim3(kPrioCrownBlock), 0, st, *p, lc);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

int tg_replay_prio_sample(const tg_replay* r, const tg_replay_prio* p, int64_t batch, const int64_t* d_indices, uint64_t seed,
                          uint64_t ordinal, float beta, float* o_obs, float* o_act, float* o_rew, float* o_next_obs, float* o_disc,
                          int64_t* o_idx, float* o_raw, float* o_weight, void* stream) {
    const char* who = "tg_replay_prio_sample";
    if (int rc = prio_check(who, r, p)) return rc;
    if (int rc = tree_check(who, p, (int64_t)r->capacity_steps * r->n)) return rc;
    TG_REQUIRE(o_obs && o_act && o_rew && o_next_obs && o_disc && o_idx && o_raw && o_weight, "%s: null pointer", who);
    TG_REQUIRE(batch > 0 && batch < ((int64_t)1 << 31), "%s: batch=%lld outside [1, 2^31)", who, (long long)batch);
    TG_REQUIRE(nonneg_finite(beta), "%s: beta=%g must be finite and >= 0", who, beta);
    TG_REQUIRE((((uintptr_t)o_obs | (uintptr_t)o_act | (uintptr_t)o_rew | (uintptr_t)o_next_obs | (uintptr_t)o_disc | (uintptr_t)o_idx |
                 (uintptr_t)o_raw | (uintptr_t)o_weight) & 15) == 0, "%s: the outputs must be 16-byte aligned", who);
    const PrioBatch out{o_obs, o_act, o_rew, o_next_obs, o_disc, o_idx, o_raw};
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(prio_sample_kernel, dim3(wave_blocks(batch)), dim3(kPrioBlock), 0, st, *r, *p, batch, d_indices, seed, ordinal, beta,
                       out);
    hipLaunchKernelGGL(prio_norm_kernel, dim3(1), dim3(kPrioCrownBlock), 0, st, (const float*)o_raw, o_weight, batch);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

}  // extern "C"
