// Shared pieces of the persistent MFMA-chain kernels (fused_rollout.hip, mlp_fwd_chain.hip): vector types and the
// weight ring that streams A fragments L2 -> LDS by LDS-DMA.
//
// One weight block = the A fragments of one 32-row output tile for all k-steps (hidden layers and head), or of all
// output tiles of the first layer (K padded to 32 = 2 k-steps): always KS KiB = KS pieces of 1 KiB (one
// wave-instruction each).  The block stream is the same every pass (L2-resident) and flows into a ring of D slots with
// P = D - 1 blocks in flight (`global_load_lds_dwordx4`, no VGPR staging: the stream needs ~15-30 GB/s per CU, far more
// bytes in flight than two register sets can hold).  Per block: a COUNTED `s_waitcnt vmcnt` (this wave's pieces of
// the block have landed; the younger blocks stay in flight), a raw `s_barrier` (everyone's pieces have landed, and
// everyone has finished reading the slot that is about to be refilled), then the DMA for block +P is issued.
// `__syncthreads()` would drain the ring (its fence waits vmcnt(0)).
//
// Two compiler behaviours to design around (hipcc, ROCm 7.2):
//   * vector-memory operations retire in issue order, stores included: the counted wait must allow for every
//     vector-memory operation issued behind the block it waits for (the caller passes that count);
//   * an LDS read WITHOUT alias-scope metadata is made to wait for every outstanding LDS-DMA (vmcnt(0)): LDS reads
//     inside the ring loop go through inlined helpers with `__restrict__` parameters (which attaches the metadata),
//     or are opaque inline assembly.
#pragma once
#include "tg_common.hpp"

namespace tg {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

// Cache policy of the chain kernels' activation / dZ stores: non-temporal (written once, read by a later kernel from beyond
// the caches anyway at the learner's 4 M-row chunks).
typedef unsigned int act_u32x4 __attribute__((ext_vector_type(4)));
__device__ static inline void act_store16(act_u32x4 v, act_u32x4* p) {
    __builtin_nontemporal_store(v, p);
}

// Panel order: the layout of the learner's INTERNAL [rows][H] bf16 tensors (stored activations, dZ), whose one reader is the
// weight-gradient kernel (mlp_dw.hip).  A 32-row tile is stored as that kernel's plain LDS panel image
// [row / 4][32-column group][row % 4][64 B] (DwGeom<H>): the 16-byte chunk c (features 8 c .. 8 c + 7) of row r sits at
//     (r / 32) * 64 H  +  (r % 32 / 4) * (H / 32 * 256)  +  (c / 4) * 256  +  (r % 4) * 64  +  (c % 4) * 16
// Rows stay time-major; a tensor is padded to whole tiles.  The chain kernels' lane (col, g) holds chunk 4 mt + g of its rows
// after block mt, so it stores its 16 bytes as they stand (no LDS transpose): one instruction covers 16 rows x 64 B = four
// 256-byte runs of whole lines; the consumer's 1-KiB LDS-DMA pieces are contiguous in memory.
// Rows past the end: their lanes computed the last row over again (every input is clamped).  A lane whose row lies inside the
// padded last tile writes that copy into ITS OWN pad slot -- never a valid row's bytes, and the consumer then reads finite
// pad rows, which it multiplies by masked-out dZ; a lane beyond the padded end (a wave whose whole tile is past the end)
// falls back on the last valid row, which it rewrites with the identical bytes the row's own lane stores.
template <int H>
struct PanelOrder {
    static constexpr int CG = H / 32;                 // 32-column groups per row
    static constexpr int ROWQ = CG * 256;             // bytes per 4-row group
    static constexpr int PANEL = 8 * ROWQ;            // bytes per 32-row tile (= 32 * 2 H)
    __host__ __device__ static constexpr int64_t chunk_off(int64_t row, int c) {
        return (row >> 5) * PANEL + ((row >> 2) & 7) * ROWQ + (c >> 2) * 256 + (row & 3) * 64 + (c & 3) * 16;
    }
    __host__ __device__ static constexpr int64_t store_row(int64_t row, int64_t rows) {
        return row < ((rows + 31) & ~(int64_t)31) ? row : rows - 1;
    }
};
// the chain kernels' store of block mt: `off[c]` = chunk_off(store_row(the lane's row of column tile c), g), once per round
template <int H>
__device__ static inline void store_panel(uint16_t* __restrict__ g, const int64_t (&off)[2], int mt, const bf16x8 (&v)[2]) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint4 u = __builtin_bit_cast(uint4, v[c]);
        act_store16(act_u32x4{u.x, u.y, u.z, u.w}, reinterpret_cast<act_u32x4*>(reinterpret_cast<char*>(g) + off[c] + mt * 256));
    }
}

// ReLU + bf16 pack of 8 accumulators: round first (v_cvt_pk_bf16_f32, 2 per instruction), then clamp the PACKED halves
// with v_pk_max_i16(x, 0) -- a negative bf16 (and -0) is a negative int16.  relu(round(x)) == round(relu(x)); 4 + 4
// instructions instead of 8 v_med3_f32 + 4 conversions (A/B on one box: rollout 8.3 -> 8.1 ms, chain with stores -1.5 %).
__device__ static inline uint32_t relu_pack_bf16x2(float a, float b) {
    typedef short i16x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const bf16x2 p = __builtin_convertvector(f32x2{a, b}, bf16x2);          // ONE v_cvt_pk_bf16_f32
    const i16x2 zero = {0, 0};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2, p), zero));
}
__device__ static inline bf16x8 relu_pack_bf16(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
    const uint4 u = {relu_pack_bf16x2(a0, a1), relu_pack_bf16x2(a2, a3), relu_pack_bf16x2(a4, a5), relu_pack_bf16x2(a6, a7)};
    return __builtin_bit_cast(bf16x8, u);
}

// Masked epilogue of one 32-feature block of a backward-data product (tg_mlp_backward_chain; tg_mlp_weight_grad's kind RH rebuilds
// the top layer's dZ with the same instructions) for one of the lane's two rows: round the 2 x 4 accumulators pairwise (dword d =
// features 2 d, 2 d + 1 of the lane's 8) and multiply each 16-bit half by its keep bit (v_pk_mul_lo_u16).  `wsh` = the block
// pair's mask word already shifted right by the lane's nibble 4 (g & 1): feature pair d of block mt is bit (mt & 1) * 8 + d
// (even feature) and 16 + that (odd feature).
__device__ static inline bf16x8 masked_pack(const f32x4& lo, const f32x4& hi, uint32_t wsh, int mt) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const uint32_t wk = wsh >> ((mt & 1) * 8);
    const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t pk = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{v[2 * d], v[2 * d + 1]}, bf16x2));
        const u16x2 keep = __builtin_bit_cast(u16x2, (wk >> d) & 0x00010001u);
        o[d] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, pk) * keep);
    }
    return __builtin_bit_cast(bf16x8, uint4{o[0], o[1], o[2], o[3]});
}

template <int KS, int WPW>
__device__ static inline void ring_dma_block(const uint4* __restrict__ gblock, uint4* __restrict__ slot, int wave, int lane) {
#pragma unroll
    for (int q = 0; q < KS / WPW; ++q) {
        const int piece = q * WPW + wave;
        __builtin_amdgcn_global_load_lds(gblock + piece * 64 + lane, (lds_void*)(slot + piece * 64), 16, 0, 0);
    }
}

// Consume the next block.  Expects in scope: wfrag, ring, n_blocks, wave, lane, the ring state (pre_pos, pre_slot,
// cur_slot) and the constants KS, WPW, D; declares `cur` (the block's fragments; TG_RING_NEXT_INTO: the caller declared it).
// WAITN: see above.
#define TG_RING_WAIT(WAITN) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAITN) : "memory");
#define TG_RING_NEXT_INTO(CUR)                                                                             \
    __builtin_amdgcn_s_barrier();                                                                          \
    asm volatile("" ::: "memory");                                                                         \
    ring_dma_block<KS, WPW>(wfrag + (int64_t)pre_pos * KS * 64, ring + pre_slot * KS * 64, wave, lane);    \
    pre_pos = (pre_pos + 1 == n_blocks) ? 0 : pre_pos + 1;                                                 \
    pre_slot = (pre_slot + 1 == D) ? 0 : pre_slot + 1;                                                     \
    CUR = ring + cur_slot * KS * 64;                                                                       \
    cur_slot = (cur_slot + 1 == D) ? 0 : cur_slot + 1;
#define TG_RING_NEXT    \
    const uint4* cur;   \
    TG_RING_NEXT_INTO(cur)
#define TG_RING_ADVANCE(WAITN) TG_RING_WAIT(WAITN) TG_RING_NEXT

// Depth-specialised kernel (mlp_bwd_chain.hip: the network depth is a template argument, the block loops are fully unrolled): block
// `c` of a round of NB blocks sits at a stream position and in ring slots that are constants of the unrolled code, so the ring
// keeps no state -- provided D divides NB (the backward chain at 5 hidden layers: 33 blocks, 3 slots), so that the ring is back
// where it was after every round.  Block c is read from slot c % D and the DMA behind its barrier fetches block (c + P) % NB into
// slot (c + P) % D.  The same barrier, the same DMAs in the same order as TG_RING_NEXT: the counted waits in front of it stay what
// they are.
// `wave` must be a scalar (readfirstlane): the DMA's LDS destination is then a scalar constant (M0) and its source a scalar base
// (stream + block position + the wave's piece) plus the lane's 32-bit offset `voff` (= 16 lane).  `voff` passes through an empty
// asm statement at every block, and so does the stream pointer: left visible, every block's address is loop-invariant, hipcc
// keeps all of them in registers across the round loop and spills (a vector spill's reload is a vector-memory operation: it
// would drain the ring; 2 NB scalar pairs spill to lanes).  Per block: two scalar adds per piece.
template <int KS, int WPW, int D, int NB>
__device__ static inline const uint4* ring_next_at(const uint4*& wfrag, uint4* ring, int c, int wave, uint32_t& voff) {
    static_assert(NB % D == 0, "the ring must be back at slot 0 after every round");
    constexpr int P = D - 1;
    __builtin_amdgcn_s_barrier();
    asm volatile("" : "+v"(voff), "+s"(wfrag) : : "memory");
    const char* gblock = reinterpret_cast<const char*>(wfrag) + ((c + P) % NB) * (KS * 1024);
    uint4* slot = ring + ((c + P) % D) * (KS * 64);
#pragma unroll
    for (int q = 0; q < KS / WPW; ++q) {
        const int piece = q * WPW + wave;
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint4*>(gblock + piece * 1024 + voff), (lds_void*)(slot + piece * 64), 16, 0, 0);
    }
    return ring + (c % D) * (KS * 64);
}

// Block-structured forward chain (mlp_fwd_chain.hip, kBlk): a round of 8 n + 2 blocks on a ring of 4 slots turns the ring by HALF a
// ring, whatever the depth n, so the ring keeps two per-round bases that swap at the round's end instead of per-block state.  Block
// c of the round sits in slot (s + c) % 4, s = 0 or 2 the slot of the round's first block: relative slots j = c % 4 = 0, 1 hang off
// the base of slot s, j = 2, 3 off the base of slot s ^ 2, at compile-time offsets.  `rd` are the lane's read pointers into those two
// slots (fragment reads: one register plus an immediate), `m0b` the LDS byte addresses of the wave's first piece in them (scalars:
// `wave` went through readfirstlane, M0 is one scalar add).  The DMA behind the barrier of a block in relative slot j refills
// relative slot j + 3 (the block before it, which every wave has finished reading) from `src + off`: a scalar base (the stream, or
// a layer's first block in it) plus a compile-time offset plus the lane's 32-bit offset `voff` (= 16 threadIdx.x: the wave's piece
// and the lane's 16 bytes in it).  Base and lane offset pass through an empty asm statement, as in ring_next_at.  The same barrier
// and the same DMAs in the same order as TG_RING_NEXT.
template <int KS, int WPW>
__device__ static inline const uint4* ring_next_rel(const char*& src, int off, const uint4* const (&rd)[2], const uint32_t (&m0b)[2], int j,
                                                    uint32_t& voff) {
    __builtin_amdgcn_s_barrier();
    asm volatile("" : "+v"(voff), "+s"(src) : : "memory");
    const int jd = (j + 3) & 3;
    const uint32_t dst = m0b[jd >> 1] + (jd & 1) * (KS * 1024);
#pragma unroll
    for (int q = 0; q < KS / WPW; ++q) {
        // (the piece's scalar base is pinned too: folded with the lane offset, hipcc adds 64-bit constants on the vector unit)
        const char* piece = src + off + q * (WPW * 1024);
        asm volatile("" : "+s"(piece));
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint4*>(piece + voff), (lds_void*)(uintptr_t)(dst + q * (WPW * 1024)), 16, 0, 0);
    }
    return rd[(j & 3) >> 1] + (j & 1) * (KS * 64);
}

}  // namespace tg
