// One hidden-to-hidden layer `j` (1 .. n_layers - 1) of mlp_bwd_chain_kernel's round: MT output blocks of 32 features.  Included
// twice by mlp_bwd_chain.hip, as the body of the run-time layer loop and of the fully unrolled one (NL), so that the run-time form
// is compiled from the text it always had.
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                // (without the head block's stores nothing but the one later DMA lies behind the second block of the first layer;
                // kFuse0: nor behind its first block -- the previous round ended without stores -- nor from the third block of the
                // last layer on, which writes LDS tiles instead of dZ)
                const bool fused_layer = kFuse0 && j == n_layers - 1;
                if constexpr (kFuse0) {
                    if (fused_layer) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // this wave's tile writes are done
                }
                if ((mt == 1 && j == 1 && !store_top) || ((kFuse0 || kPanel) && mt == 0 && j == 1 && !store_top) ||
                    (fused_layer && mt >= (kPanel ? 1 : 2))) {
                    TG_RING_WAIT((P - 1) * (KS / WPW))
                } else {
                    TG_RING_WAIT(kWaitN)
                }
                TG_BWD_RING_NEXT((j - 1) * MT + mt + 1)

                if (mt == 0) {
                    prefetch_mask(round, j);
                    mask_words(mw);
                }
                f32x4 acc[2][2] = {};
                // scheduling fences around the block's products: left alone, hipcc threads the pack / mask arithmetic of the
                // neighbouring blocks through the MFMA sequence (s_nop-padded); kept apart the kernel is 2.4 % faster (same-box A/B)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < K8; ++ks)
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        const bf16x8 a = __builtin_bit_cast(bf16x8, cur[(ks * 2 + f) * 64 + lane]);
#pragma unroll
                        for (int c = 0; c < 2; ++c) acc[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xin[c][ks], acc[f][c], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (kFuse0) {
                    // the tiles of block mt - 1 are complete behind this block's barrier; their products go behind this block's own
                    // (in front of them the fragment reads' latency is exposed: same-box A/B 2522 -> 2513 us per 2^22 rows)
                    if (fused_layer && mt >= 1) owner_work(mt - 1);
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) xout[c][mt] = masked_pack(acc[0][c], acc[1][c], mw[c][mt >> 1], mt);
                if (kFuse0 && fused_layer) {
                    // the block's 32 rows x 32 features into T[mt & 1][wave]; rows past the end (clamped duplicates of the last row)
                    // as zeros: they must not be counted twice in the contraction
                    char* tw = tiles + ((mt & 1) * WPW + wave) * 2048;
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int row = 16 * c + col;
                        uint4 o = __builtin_bit_cast(uint4, xout[c][mt]);
                        if (row0 + row >= rows) o = uint4{0u, 0u, 0u, 0u};
                        lds_store16(tw + (row >> 2) * 256 + (row & 3) * 64 + ((grp ^ ((row >> 2) & 3)) * 16), o);
                    }
                } else if constexpr (kPanel) {
                    const bf16x8 pv[2] = {xout[0][mt], xout[1][mt]};
                    store_panel<H>(ptrs.dz[j], poff, mt, pv);
                } else if (mt & 1) {
                    const bf16x8 pa[2] = {xout[0][mt - 1], xout[1][mt - 1]}, pb[2] = {xout[0][mt], xout[1][mt]};
                    store_pair(stage, ptrs.dz[j] + 32 * (mt - 1), row0, rows, H, lane, pa, pb);
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int ks = 0; ks < K8; ++ks) xin[c][ks] = xout[c][ks];
            ++mseq;
