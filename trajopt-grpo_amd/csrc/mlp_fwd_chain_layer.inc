// One hidden-to-hidden layer `l` of mlp_fwd_chain_kernel's block-structured form (kBlk): MT output blocks of 32 features.  Included
// three times by mlp_fwd_chain.hip -- the first H x H layer (kFirst), the rolled loop over the middle ones, the top one (kTop, whose
// activation is never written) -- so that every wait count, every ring slot and whether a block stores are constants of its text.
// In scope: l, kFirst, kTop, `lay` (the stream at this layer's first block; left at the next layer's), and the round's state.
// The arithmetic, the barriers, the DMAs, the stores and the counted waits are those of the run-time layer loop, block for block.
            {
                const float* bl = bias_s + (l + 1) * H + 8 * grp;
                // this layer's pointers, read here and nowhere in its blocks (scalars; the asm keeps hipcc from re-reading the kernel
                // arguments at every store).  The entry point requires every mask plane, so there is no null test.
                typedef __attribute__((address_space(1))) char global_char;
                global_char* pl = kTop ? nullptr : (global_char*)(reinterpret_cast<char*>(acts.p[l + 1]) + round_off);
                typedef __attribute__((address_space(1))) uint32_t global_u32;
                global_u32* mlg = (global_u32*)acts.m[l];
                asm volatile("" : "+s"(pl), "+s"(mlg));
                uint32_t* ml = (uint32_t*)mlg;                      // (through the global address space: the asm hides where it points)
                uint32_t mw[2][MT / 2];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    // (TG_PANEL_WAIT's argument: the storing blocks among the three in front of this one, see the kernel's head)
                    const int same = mt < 3 ? mt : 3;
                    __builtin_amdgcn_sched_barrier(0);
                    if (kTop) { TG_PANEL_WAIT(3 - same) } else if (kFirst) { TG_PANEL_WAIT(same) } else { TG_PANEL_WAIT(3) }
                    if (kTop && mt + 3 >= MT + 1) ring_next_rel<KS, WPW>(wsrc, (mt + 3 - (MT + 1)) * (KS * 1024), rd, m0b, 1 + mt, voff);
                    else ring_next_rel<KS, WPW>(lay, (mt + 3) * (KS * 1024), rd, m0b, 1 + mt, voff);
                    mw[mt / (MT / 2)][mt % (MT / 2)] = pair_mask_word(xin[mt / (MT / 2)], mt % (MT / 2), 4 * (grp & 1));
                    bf16x8 o[2];
                    chain_block_pairs((uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint4*)rd[((1 + mt) & 3) >> 1], (1 + mt) & 1,
                                      bl + 32 * mt, xin, o);
                    xout[0][mt] = o[0];
                    xout[1][mt] = o[1];
                    if (mt == MT - 1) {
#pragma unroll
                        for (int c = 0; c < 2; ++c) store_mask_words<MT>(ml, rowc[c], grp, mw[c]);
                    }
                    if (!kTop) {
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            const uint4 u = __builtin_bit_cast(uint4, o[c]);
                            // (scalar base, the lane's 32-bit offset, the block as the immediate: no address arithmetic -- the offset
                            // is opaque here, or hipcc adds it to the base once per layer and keeps two 64-bit lane addresses)
                            asm volatile("" : "+v"(poff32[c]));
                            __builtin_nontemporal_store(act_u32x4{u.x, u.y, u.z, u.w},
                                                        (__attribute__((address_space(1))) act_u32x4*)(pl + poff32[c] + mt * 256));
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int ks = 0; ks < K8; ++ks) xin[c][ks] = xout[c][ks];
                lay += MT * (KS * 1024);
            }
