// Hidden activation of the fp32 policy kernels (fused_rollout_f32.hip, mlp_f32_chain.hip): a compile-time template argument,
// TG_ACT_RELU or TG_ACT_TANH (include/trajopt_grpo_hip.h), so that the ReLU instantiations compile to the code they were before
// the argument existed.  Room is left for more (Sigmoid): a new value here, a case in the launchers' switches.
#pragma once

#include "tg_common.hpp"

namespace tg {

template <int kAct>
constexpr bool act_supported() { return kAct == TG_ACT_RELU || kAct == TG_ACT_TANH; }

// a = act(z) of one fp32 pre-activation.  Tanh: the device library's tanhf (ocml: an odd polynomial below |z| = 0.625, else
// 1 - 2 / (exp(2|z|) + 1) with v_exp_f32 / v_rcp_f32, sign copied back); |tanhf(z) - tanh(z)| <= 4 * 2^-24 for every finite z
// (tests/test_tanh_gpu.py checks that bound against fp64 over a dense sweep of [-20, 20]).
template <int kAct>
__device__ static inline float act_f32(float z) {
    static_assert(act_supported<kAct>(), "unknown hidden activation");
    if constexpr (kAct == TG_ACT_TANH) return tanhf(z);
    else return fmaxf(z, 0.0f);
}

}  // namespace tg
