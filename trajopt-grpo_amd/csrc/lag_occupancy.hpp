// Occupancy hints of the Lagged<> kernel instantiations (included at the end of env_dynamics.hpp).
//
// A Lagged kernel holds A + 1 more values across the step than its `_sub` sibling (the motor state and its gain).  Where the
// compiler had packed the sibling to the edge of an occupancy class (waves per SIMD that the 512-entry unified register file admits),
// those few values tip the Lagged instantiation into the class below, and the allocator then spreads out in it.  lag_min_waves()
// names, for the instantiations where that happens AND the compiler can hold the sibling's class without scratch, that class; the
// kernels pass it to amdgpu_waves_per_eu, which makes the compiler schedule and allocate for it.  0 = no hint: every other
// instantiation (all that are not Lagged among them) gets no attribute at all and compiles as it did.
// How the rows were found (tools/kernel_resources.py on the cross-compiled library, no GPU): build with no rows; list the Lagged
// kernels whose class is below that of the same kernel without the wrapper (57); give each its sibling's class; build again and
// drop the rows whose kernel now uses scratch (24: the per-step, one-launch and final-state kernels in float, where the step itself
// is the register peak, and the bf16 kernel with a parameter table for QuadPole).  The 33 rows left are below;
// profiles/r18_motor_lag_probe.md lists both groups with their figures.  Redo this after a compiler change.
#pragma once

namespace tg {

enum { kLagFamFinal, kLagFamF32, kLagFamF32x16 };         // the kernel families that have rows

// kFam: the kernel family; EnvK, R: its Env type and arithmetic type; P0..P2: its remaining template arguments in order
// (final_state_kernel: none; the fp32 fused kernels: H, NHH, kAct).
template <int kFam, typename EnvK, typename R, int P0 = 0, int P1 = 0, int P2 = 0>
constexpr int lag_min_waves() {
    if constexpr (!EnvTraits<EnvK>::kLag) return 0;
    else if constexpr (kFam == kLagFamFinal && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPoleEnv<double>>>>> && std::is_same_v<R, double>) return 4;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPole2DEnv<float>>>>> && P0 == 128 && P1 == 0 && P2 == 0) return 4;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPole2DEnv<float>>>>> && P0 == 128 && P1 == 2 && P2 == 0) return 2;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPole2DEnv<float>>>>> && P0 == 64 && P1 == 0 && P2 == 0) return 4;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPole2DEnv<float>>>>> && P0 == 64 && P1 == 1 && P2 == 1) return 3;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>> && P0 == 128 && P1 == 0 && P2 == 0) return 3;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>> && P0 == 128 && P1 == 0 && P2 == 1) return 3;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>> && P0 == 64 && P1 == 0 && P2 == 0) return 3;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>> && P0 == 64 && P1 == 0 && P2 == 1) return 3;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<QuadPoleEnv<float>>>> && P0 == 128 && P1 == 1 && P2 == 0) return 2;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<QuadPoleEnv<float>>>> && P0 == 64 && P1 == 2 && P2 == 0) return 2;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, Lagged<Substepped<QuadPoleEnv<float>>>> && P0 == 64 && P1 == 3 && P2 == 1) return 2;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>>> && P0 == 128 && P1 == 0 && P2 == 0) return 3;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>>> && P0 == 128 && P1 == 0 && P2 == 1) return 3;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>>> && P0 == 64 && P1 == 0 && P2 == 0) return 3;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>>> && P0 == 64 && P1 == 0 && P2 == 1) return 3;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<QuadPoleEnv<float>>>>> && P0 == 128 && P1 == 1 && P2 == 0) return 2;
    else if constexpr (kFam == kLagFamF32 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<QuadPoleEnv<float>>>>> && P0 == 64 && P1 == 3 && P2 == 1) return 2;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPole2DEnv<float>>>>> && P0 == 128 && P1 == 2 && P2 == 1) return 2;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>> && P0 == 128 && P1 == 0 && P2 == 1) return 3;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>> && P0 == 64 && P1 == 0 && P2 == 1) return 3;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>> && P0 == 64 && P1 == 3 && P2 == 0) return 2;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, Lagged<Substepped<QuadPole2DEnv<float>>>> && P0 == 128 && P1 == 0 && P2 == 0) return 5;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, Lagged<Substepped<QuadPole2DEnv<float>>>> && P0 == 128 && P1 == 1 && P2 == 0) return 3;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, Lagged<Substepped<QuadPole2DEnv<float>>>> && P0 == 64 && P1 == 0 && P2 == 0) return 5;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, Lagged<Substepped<QuadPoleEnv<float>>>> && P0 == 64 && P1 == 1 && P2 == 0) return 3;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<PerEnv<QuadPole2DEnv<float>>>>>> && P0 == 128 && P1 == 0 && P2 == 1) return 4;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<PerEnv<QuadPole2DEnv<float>>>>>> && P0 == 64 && P1 == 0 && P2 == 1) return 4;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<PerEnv<QuadPole2DEnv<float>>>>>> && P0 == 64 && P1 == 1 && P2 == 1) return 3;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>>> && P0 == 128 && P1 == 0 && P2 == 0) return 3;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<PerEnv<QuadPoleEnv<float>>>>>> && P0 == 64 && P1 == 0 && P2 == 0) return 3;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<QuadPole2DEnv<float>>>>> && P0 == 64 && P1 == 2 && P2 == 0) return 3;
    else if constexpr (kFam == kLagFamF32x16 && std::is_same_v<EnvK, ObsNormed<Lagged<Substepped<QuadPoleEnv<float>>>>> && P0 == 64 && P1 == 3 && P2 == 1) return 2;
    else return 0;
}
}  // namespace tg
