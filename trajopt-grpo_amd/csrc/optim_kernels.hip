// One launch per optimizer step, one more for every derived weight layout -- instead of torch.optim.Adam's ~8 multi-tensor
// launches plus cat / gather / convert per weight stream (pipelines/*: `torch.optim.Adam(policy.parameters(), lr=...)`,
// algorithms/grpo.py:145 / ppo.py:183 `optimizer.step()`): at C2's 0.45 ms per update those ~20 small launches were a fifth of
// the step.
//
//   tg_adam_step      torch.optim.Adam's default (foreach, non-capturable, no amsgrad / weight decay / maximize) update of up to 64
//                     tensors in one launch, the SAME fp32 operation sequence per element -- lerp, mul, addcmul, sqrt, div, add,
//                     addcdiv, each rounded where torch's separate kernels round -- so the weights stay bit-identical to
//                     `optimizer.step()` (tests/test_gpu_parity.py::test_fused_adam_is_bit_identical_to_torch);
//   tg_gather_streams every derived layout of the weights (the chain kernels' bf16 fragment streams and f32 bias tables, the fp32
//                     chain stream) rebuilt from the fp32 masters by one gather: element j of segment s = master
//                     tensor (code >> 24), offset (code & 0xFFFFFF), or zero.
//   tg_grad_clip_coef global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) without a host round trip: the L2 norm of the
//                     flat gradient bucket (squares summed in float64, in a fixed order) and min(1, max_norm / (norm + 1e-6)) as
//                     two device floats; tg_adam_step_clip / tg_adam_step_push_clip read the coefficient and step on g * coef.
#include "adam_update.hpp"

namespace tg {

// kPush: the thread that has just updated a parameter also writes it into every derived layout it appears in (adam_push) --
// tg_gather_streams folded into the optimizer step.
// kClip: the gradient is first scaled by *coef (tg_grad_clip_coef's coefficient: one float32 product, rounded once, as
// clip_grad_norm_'s g.mul_(coef) rounds it), and a gradient that is not zeroed is left holding the scaled value.
template <bool kPush, bool kClip>
__global__ __launch_bounds__(256) void adam_kernel(const AdamTensor* __restrict__ table, int32_t n_tensors, int64_t total, AdamScalars a,
                                                   int32_t zero_grads, const GatherSegment* __restrict__ seg,
                                                   const int32_t* __restrict__ inv_start, const int32_t* __restrict__ inv_dst,
                                                   const float* __restrict__ coef) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int k = 0;
    for (int t = 1; t < n_tensors; ++t)
        if (e >= table[t].first) k = t;
    const AdamTensor d = table[k];
    const int64_t i = e - d.first;
    float g = d.g[i];
    if constexpr (kClip) g = rn_mul(g, *coef);
    float m = d.m[i], v = d.v[i];
    const float p = adam_update(g, m, v, d.p[i], a);
    d.m[i] = m; d.v[i] = v; d.p[i] = p;
    if (zero_grads) d.g[i] = 0.0f;          // the next step's optimizer.zero_grad(set_to_none=False), while the line is here
    else if constexpr (kClip) d.g[i] = g;   // the caller reads clipped gradients, as after clip_grad_norm_
    if constexpr (kPush) adam_push(e, p, seg, inv_start, inv_dst);
}

// adam_kernel behind tg_kl_control's device control block (policy_shift.hip; ctl f64 [8], ctl[0] = stopped, ctl[1] = lr): kernels of
// their own, so that the four above keep their code.  Every thread reads ctl[0], a uniform load: once a check has latched it, a
// launch that was already enqueued writes no parameter, no moment and no derived layout -- it zeroes its gradient element if
// zero_grads asks and leaves the gradient as it is otherwise (the clip product is not written back).
// lr_from_ctl: step_size is formed here, in double, from the device's rate and the host's bc1 = 1 - beta1^step, by the division
// adam_scalars() does: a block that holds the host's lr gives the plain launch's bits.
template <bool kPush, bool kClip>
__global__ __launch_bounds__(256) void adam_ctl_kernel(const AdamTensor* __restrict__ table, int32_t n_tensors, int64_t total, AdamScalars a,
                                                       int32_t zero_grads, const GatherSegment* __restrict__ seg,
                                                       const int32_t* __restrict__ inv_start, const int32_t* __restrict__ inv_dst,
                                                       const float* __restrict__ coef, const double* __restrict__ ctl, int32_t lr_from_ctl,
                                                       double bc1) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int k = 0;
    for (int t = 1; t < n_tensors; ++t)
        if (e >= table[t].first) k = t;
    const AdamTensor d = table[k];
    const int64_t i = e - d.first;
    if (ctl[0] != 0.0) {
        if (zero_grads) d.g[i] = 0.0f;
        return;
    }
    if (lr_from_ctl) a.step_size = (float)((ctl[1] / bc1) * -1.0);
    float g = d.g[i];
    if constexpr (kClip) g = rn_mul(g, *coef);
    float m = d.m[i], v = d.v[i];
    const float p = adam_update(g, m, v, d.p[i], a);
    d.m[i] = m; d.v[i] = v; d.p[i] = p;
    if (zero_grads) d.g[i] = 0.0f;
    else if constexpr (kClip) d.g[i] = g;
    if constexpr (kPush) adam_push(e, p, seg, inv_start, inv_dst);
}

// flag[0] |= 1 when any element of tensor pair (p, g) of the table differs bitwise (the learner's check that "old_policy is the
// policy" really held when it let the first update stand in for the old policy's pass)
__global__ __launch_bounds__(256) void params_differ_kernel(const AdamTensor* __restrict__ table, int32_t n_tensors, int64_t total,
                                                            int32_t* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int k = 0;
    for (int t = 1; t < n_tensors; ++t)
        if (e >= table[t].first) k = t;
    const AdamTensor d = table[k];
    const int64_t i = e - d.first;
    if (__float_as_uint(d.p[i]) != __float_as_uint(d.g[i])) atomicOr(flag, 1);
}

__global__ __launch_bounds__(256) void gather_streams_kernel(const GatherSegment* __restrict__ seg, int32_t n_seg, int64_t total,
                                                             const AdamTensor* __restrict__ table) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int k = 0;
    for (int t = 1; t < n_seg; ++t)
        if (e >= seg[t].first) k = t;
    const GatherSegment s = seg[k];
    const int64_t j = e - s.first;
    const int32_t c = s.code[j];
    const float v = c < 0 ? 0.0f : table[c >> 24].p[c & 0xFFFFFF];
    if (s.is_bf16) reinterpret_cast<__bf16*>(s.dst)[j] = (__bf16)v;
    else reinterpret_cast<float*>(s.dst)[j] = v;
}

// ---- global gradient norm: two small launches, ordered by the stream ----
// Launch 1: block b sums the squares of elements [b * kNormChunk, (b + 1) * kNormChunk) (grid-stride beyond kNormMaxBlocks chunks)
// in float64 and writes ONE partial.  The product of two float32 values is exact in float64 and a sum of n < 2^53 of them cannot
// overflow, so the only rounding is that of the additions.  Which elements a thread adds, and the order of every addition after
// that (xor-shuffle tree inside a wave, the four waves' sums in wave order), depend on n alone: the same bytes give the same bits.
constexpr int kNormThreads = 256, kNormPerThread = 16, kNormChunk = kNormThreads * kNormPerThread, kNormMaxBlocks = 1024;

static inline int64_t norm_blocks(int64_t n) { return n <= 0 ? 0 : (ceil_div(n, kNormChunk) < kNormMaxBlocks ? ceil_div(n, kNormChunk) : kNormMaxBlocks); }

// the sum over the block's 256 threads, in a fixed order; valid in thread 0
__device__ static inline double block_sum_f64(double s, double* lds4) {
    for (int off = kWave / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) lds4[threadIdx.x / kWave] = s;
    __syncthreads();
    return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

__global__ __launch_bounds__(kNormThreads) void sumsq_partials_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ partial) {
    __shared__ double lds4[kNormThreads / kWave];
    double s = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * kNormChunk; base < n; base += (int64_t)gridDim.x * kNormChunk) {
        float v[kNormPerThread];
#pragma unroll
        for (int k = 0; k < kNormPerThread; ++k) {          // (consecutive lanes, consecutive floats: every load is one full line per wave)
            const int64_t i = base + k * kNormThreads + threadIdx.x;
            v[k] = i < n ? x[i] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kNormPerThread; ++k) s += (double)v[k] * (double)v[k];
    }
    s = block_sum_f64(s, lds4);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Launch 2 (one block): the partials in a fixed order, then out2 = {norm, min(1, max_norm / (norm + 1e-6))} in float32 -- the
// coefficient as clip_grad_norm_ forms it (float32 sum, float32 quotient, clamp; a NaN norm gives a NaN coefficient, as torch.clamp does)
__global__ __launch_bounds__(kNormThreads) void clip_coef_kernel(const double* __restrict__ partial, int32_t n_partial, float max_norm,
                                                                 float* __restrict__ out2) {
    __shared__ double lds4[kNormThreads / kWave];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += kNormThreads) s += partial[i];
    s = block_sum_f64(s, lds4);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        const float q = rn_div(max_norm, rn_add(norm, 1e-6f));
        out2[0] = norm;
        out2[1] = q > 1.0f ? 1.0f : q;
    }
}

}  // namespace tg

using namespace tg;

// the argument checks tg_adam_step[_clip] and tg_adam_step_push[_clip] share; push: the layout tables are part of the call
static int adam_args_ok(const char* who, const void* d_table, int32_t n_tensors, int64_t total, double beta1, int64_t step, bool push,
                        const void* d_segments, int32_t n_segments, const void* d_inv_start, const void* d_inv_dst) {
    if (push) TG_REQUIRE(d_table && d_segments && d_inv_start && d_inv_dst, "%s: null pointer", who);
    else TG_REQUIRE(d_table, "%s: null table", who);
    TG_REQUIRE(n_tensors >= 1 && n_tensors <= kAdamMaxTensors, "%s: %d tensors outside 1..%d", who, n_tensors, kAdamMaxTensors);
    if (push)
        TG_REQUIRE(n_segments >= 1 && n_segments <= kGatherMaxSegments, "%s: %d segments outside 1..%d", who, n_segments, kGatherMaxSegments);
    TG_REQUIRE(total >= 0 && step >= 1, "%s: bad sizes (total %lld, step %lld)", who, (long long)total, (long long)step);
    TG_REQUIRE(1.0 - beta1 < 0.5, "%s: beta1 = %g: lerp's other branch (weight >= 0.5) is not implemented", who, beta1);
    return TG_OK;
}

extern "C" {

int tg_adam_step(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                 int64_t step, int32_t zero_grads, void* stream) {
    if (int rc = adam_args_ok("tg_adam_step", d_table, n_tensors, total, beta1, step, false, nullptr, 0, nullptr, nullptr)) return rc;
    if (total == 0) return TG_OK;
    static_assert(sizeof(tg_adam_tensor) == sizeof(AdamTensor), "ABI struct and kernel struct must agree");
    hipLaunchKernelGGL((adam_kernel<false, false>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const AdamTensor*>(d_table), n_tensors, total, adam_scalars(lr, beta1, beta2, eps, step), zero_grads,
                       nullptr, nullptr, nullptr, nullptr);
    TG_LAUNCH_CHECK("tg_adam_step");
    return TG_OK;
}

int tg_adam_step_clip(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                      int64_t step, int32_t zero_grads, const float* d_coef, void* stream) {
    if (int rc = adam_args_ok("tg_adam_step_clip", d_table, n_tensors, total, beta1, step, false, nullptr, 0, nullptr, nullptr)) return rc;
    TG_REQUIRE(d_coef, "tg_adam_step_clip: null d_coef");
    if (total == 0) return TG_OK;
    hipLaunchKernelGGL((adam_kernel<false, true>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const AdamTensor*>(d_table), n_tensors, total, adam_scalars(lr, beta1, beta2, eps, step), zero_grads,
                       nullptr, nullptr, nullptr, d_coef);
    TG_LAUNCH_CHECK("tg_adam_step_clip");
    return TG_OK;
}

int tg_adam_step_push(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                      int64_t step, int32_t zero_grads, const tg_gather_segment* d_segments, int32_t n_segments,
                      const int32_t* d_inv_start, const int32_t* d_inv_dst, void* stream) {
    if (int rc = adam_args_ok("tg_adam_step_push", d_table, n_tensors, total, beta1, step, true, d_segments, n_segments, d_inv_start, d_inv_dst))
        return rc;
    if (total == 0) return TG_OK;
    hipLaunchKernelGGL((adam_kernel<true, false>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const AdamTensor*>(d_table), n_tensors, total, adam_scalars(lr, beta1, beta2, eps, step), zero_grads,
                       reinterpret_cast<const GatherSegment*>(d_segments), d_inv_start, d_inv_dst, nullptr);
    TG_LAUNCH_CHECK("tg_adam_step_push");
    return TG_OK;
}

int tg_adam_step_push_clip(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                           int64_t step, int32_t zero_grads, const tg_gather_segment* d_segments, int32_t n_segments,
                           const int32_t* d_inv_start, const int32_t* d_inv_dst, const float* d_coef, void* stream) {
    if (int rc = adam_args_ok("tg_adam_step_push_clip", d_table, n_tensors, total, beta1, step, true, d_segments, n_segments, d_inv_start,
                              d_inv_dst))
        return rc;
    TG_REQUIRE(d_coef, "tg_adam_step_push_clip: null d_coef");
    if (total == 0) return TG_OK;
    hipLaunchKernelGGL((adam_kernel<true, true>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const AdamTensor*>(d_table), n_tensors, total, adam_scalars(lr, beta1, beta2, eps, step), zero_grads,
                       reinterpret_cast<const GatherSegment*>(d_segments), d_inv_start, d_inv_dst, d_coef);
    TG_LAUNCH_CHECK("tg_adam_step_push_clip");
    return TG_OK;
}

}  // extern "C"

// the four `_ctl` entry points: the plain entry point's checks, the control block's, one launch of adam_ctl_kernel
template <bool kPush, bool kClip>
static int adam_step_ctl(const char* who, const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2,
                         double eps, int64_t step, int32_t zero_grads, const tg_gather_segment* d_segments, int32_t n_segments,
                         const int32_t* d_inv_start, const int32_t* d_inv_dst, const float* d_coef, const double* d_ctl, int32_t lr_from_ctl,
                         double bc1, void* stream) {
    if (int rc = adam_args_ok(who, d_table, n_tensors, total, beta1, step, kPush, d_segments, n_segments, d_inv_start, d_inv_dst)) return rc;
    if (kClip) TG_REQUIRE(d_coef, "%s: null d_coef", who);
    TG_REQUIRE(d_ctl && ((uintptr_t)d_ctl & 7) == 0, "%s: d_ctl is null or not 8-B aligned", who);
    TG_REQUIRE(lr_from_ctl == 0 || lr_from_ctl == 1, "%s: lr_from_ctl = %d is neither 0 nor 1", who, lr_from_ctl);
    TG_REQUIRE(bc1 > 0.0 && bc1 <= 1.0, "%s: bc1 = %g outside (0, 1] (1 - beta1^step)", who, bc1);
    if (total == 0) return TG_OK;
    hipLaunchKernelGGL((adam_ctl_kernel<kPush, kClip>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const AdamTensor*>(d_table), n_tensors, total, adam_scalars(lr, beta1, beta2, eps, step), zero_grads,
                       reinterpret_cast<const GatherSegment*>(d_segments), d_inv_start, d_inv_dst, d_coef, d_ctl, lr_from_ctl, bc1);
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}

extern "C" {

int tg_adam_step_ctl(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                     int64_t step, int32_t zero_grads, const double* d_ctl, int32_t lr_from_ctl, double bc1, void* stream) {
    return adam_step_ctl<false, false>("tg_adam_step_ctl", d_table, n_tensors, total, lr, beta1, beta2, eps, step, zero_grads, nullptr, 0, nullptr,
                                       nullptr, nullptr, d_ctl, lr_from_ctl, bc1, stream);
}

int tg_adam_step_ctl_clip(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                          int64_t step, int32_t zero_grads, const float* d_coef, const double* d_ctl, int32_t lr_from_ctl, double bc1,
                          void* stream) {
    return adam_step_ctl<false, true>("tg_adam_step_ctl_clip", d_table, n_tensors, total, lr, beta1, beta2, eps, step, zero_grads, nullptr, 0,
                                      nullptr, nullptr, d_coef, d_ctl, lr_from_ctl, bc1, stream);
}

int tg_adam_step_push_ctl(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2, double eps,
                          int64_t step, int32_t zero_grads, const tg_gather_segment* d_segments, int32_t n_segments,
                          const int32_t* d_inv_start, const int32_t* d_inv_dst, const double* d_ctl, int32_t lr_from_ctl, double bc1,
                          void* stream) {
    return adam_step_ctl<true, false>("tg_adam_step_push_ctl", d_table, n_tensors, total, lr, beta1, beta2, eps, step, zero_grads, d_segments,
                                      n_segments, d_inv_start, d_inv_dst, nullptr, d_ctl, lr_from_ctl, bc1, stream);
}

int tg_adam_step_push_ctl_clip(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, double lr, double beta1, double beta2,
                               double eps, int64_t step, int32_t zero_grads, const tg_gather_segment* d_segments, int32_t n_segments,
                               const int32_t* d_inv_start, const int32_t* d_inv_dst, const float* d_coef, const double* d_ctl,
                               int32_t lr_from_ctl, double bc1, void* stream) {
    return adam_step_ctl<true, true>("tg_adam_step_push_ctl_clip", d_table, n_tensors, total, lr, beta1, beta2, eps, step, zero_grads, d_segments,
                                     n_segments, d_inv_start, d_inv_dst, d_coef, d_ctl, lr_from_ctl, bc1, stream);
}

int64_t tg_grad_clip_workspace(int64_t n) { return norm_blocks(n) * (int64_t)sizeof(double); }

int tg_grad_clip_coef(const float* d_flat, int64_t n, double max_norm, float* d_out2, double* d_work, void* stream) {
    TG_REQUIRE(n >= 0, "tg_grad_clip_coef: negative size %lld", (long long)n);
    TG_REQUIRE(d_out2 && (n == 0 || (d_flat && d_work)), "tg_grad_clip_coef: null pointer");
    TG_REQUIRE(isfinite(max_norm) && max_norm > 0.0, "tg_grad_clip_coef: max_norm = %g must be finite and > 0", max_norm);
    const int32_t blocks = (int32_t)norm_blocks(n);
    if (blocks > 0) {
        hipLaunchKernelGGL(sumsq_partials_kernel, dim3((unsigned)blocks), dim3(kNormThreads), 0, (hipStream_t)stream, d_flat, n, d_work);
        TG_LAUNCH_CHECK("tg_grad_clip_coef (partials)");
    }
    // (n == 0: no partials, the sum is 0 and out2 = {0, 1})
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(kNormThreads), 0, (hipStream_t)stream, d_work, blocks, (float)max_norm, d_out2);
    TG_LAUNCH_CHECK("tg_grad_clip_coef");
    return TG_OK;
}

int tg_params_differ(const tg_adam_tensor* d_table, int32_t n_tensors, int64_t total, int32_t* d_flag, void* stream) {
    TG_REQUIRE(d_table && d_flag, "tg_params_differ: null pointer");
    TG_REQUIRE(n_tensors >= 1 && n_tensors <= kAdamMaxTensors && total >= 0, "tg_params_differ: bad sizes");
    if (total == 0) return TG_OK;
    hipLaunchKernelGGL(params_differ_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const AdamTensor*>(d_table), n_tensors, total, d_flag);
    TG_LAUNCH_CHECK("tg_params_differ");
    return TG_OK;
}

int tg_gather_streams(const tg_gather_segment* d_segments, int32_t n_segments, int64_t total, const tg_adam_tensor* d_table, void* stream) {
    TG_REQUIRE(d_segments && d_table, "tg_gather_streams: null pointer");
    TG_REQUIRE(n_segments >= 1 && n_segments <= kGatherMaxSegments, "tg_gather_streams: %d segments outside 1..%d", n_segments, kGatherMaxSegments);
    TG_REQUIRE(total >= 0, "tg_gather_streams: negative size");
    if (total == 0) return TG_OK;
    static_assert(sizeof(tg_gather_segment) == sizeof(GatherSegment), "ABI struct and kernel struct must agree");
    hipLaunchKernelGGL(gather_streams_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const GatherSegment*>(d_segments), n_segments, total, reinterpret_cast<const AdamTensor*>(d_table));
    TG_LAUNCH_CHECK("tg_gather_streams");
    return TG_OK;
}

}  // extern "C"
