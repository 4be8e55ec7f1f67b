// Shared host-side helpers for libnnue_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "nnue_hip.h"

// Records a printf-style message retrievable through nnue_hip_last_error().
void nnue_set_error(const char* fmt, ...);

#define NNUE_REQUIRE(cond, code, ...)     \
  do {                                    \
    if (!(cond)) {                        \
      nnue_set_error(__VA_ARGS__);        \
      return (code);                      \
    }                                     \
  } while (0)

static inline int nnue_launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    nnue_set_error("%s: %s", what, hipGetErrorString(e));
    return NNUE_E_LAUNCH;
  }
  return NNUE_OK;
}

static inline bool nnue_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int64_t nnue_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

constexpr int kWave = 64;  // CDNA4 wavefront

// The optimizer updates' {weight clip} x {weight average} choice of a kernel instantiation, made in one place: calls
// f(std::bool_constant<kClip>{}, std::bool_constant<kEma>{}) for the two run-time flags and returns what it returns.
template <class F>
static inline auto with_clip_ema(bool clip_on, bool ema_on, F&& f) {
  if (ema_on) return clip_on ? f(std::true_type{}, std::true_type{}) : f(std::false_type{}, std::true_type{});
  return clip_on ? f(std::true_type{}, std::false_type{}) : f(std::false_type{}, std::false_type{});
}

// Zero fills as ordinary kernels.  hipMemsetAsync captured into a hipGraph ahead of a kernel that scatters or
// accumulates into the same buffer was observed not to be ordered reliably before that kernel on this stack (ROCm 7.0:
// replayed training steps of the id-list path read stale values), so nothing in a capturable path uses memset nodes.
#ifdef __HIPCC__
// Per-sample softmax cross-entropy from the row maximum mx, the label's logit z_y and se = sum exp(z - mx).  Formed as
// (mx - z_y) + log(se): exact to a few ulp of the loss itself, where (mx + log(se)) - z_y rounds at the scale of the
// logits.  Shared by the stand-alone loss (optim_kernels.hip) and the fused classifier step (classifier_kernels.hip).
__device__ __forceinline__ float nnue_ce_sample_loss(float mx, float z_y, float se) { return (mx - z_y) + logf(se); }

// Soft targets (include/nnue_hip.h, "soft targets"): a second label and a mixing weight per sample (NULL, NULL: a2 = a,
// lam = 1) and one smoothing constant per call.  Shared by the same two places as the plain loss.
struct SoftTargets { const int64_t* labels_b; const float* lam; float eps; };
// a sample counts iff a is a class and (lam == 1 or a2 is one); otherwise its loss and its gradient row are 0
__device__ __forceinline__ bool nnue_soft_counts(int64_t a, int64_t a2, float lam, int C) {
  return a >= 0 && a < C && (lam == 1.0f || (a2 >= 0 && a2 < C));
}
// The plain form with the target spread over two labels and, by eps / C, over every class: csum = sum_c (mx - z_c).  Every
// term is non-negative and each mx - z is formed before anything is summed; with eps = 0, lam = 1 the products are exact
// and the value is nnue_ce_sample_loss(mx, z_a, se).  z_a2 of a sample whose a2 is no class (lam == 1): pass z_a.
__device__ __forceinline__ float nnue_ce_soft_sample_loss(float mx, float z_a, float z_a2, float se, float csum, float lam, float eps, int C) {
  return ((1.0f - eps) * (lam * (mx - z_a) + (1.0f - lam) * (mx - z_a2)) + logf(se)) + (eps / (float)C) * csum;
}
// t_c of the definition
__device__ __forceinline__ float nnue_soft_target(bool is_a, bool is_a2, float lam, float eps, int C) {
  return (1.0f - eps) * (lam * (is_a ? 1.0f : 0.0f) + (1.0f - lam) * (is_a2 ? 1.0f : 0.0f)) + eps / (float)C;
}

// Distillation (include/nnue_hip.h, "soft targets": the teacher arm): one row of teacher logits per sample beside the soft
// targets, a weight alpha in (0, 1] and a temperature T > 0 per call (alpha == 0 never reaches a kernel: the launcher runs
// the soft call).  The per-element arithmetic below is shared by both tail kernels and the stand-alone loss; the fmas are
// explicit so that every kernel forms the same bits whatever stands around the call.
struct DistillTargets : SoftTargets { const float* teacher; float alpha, temperature; };
// exp((v - vmax) / T): the numerator of q (v = u, vmax = mu) and of pT (v = z, vmax = mx); v - vmax is formed first
__device__ __forceinline__ float nnue_distill_exp(float v, float vmax, float T) { return expf((v - vmax) / T); }
// acc + one term of sU * sum_c q_c ((mx - z_c) - (mu - u_c)), eu = exp((u - mu) / T): the term is 0 where q underflows,
// whatever the distances
__device__ __forceinline__ float nnue_distill_kl_acc(float acc, float eu, float z, float mx, float u, float mu) {
  return fmaf(eu, (mx - z) - (mu - u), acc);
}
// loss_b from the soft loss and the three sums: KL = (log sT - log sU) + (ksum / sU) / T, both logs >= 0
__device__ __forceinline__ float nnue_distill_sample_loss(float l_soft, float sT, float sU, float ksum, float alpha, float T) {
  const float kl = (logf(sT) - logf(sU)) + (ksum / sU) / T;
  return fmaf(alpha * T * T, kl, (1.0f - alpha) * l_soft);
}
// d loss / d logit z of a sample that counts: soft = exp(z - mx) / se - t (ce_dlogit_soft's fma), ez and eu the numerators
// of pT and q, inv_sT = 1 / sT, inv_sU = 1 / sU
__device__ __forceinline__ float nnue_distill_dlogit(float soft, float ez, float inv_sT, float eu, float inv_sU, float alpha, float T,
                                                     float scale_over_b) {
  const float d = fmaf(ez, inv_sT, -(eu * inv_sU));
  return fmaf(alpha * T, d, (1.0f - alpha) * soft) * scale_over_b;
}

namespace {
__global__ __launch_bounds__(256) void nnue_zero_floats_kernel(float* __restrict__ dst, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) dst[i] = 0.0f;
}
__global__ __launch_bounds__(256) void nnue_zero_counters_kernel(int* __restrict__ n, float* __restrict__ sink, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B) {
    n[i] = 0;
    sink[i] = 0.0f;
  }
}
}  // namespace
__attribute__((unused)) static inline void nnue_zero_floats(float* dst, size_t count, hipStream_t s) {
  if (count) hipLaunchKernelGGL(nnue_zero_floats_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, dst, count);
}
__attribute__((unused)) static inline void nnue_zero_counters(int* n, float* sink, int B, hipStream_t s) {
  hipLaunchKernelGGL(nnue_zero_counters_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, n, sink, B);
}
#endif

