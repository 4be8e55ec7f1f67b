// Loss and step tail on gfx950: mean cross-entropy with its gradient (train.py:250-254) and
// clip_grad_norm_ + SGD(momentum, weight_decay) / Adam on one flat buffer or on a list of separate tensors
// (train.py:363-366, :457-471).
// Both are small streaming kernels; sums are staged so results are bitwise reproducible.
#include "common.h"

#include <cstdlib>

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s));
  return v;
}

// one wave per sample
__global__ __launch_bounds__(256) void cross_entropy_kernel(const float* __restrict__ logits,
                                                            const int64_t* __restrict__ labels, int B, int C,
                                                            float scale_over_b, float* __restrict__ sample_loss,
                                                            float* __restrict__ d_logits) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const float* __restrict__ z = logits + (size_t)b * C;
  float mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, z[c]);
  mx = wave_max(mx);
  float se = 0.f;
  for (int c = lane; c < C; c += 64) se += expf(z[c] - mx);
  se = wave_sum(se);
  const int64_t y = labels[b];
  const bool ok = y >= 0 && y < C;
  if (lane == 0) sample_loss[b] = ok ? nnue_ce_sample_loss(mx, z[y], se) : 0.0f;
  if (d_logits) {
    const float inv = 1.0f / se;
    for (int c = lane; c < C; c += 64) {
      const float p = expf(z[c] - mx) * inv;
      d_logits[(size_t)b * C + c] = ok ? (p - (c == y ? 1.0f : 0.0f)) * scale_over_b : 0.0f;
    }
  }
}

// single block: fixed-order mean of the per-sample losses
__global__ __launch_bounds__(256) void mean_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *out = ((red[0] + red[1]) + (red[2] + red[3])) / (float)n;
}

// evaluation: argmax (first maximum, as numpy: a NaN beats every number and the first NaN wins) and one integer atomic per
// sample into the confusion matrix;
// C == 1 is the reference's binary rule (output > 0.5 vs target > 0.5)
__global__ __launch_bounds__(256) void confusion_kernel(const float* __restrict__ logits,
                                                        const int64_t* __restrict__ labels, int B, int C, int K,
                                                        unsigned long long* __restrict__ confusion) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* __restrict__ z = logits + (size_t)b * C;
  int pred, truth;
  if (C == 1) {
    pred = z[0] > 0.5f ? 1 : 0;
    truth = labels[b] > 0 ? 1 : 0;  // integer labels: > 0.5  <=>  >= 1
  } else {
    pred = 0;
    float best = z[0];
    for (int c = 1; c < C && best == best; ++c)
      if (!(z[c] <= best)) {  // greater, or NaN
        best = z[c];
        pred = c;
      }
    const int64_t y = labels[b];
    if (y < 0 || y >= K) return;  // out-of-range label: not counted (caller validates)
    truth = (int)y;
  }
  atomicAdd(&confusion[(size_t)truth * K + pred], 1ull);
}

constexpr int kNormBlocks = 1024;

// clip_grad_norm_'s coefficient, clamp(max_norm / (norm + 1e-6), max=1) as torch forms it: a NaN norm gives a NaN
// coefficient (every gradient becomes NaN, as in the reference), where fminf would drop the NaN and apply 1.
// max_norm <= 0: no clipping.
__device__ __forceinline__ float clip_coefficient(float norm, float max_norm) {
  if (!(max_norm > 0.0f)) return 1.0f;
  const float c = max_norm / (norm + 1e-6f);
  return c > 1.0f ? 1.0f : c;
}

#include "optim_update.h"  // sgd_update, AdamBias, adam_bias_correction, adam_update: shared with the product epilogues

// The weight clip of a flat buffer (include/nnue_hip.h, "weight clip"), by value in the kernel arguments: the bound and up to
// four half-open element ranges of the buffer (unused ones empty).  The apply kernels take it as their last argument.  The SGD
// kernels are compiled twice: kClip = false is the kernel without it, instruction for instruction, and what a bound of 0 launches;
// the Adam kernel branches on the bound (see adam_apply_ext_kernel).
struct FlatClip {
  float bound;
  int64_t lo[4], hi[4];
  __device__ __forceinline__ bool covers(int64_t i) const {
    return (i >= lo[0] && i < hi[0]) || (i >= lo[1] && i < hi[1]) || (i >= lo[2] && i < hi[2]) || (i >= lo[3] && i < hi[3]);
  }
  __device__ __forceinline__ float apply(int64_t i, float w) const { return covers(i) ? clip_weight(w, bound) : w; }
};

// The weight average of a flat buffer (include/nnue_hip.h, "weight average"), by value in the kernel arguments behind the clip:
// the average's buffer, laid out like the parameters (NULL: off), and its rate 1 - decay as a float or -- where omd_dev is not
// NULL -- as the device scalar that replaces it, as lr_dev replaces lr.  The SGD kernels are compiled once more with kEma (the
// kernels without it keep their text); the Adam kernels branch on the pointer, as they do on the clip's bound.
struct FlatEma {
  float* __restrict__ e;
  float omd;
  const float* __restrict__ omd_dev;
  __device__ __forceinline__ float rate() const { return omd_dev ? omd_dev[0] : omd; }
};

// Block partial of sum (g * scale)^2: 16-byte loads, four independent chains per thread (the 268 MB gradient of
// the 224x224 configuration is one streaming read; a dependent scalar chain reached only 1.25 TB/s).
__device__ __forceinline__ float sqnorm_block_partial(const float* __restrict__ g, int64_t count, float scale, float* red,
                                                      int blk, int nblk) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  const int64_t stride = (int64_t)nblk * 256;
  const int64_t tid = (int64_t)blk * 256 + threadIdx.x;
  const int64_t n4 = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? (count >> 2) : 0;
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
  auto sq = [&](float4 v, float a) {
    v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
    return fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, a))));
  };
  int64_t i = tid;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const float4 v0 = g4[i], v1 = g4[i + stride], v2 = g4[i + 2 * stride], v3 = g4[i + 3 * stride];
    a0 = sq(v0, a0); a1 = sq(v1, a1); a2 = sq(v2, a2); a3 = sq(v3, a3);
  }
  for (; i < n4; i += stride) a0 = sq(g4[i], a0);
  for (int64_t j = n4 * 4 + tid; j < count; j += stride) {
    const float v = g[j] * scale;
    a1 = fmaf(v, v, a1);
  }
  float acc = wave_sum((a0 + a1) + (a2 + a3));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// The plain block partial over g[0, count) without [lo, hi) (a producer already summed that range; lo == hi: nothing
// skipped).  Two passes through the same routine; the barrier between them protects the reduction buffer.
__device__ __forceinline__ float sqnorm_block_partial_skip(const float* __restrict__ g, int64_t count, float scale, float* red, int blk,
                                                           int nblk, int64_t lo, int64_t hi) {
  if (lo >= hi) return sqnorm_block_partial(g, count, scale, red, blk, nblk);
  const float a = sqnorm_block_partial(g, lo, scale, red, blk, nblk);
  __syncthreads();
  const float b = sqnorm_block_partial(g + hi, count - hi, scale, red, blk, nblk);
  return a + b;
}

__global__ __launch_bounds__(256) void sqnorm_stage1(const float* __restrict__ g, int64_t count, float scale,
                                                     float* __restrict__ partial, int64_t lo, int64_t hi) {
  __shared__ float red[4];
  const float v = sqnorm_block_partial_skip(g, count, scale, red, blockIdx.x, gridDim.x, lo, hi);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

// The norm launch with the second stage of a deferred nnue_ste_conv_backward riding in it (feature_kernels.hip,
// ste_conv_backward_stage2: one wave per (channel, term), lanes stride over the output's contiguous run of partials,
// the same sums in the same order).  Workgroups [0, s2_blocks) write d_thr / d_weight -- the first `skip` elements of
// g -- and leave the squares of their four outputs in partial[nb + block] (nb = plain norm workgroups); the others are the plain norm
// workgroups over g[skip:].
__global__ __launch_bounds__(256) void sqnorm_stage1_ste(const float* __restrict__ g, int64_t count, float scale,
                                                         float* __restrict__ partial, const float* __restrict__ ste_partial,
                                                         int chunks, int fps, float* __restrict__ d_thr,
                                                         float* __restrict__ d_weight, int s2_blocks, int64_t skip, int64_t lo,
                                                         int64_t hi, int nb) {
  __shared__ float red[4];
  if ((int)blockIdx.x >= s2_blocks) {
    const float v = sqnorm_block_partial_skip(g + skip, count - skip, scale, red, (int)blockIdx.x - s2_blocks, nb,
                                              lo > skip ? lo - skip : 0, hi > skip ? hi - skip : 0);
    if (threadIdx.x == 0) partial[blockIdx.x - s2_blocks] = v;
    return;
  }
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  float sq = 0.0f;
  if (o < fps * 28) {
    const int c = o / 28, q = o - c * 28;
    const float* __restrict__ run = ste_partial + (size_t)o * chunks;
    float acc = 0.0f;
    int k = lane;
    for (; k + 7 * 64 < chunks; k += 8 * 64) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = run[k + 64 * u];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; k < chunks; k += 64) acc += run[k];
    acc = wave_sum(acc);
    if (lane == 0) {
      if (q == 27) d_thr[c] = -acc;
      else d_weight[c * 27 + q] = acc;
    }
    sq = (acc * scale) * (acc * scale);
  }
  if (lane == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) partial[nb + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The norm step of every apply kernel.  Every block re-derives the norm from the norm launch's partials (at most 4 KiB,
// L2-resident) in the same fixed order -- plus, where given, a producer's sums of squares (unscaled) of the range the norm launch
// skipped -- before it streams its share of the update.  Returns clip_grad_norm_'s coefficient; the first workgroup leaves the
// norm in norm_out and the coefficient in coef_out (for the producer that applies [skip_lo, skip_hi) itself) where they are given.
__device__ __forceinline__ float clip_from_partials(const float* __restrict__ partial, int nparts, const float* __restrict__ ext_partial,
                                                    int ext_count, float scale, float max_norm, float* __restrict__ norm_out,
                                                    float* __restrict__ coef_out) {
  __shared__ double red[4];
  __shared__ float coef_s;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += (double)partial[i];
  if (ext_partial) {
    const double s2 = (double)scale * (double)scale;
    for (int i = threadIdx.x; i < ext_count; i += 256) acc += (double)ext_partial[i] * s2;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
    if (norm_out && blockIdx.x == 0) *norm_out = norm;
    coef_s = clip_coefficient(norm, max_norm);
    if (coef_out && blockIdx.x == 0) *coef_out = coef_s;
  }
  __syncthreads();
  return coef_s;
}

template <bool kClip, bool kEma>
__global__ __launch_bounds__(256) void sgd_apply_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, int64_t count, float lr, float momentum,
                                                        float wd, float max_norm, float scale, int first_step,
                                                        const float* __restrict__ partial, int nparts,
                                                        float* __restrict__ norm_out, const float* __restrict__ ext_partial,
                                                        int ext_count, float* __restrict__ coef_out, int64_t skip_lo, int64_t skip_hi,
                                                        const float* __restrict__ lr_dev, const FlatClip fc, const FlatEma fe) {
  if (lr_dev) lr = lr_dev[0];  // the learning rate as a device scalar: a scheduler changes it without re-capturing the step
  float omd = 0.0f;
  if constexpr (kEma) omd = fe.rate();
  // The first kPre passes of this thread's share are requested BEFORE the norm is re-derived: after a kernel boundary
  // both the partials and the parameters are first touches (~2 us each from a cold L2), and the two waits would
  // otherwise run one after the other.  Unconditional loads from clamped indices; results used only where valid.  (live == 0,
  // the hole is the whole buffer: no index is valid and nothing is read; the launch still writes norm_out / coef_out.)
  constexpr int kPre = 4;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t hole = skip_hi - skip_lo;  // 0: everything is updated here
  const int64_t live = count - hole, j0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float pw[kPre] = {}, pg[kPre] = {}, pm[kPre] = {}, pe[kPre] = {};
#pragma unroll
  for (int u = 0; u < kPre && live > 0; ++u) {
    const int64_t j = j0 + u * stride < live ? j0 + u * stride : 0;
    const int64_t i = j < skip_lo ? j : j + hole;
    pw[u] = p[i];
    pg[u] = g[i];
    pm[u] = (m && !first_step) ? m[i] : 0.0f;
    if constexpr (kEma) pe[u] = fe.e[i];  // the average is requested together with the parameters
  }
  float clip = 1.0f;
  if (max_norm > 0.0f || norm_out || coef_out) {
    clip = clip_from_partials(partial, nparts, ext_partial, ext_count, scale, max_norm, norm_out, coef_out);
  }
  const float gs = clip * scale;
#pragma unroll
  for (int u = 0; u < kPre; ++u) {
    const int64_t j = j0 + u * stride;
    if (j < live) {
      const int64_t i = j < skip_lo ? j : j + hole;
      float mn;
      float wn = sgd_update(pw[u], pg[u], pm[u], mn, gs, lr, momentum, wd, m != nullptr, first_step);
      if constexpr (kClip) wn = fc.apply(i, wn);
      p[i] = wn;
      if (m) m[i] = mn;
      if constexpr (kEma) fe.e[i] = ema_update(pe[u], wn, omd);
    }
  }
  for (int64_t j = j0 + kPre * stride; j < live; j += stride) {
    const int64_t i = j < skip_lo ? j : j + hole;
    float mn;
    float wn = sgd_update(p[i], g[i], (m && !first_step) ? m[i] : 0.0f, mn, gs, lr, momentum, wd, m != nullptr, first_step);
    if constexpr (kClip) wn = fc.apply(i, wn);
    p[i] = wn;
    if (m) m[i] = mn;
    if constexpr (kEma) fe.e[i] = ema_update(fe.e[i], wn, omd);
  }
}

// The same update with 16-byte accesses for buffers that are launch-sized (count, the hole and the pointers multiples of 4 /
// 16 bytes): one float4 per thread and pass, the first two passes requested before the norm is re-derived.  (The scalar kernel
// stays for big buffers: with 16-byte accesses it streamed 1.34 GB slower, 225-257 vs 211 us.)  kClip: every boundary of the
// clip's ranges is a multiple of 4 (the entry point checks it), so a float4 lies inside a range or outside it.
template <bool kClip, bool kEma>
__global__ __launch_bounds__(256) void sgd_apply_vec_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            int64_t count, float lr, float momentum, float wd, float max_norm, float scale,
                                                            int first_step, const float* __restrict__ partial, int nparts,
                                                            float* __restrict__ norm_out, const float* __restrict__ ext_partial, int ext_count,
                                                            float* __restrict__ coef_out, int64_t skip_lo, int64_t skip_hi,
                                                            const float* __restrict__ lr_dev, const FlatClip fc, const FlatEma fe) {
  if (lr_dev) lr = lr_dev[0];
  float omd = 0.0f;
  if constexpr (kEma) omd = fe.rate();
  constexpr int kPre = 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t hole4 = (skip_hi - skip_lo) >> 2, lo4 = skip_lo >> 2, live4 = (count >> 2) - hole4;
  const int64_t j0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
  const float4* __restrict__ m4 = reinterpret_cast<const float4*>(m);
  float4* __restrict__ e4 = reinterpret_cast<float4*>(fe.e);
  float4 pw[kPre] = {}, pg[kPre] = {}, pm[kPre] = {}, pe[kPre] = {};
#pragma unroll
  for (int u = 0; u < kPre && live4 > 0; ++u) {  // live4 == 0: nothing to read (see sgd_apply_kernel)
    const int64_t j = j0 + u * stride < live4 ? j0 + u * stride : 0;
    const int64_t i = j < lo4 ? j : j + hole4;
    pw[u] = p4[i];
    pg[u] = g4[i];
    pm[u] = (m && !first_step) ? m4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (kEma) pe[u] = e4[i];  // the average is requested together with the parameters
  }
  float clip = 1.0f;
  if (max_norm > 0.0f || norm_out || coef_out) {
    clip = clip_from_partials(partial, nparts, ext_partial, ext_count, scale, max_norm, norm_out, coef_out);
  }
  const float gs = clip * scale;
  auto one = [&](float w, float gv, float mv, float& m_new) {
    return sgd_update(w, gv, mv, m_new, gs, lr, momentum, wd, m != nullptr, first_step);
  };
  auto apply = [&](int64_t i, const float4& w, const float4& gv, const float4& mv, const float4& ev) {
    float4 mn, wn;
    wn.x = one(w.x, gv.x, mv.x, mn.x); wn.y = one(w.y, gv.y, mv.y, mn.y);
    wn.z = one(w.z, gv.z, mv.z, mn.z); wn.w = one(w.w, gv.w, mv.w, mn.w);
    if constexpr (kClip) {
      if (fc.covers(4 * i)) {
        wn.x = clip_weight(wn.x, fc.bound); wn.y = clip_weight(wn.y, fc.bound);
        wn.z = clip_weight(wn.z, fc.bound); wn.w = clip_weight(wn.w, fc.bound);
      }
    }
    if (m) reinterpret_cast<float4*>(m)[i] = mn;
    reinterpret_cast<float4*>(p)[i] = wn;
    if constexpr (kEma)
      e4[i] = make_float4(ema_update(ev.x, wn.x, omd), ema_update(ev.y, wn.y, omd), ema_update(ev.z, wn.z, omd), ema_update(ev.w, wn.w, omd));
  };
#pragma unroll
  for (int u = 0; u < kPre; ++u) {
    const int64_t j = j0 + u * stride;
    if (j < live4) apply(j < lo4 ? j : j + hole4, pw[u], pg[u], pm[u], pe[u]);
  }
  for (int64_t j = j0 + kPre * stride; j < live4; j += stride) {
    const int64_t i = j < lo4 ? j : j + hole4;
    float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (kEma) ev = e4[i];
    apply(i, p4[i], g4[i], (m && !first_step) ? m4[i] : make_float4(0.f, 0.f, 0.f, 0.f), ev);
  }
}

// Adam (torch.optim.Adam defaults: L2 weight decay folded into the gradient, bias-corrected moments, no
// amsgrad).  The step number lives in device memory (step_counter[0], incremented here by the norm kernel's
// first thread) so that the launch has no changing host argument and can be replayed from a hipGraph.
// kSkip (nnue_adam_step_ext): the norm launch skips [lo, hi) of the gradient -- a producer left that range's sums of squares.
template <bool kSkip>
__global__ __launch_bounds__(256) void sqnorm_stage1_count(const float* __restrict__ g, int64_t count, float scale,
                                                           float* __restrict__ partial, int* __restrict__ step_counter, int64_t lo,
                                                           int64_t hi) {
  __shared__ float red[4];
  if (blockIdx.x == 0 && threadIdx.x == 0) step_counter[0] += 1;
  const float v = kSkip ? sqnorm_block_partial_skip(g, count, scale, red, blockIdx.x, gridDim.x, lo, hi)
                        : sqnorm_block_partial(g, count, scale, red, blockIdx.x, gridDim.x);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

// The apply launch of nnue_adam_step (kExt = false) and of nnue_adam_step_ext (kExt = true: it adds the producer's partials to the
// norm, leaves the clip coefficient in coef_out and -- with skip_lo < skip_hi -- does not touch that range, whose producer applies
// the update itself; without kExt those arguments are not read).
// The weight clip here is a uniform branch on the descriptor's bound (0: off), not a second instantiation: adam_update leaves its
// multiply-adds to the compiler's contraction (optim_update.h), and a clamping instantiation of this kernel was compiled with one
// of them fused that the plain one keeps apart (one ulp) -- with one text both arms share the arithmetic, and it is the
// arithmetic the kernel had before the clip existed (compared instruction by instruction).  The average is a uniform branch on
// its pointer for the same reason.
template <bool kExt>
__global__ __launch_bounds__(256) void adam_apply_ext_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, int64_t count, float lr, float beta1, float beta2,
                                                             float eps, float wd, float max_norm, float scale,
                                                             const int* __restrict__ step_counter, const float* __restrict__ partial,
                                                             int nparts, float* __restrict__ norm_out,
                                                             const float* __restrict__ ext_partial, int ext_count,
                                                             float* __restrict__ coef_out, int64_t skip_lo, int64_t skip_hi,
                                                             const float* __restrict__ lr_dev, const FlatClip fc, const FlatEma fe) {
  if (lr_dev) lr = lr_dev[0];
  const float gs = clip_from_partials(partial, nparts, kExt ? ext_partial : nullptr, kExt ? ext_count : 0, scale, max_norm, norm_out,
                                      kExt ? coef_out : nullptr) * scale;
  const AdamBias bc = adam_bias_correction(lr, beta1, beta2, step_counter[0]);
  const float omd = fe.e ? fe.rate() : 0.0f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t hole = kExt ? skip_hi - skip_lo : 0, live = count - hole;  // hole 0: everything is updated here
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < live; j += stride) {
    const int64_t i = (!kExt || j < skip_lo) ? j : j + hole;
    float mi = m[i], vi = v[i];
    float wn = adam_update(p[i], g[i], mi, vi, gs, bc, beta1, beta2, eps, wd);
    if (fc.bound > 0.0f) wn = fc.apply(i, wn);  // (uniform; see the note above)
    p[i] = wn;
    m[i] = mi;
    v[i] = vi;
    if (fe.e) fe.e[i] = ema_update(fe.e[i], wn, omd);  // (uniform, like the clip: one text, the plain arm's arithmetic unchanged)
  }
}


// The stand-alone pass of the weight average: e <- ema_update(e, w, omd).  kVec: both pointers 16-byte aligned -- float4 q covers
// elements [4q, 4q + 4), and the count % 4 elements behind the last whole one are taken one per thread by the first workgroup.
template <bool kVec>
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ e, const float* __restrict__ w, int64_t count, float omd,
                                                         const float* __restrict__ omd_dev) {
  if (omd_dev) omd = omd_dev[0];
  const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if constexpr (kVec) {
    const int64_t n4 = count >> 2;
    float4* __restrict__ e4 = reinterpret_cast<float4*>(e);
    const float4* __restrict__ w4 = reinterpret_cast<const float4*>(w);
    for (int64_t i = t0; i < n4; i += stride) {
      const float4 ev = e4[i], wv = w4[i];
      e4[i] = make_float4(ema_update(ev.x, wv.x, omd), ema_update(ev.y, wv.y, omd), ema_update(ev.z, wv.z, omd), ema_update(ev.w, wv.w, omd));
    }
    const int64_t i = 4 * n4 + t0;
    if (t0 < 4 && i < count) e[i] = ema_update(e[i], w[i], omd);
  } else {
    for (int64_t i = t0; i < count; i += stride) e[i] = ema_update(e[i], w[i], omd);
  }
}

// ---- the multi-tensor form: torch.optim's list of separate parameters (one segment per tensor, any sizes, any views) ----
// Stage 1 writes one sum-of-squares partial per kMultiChunk elements of each segment, segments in list order; stage 2's
// workgroups re-derive the global norm from all partials (fixed order, double) and stream kMultiUnit-element units of the
// update through the per-element helpers above.  The segment table rides in the kernel arguments, so a step has no host-to-
// device copy; a list longer than one table is split over several launches that write disjoint ranges of the partials.
constexpr int kMultiChunk = 16384;       // elements per norm partial (4096 partials for the 268 MB table of the 224x224 model)
constexpr int kMultiUnit = 4096;         // elements per apply unit: 256 threads x 4 float4
constexpr int kMultiApplyBlocks = 2048;  // apply grid cap: each workgroup then streams >= 8 units of a big table per re-reduction
constexpr int kMultiSegs = 45;

struct MultiSeg {
  float* p;
  const float* g;
  float* m;       // SGD momentum buffer (NULL: momentum 0) / Adam exp_avg
  float* v;       // Adam exp_avg_sq
  int32_t* step;  // Adam step counter (device)
  int64_t count;
  int32_t chunk0, unit0;  // this segment's first norm chunk / apply unit within the launch
  float lr, a, b, wd, eps;  // a: momentum or beta1; b: beta2
  int32_t first;            // SGD: no momentum buffer yet (the update writes it without reading)
  float clip;               // weight clip of this segment (include/nnue_hip.h, "weight clip"); 0: not clamped
};

template <int kSegs>
struct MultiArgsT {
  static constexpr int kCap = kSegs;
  static constexpr bool kEma = false;
  float* partial;      // all partials of the list (the apply reads [0, nparts))
  float* norm_out;     // pre-clip norm (first apply launch only), may be NULL
  const float* lr_dev; // n device floats replacing lr, indexed by seg_base + segment; may be NULL
  int32_t nparts, part_base, seg_base, n, chunks, units, need_norm;
  float max_norm;
  MultiSeg seg[kSegs];
};
using MultiArgs = MultiArgsT<kMultiSegs>;
static_assert(sizeof(MultiArgs) <= 4096, "the segment table must fit the 4 KiB kernel-argument budget");

// The table of a list that keeps a weight average (include/nnue_hip.h, "weight average"): per segment the average's buffer (NULL:
// that segment is off) and its rate.  A table of its own with fewer segments, so the lists without an average keep their
// 45-segment launches.
constexpr int kMultiSegsEma = 38;
struct MultiArgsEma : MultiArgsT<kMultiSegsEma> {
  static constexpr bool kEma = true;
  float* e[kMultiSegsEma];
  float omd[kMultiSegsEma];
};
static_assert(sizeof(MultiArgsEma) <= 4096, "the segment table must fit the 4 KiB kernel-argument budget");

// the last segment whose first chunk (by_unit: unit) is <= x; x is wave-uniform, so these are scalar loads of the arguments
template <class Args>
__device__ __forceinline__ int multi_find(const Args& A, int x, bool by_unit) {
  int lo = 0, hi = A.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((by_unit ? A.seg[mid].unit0 : A.seg[mid].chunk0) <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float sq4(float4 x, float a) { return fmaf(x.w, x.w, fmaf(x.z, x.z, fmaf(x.y, x.y, fmaf(x.x, x.x, a)))); }

// Stage 1.  Element e0 + it*4096 + j*1024 + 4*thread + k of a chunk always enters chain j in the same position, whether it
// arrives in a 16-byte load (g aligned, whole chunk in range) or in guarded scalar loads (a misaligned view, the ragged
// last chunk): the partial does not depend on where the gradient happens to lie.  Adam: the first workgroup also
// advances the segments' step counters (as sqnorm_stage1_count does).
template <class Args>
__global__ __launch_bounds__(256) void multi_sqnorm_kernel(const Args A) {
  __shared__ float red[4];
  if (blockIdx.x == 0 && (int)threadIdx.x < A.n && A.seg[threadIdx.x].step) A.seg[threadIdx.x].step[0] += 1;
  if (!A.need_norm) return;
  const int c = blockIdx.x;
  const MultiSeg& S = A.seg[multi_find(A, c, false)];
  const float* __restrict__ g = S.g;
  const int64_t e0 = (int64_t)(c - S.chunk0) * kMultiChunk + 4 * threadIdx.x;
  constexpr int kIt = kMultiChunk / kMultiUnit;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0 && (int64_t)(c - S.chunk0 + 1) * kMultiChunk <= S.count) {
    float4 x[kIt][4];
#pragma unroll
    for (int it = 0; it < kIt; ++it)
#pragma unroll
      for (int j = 0; j < 4; ++j) x[it][j] = *reinterpret_cast<const float4*>(g + e0 + it * kMultiUnit + j * 1024);
#pragma unroll
    for (int it = 0; it < kIt; ++it)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = sq4(x[it][j], a[j]);
  } else {
    for (int it = 0; it < kIt; ++it)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t i = e0 + it * kMultiUnit + j * 1024;
        float4 x;
        x.x = i < S.count ? g[i] : 0.0f;
        x.y = i + 1 < S.count ? g[i + 1] : 0.0f;
        x.z = i + 2 < S.count ? g[i + 2] : 0.0f;
        x.w = i + 3 < S.count ? g[i + 3] : 0.0f;
        a[j] = sq4(x, a[j]);
      }
  }
  const float acc = wave_sum((a[0] + a[1]) + (a[2] + a[3]));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) A.partial[A.part_base + c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One apply unit in registers.  Vector form (p, g and the state share their offset within 16 bytes): float4 q of the
// segment starts at element head + 4q, and unit k holds float4s k*1024 + j*256 + thread; the < 4 elements before the first
// aligned one (head) go with unit 0, those after the last whole float4 (tail) with the segment's last unit.  Scalar form
// (mixed offsets): unit k holds elements k*4096 + r*256 + thread.
template <bool kAdam>
struct MultiUnit {
  float4 w[4], g[4], m[4], v[4];
  int64_t base;  // vector form: element of the unit's first float4; scalar form: first element of the unit
  int lim;       // elements of the segment from base on, capped at one unit
  bool vec;

  // component c of quad j: vector form element 4*(j*256 + thread) + c; scalar form element (4*j + c)*256 + thread.  The
  // wave-uniform base pointer keeps the per-thread offset 32-bit and shared by all quads.
  __device__ __forceinline__ int offset(int j, int c) const {
    return vec ? 4 * (j * 256 + (int)threadIdx.x) + c : (4 * j + c) * 256 + (int)threadIdx.x;
  }

  __device__ __forceinline__ void load(const MultiSeg& S, int k, bool read_m) {
    const uintptr_t off = reinterpret_cast<uintptr_t>(S.p) & 15;
    vec = (reinterpret_cast<uintptr_t>(S.g) & 15) == off && (!S.m || (reinterpret_cast<uintptr_t>(S.m) & 15) == off) &&
          (!kAdam || (reinterpret_cast<uintptr_t>(S.v) & 15) == off);
    base = (int64_t)k * kMultiUnit + (vec ? (int64_t)((16 - off) & 15) / 4 : 0);
    lim = S.count - base < kMultiUnit + 16 ? (int)(S.count - base) : kMultiUnit + 16;
    const float* __restrict__ P = S.p + base;
    const float* __restrict__ G = S.g + base;
    const float* __restrict__ M = S.m + base;
    const float* __restrict__ V = S.v + base;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = g[j] = m[j] = v[j] = z;
      if (vec) {
        const int o = offset(j, 0);
        if (o + 4 <= lim) {
          w[j] = *reinterpret_cast<const float4*>(P + o);
          g[j] = *reinterpret_cast<const float4*>(G + o);
          if (read_m) m[j] = *reinterpret_cast<const float4*>(M + o);
          if (kAdam) v[j] = *reinterpret_cast<const float4*>(V + o);
        }
      } else {
        auto one = [&](int c, float& wc, float& gc, float& mc, float& vc) {
          const int o = offset(j, c);
          if (o >= lim) return;
          wc = P[o];
          gc = G[o];
          if (read_m) mc = M[o];
          if (kAdam) vc = V[o];
        };
        one(0, w[j].x, g[j].x, m[j].x, v[j].x);
        one(1, w[j].y, g[j].y, m[j].y, v[j].y);
        one(2, w[j].z, g[j].z, m[j].z, v[j].z);
        one(3, w[j].w, g[j].w, m[j].w, v[j].w);
      }
    }
  }

  __device__ __forceinline__ void store(const MultiSeg& S) const {
    float* __restrict__ P = S.p + base;
    float* __restrict__ M = S.m + base;
    float* __restrict__ V = S.v + base;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (vec) {
        const int o = offset(j, 0);
        if (o + 4 > lim) continue;
        *reinterpret_cast<float4*>(P + o) = w[j];
        if (S.m) *reinterpret_cast<float4*>(M + o) = m[j];
        if (kAdam) *reinterpret_cast<float4*>(V + o) = v[j];
      } else {
        auto one = [&](int c, float wc, float mc, float vc) {
          const int o = offset(j, c);
          if (o >= lim) return;
          P[o] = wc;
          if (S.m) M[o] = mc;
          if (kAdam) V[o] = vc;
        };
        one(0, w[j].x, m[j].x, v[j].x);
        one(1, w[j].y, m[j].y, v[j].y);
        one(2, w[j].z, m[j].z, v[j].z);
        one(3, w[j].w, m[j].w, v[j].w);
      }
    }
  }

  // the unit's new weights (w, after the update) into the segment's average: 16-byte accesses where the unit is in its vector
  // form and the average shares the parameters' offset within 16 bytes, else one element at a time
  __device__ __forceinline__ void average(const MultiSeg& S, float* __restrict__ ema, float omd) const {
    float* __restrict__ E = ema + base;
    const bool evec = vec && ((reinterpret_cast<uintptr_t>(ema) ^ reinterpret_cast<uintptr_t>(S.p)) & 15) == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (evec) {
        const int o = offset(j, 0);
        if (o + 4 > lim) continue;
        const float4 ev = *reinterpret_cast<const float4*>(E + o);
        *reinterpret_cast<float4*>(E + o) = make_float4(ema_update(ev.x, w[j].x, omd), ema_update(ev.y, w[j].y, omd),
                                                        ema_update(ev.z, w[j].z, omd), ema_update(ev.w, w[j].w, omd));
      } else {
        auto one = [&](int c, float wc) {
          const int o = vec ? offset(j, 0) + c : offset(j, c);
          if (vec ? offset(j, 0) + 4 > lim : o >= lim) return;
          E[o] = ema_update(E[o], wc, omd);
        };
        one(0, w[j].x);
        one(1, w[j].y);
        one(2, w[j].z);
        one(3, w[j].w);
      }
    }
  }
};

// the per-segment constants of the update: learning rate (lr_dev wins) and, for Adam, the bias corrections of the step
// stage 1 has just counted
struct MultiHyper {
  float lr;
  AdamBias bc;
};
template <bool kAdam, class Args>
__device__ __forceinline__ MultiHyper multi_hyper(const Args& A, int s) {
  const MultiSeg& S = A.seg[s];
  MultiHyper h;
  h.lr = A.lr_dev ? A.lr_dev[A.seg_base + s] : S.lr;
  h.bc = kAdam ? adam_bias_correction(h.lr, S.a, S.b, S.step[0]) : AdamBias{0.f, 0.f};
  return h;
}

template <bool kAdam>
__device__ __forceinline__ float multi_update(const MultiSeg& S, const MultiHyper& h, float w, float g, float& m, float& v, float gs) {
  float out;
  if (kAdam) {
    out = adam_update(w, g, m, v, gs, h.bc, S.a, S.b, S.eps, S.wd);
  } else {
    float mn;
    out = sgd_update(w, g, m, mn, gs, h.lr, S.a, S.wd, S.m != nullptr, S.first != 0);
    m = mn;
  }
  return S.clip > 0.0f ? clip_weight(out, S.clip) : out;  // (wave-uniform: the segment's)
}

// Stage 2.  The first unit is requested before the norm is re-derived (both are first touches after the kernel boundary).
template <bool kAdam, class Args>
__global__ __launch_bounds__(256) void multi_apply_kernel(const Args A) {
  int u = blockIdx.x;
  int s = multi_find(A, u, true);
  MultiUnit<kAdam> U;
  U.load(A.seg[s], u - A.seg[s].unit0, A.seg[s].m && (kAdam || !A.seg[s].first));
  float clip = 1.0f;
  if (A.need_norm) clip = clip_from_partials(A.partial, A.nparts, nullptr, 0, 1.0f, A.max_norm, A.norm_out, nullptr);
  int hs = s;
  MultiHyper h = multi_hyper<kAdam>(A, s);
  while (true) {
    const MultiSeg& S = A.seg[s];
    if (hs != s) {
      h = multi_hyper<kAdam>(A, s);
      hs = s;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      U.w[j].x = multi_update<kAdam>(S, h, U.w[j].x, U.g[j].x, U.m[j].x, U.v[j].x, clip);
      U.w[j].y = multi_update<kAdam>(S, h, U.w[j].y, U.g[j].y, U.m[j].y, U.v[j].y, clip);
      U.w[j].z = multi_update<kAdam>(S, h, U.w[j].z, U.g[j].z, U.m[j].z, U.v[j].z, clip);
      U.w[j].w = multi_update<kAdam>(S, h, U.w[j].w, U.g[j].w, U.m[j].w, U.v[j].w, clip);
    }
    U.store(S);
    if constexpr (Args::kEma) {
      if (A.e[s]) U.average(S, A.e[s], A.omd[s]);  // (wave-uniform: the segment's)
    }
    // vector form: the head (unit 0) and the tail (last unit) elements, one per thread (tiny segments have both)
    const int k = u - S.unit0;
    if (U.vec) {
      const int64_t head = U.base - (int64_t)k * kMultiUnit, t = threadIdx.x;  // head < 4
      const int64_t tail0 = S.count <= head ? S.count : head + ((S.count - head) & ~(int64_t)3);
      const bool last = (int64_t)(k + 1) * kMultiUnit >= S.count;
      for (int pass = 0; pass < 2; ++pass) {
        const int64_t e = pass == 0 ? (k == 0 && t < head && t < S.count ? t : -1) : (last && tail0 + t < S.count ? tail0 + t : -1);
        if (e < 0) continue;
        float mv = (S.m && (kAdam || !S.first)) ? S.m[e] : 0.0f, vv = kAdam ? S.v[e] : 0.0f;
        const float wn = multi_update<kAdam>(S, h, S.p[e], S.g[e], mv, vv, clip);
        S.p[e] = wn;
        if constexpr (Args::kEma) {
          if (A.e[s]) A.e[s][e] = ema_update(A.e[s][e], wn, A.omd[s]);
        }
        if (S.m) S.m[e] = mv;
        if (kAdam) S.v[e] = vv;
      }
    }
    u += gridDim.x;
    if (u >= A.units) break;
    while (s + 1 < A.n && A.seg[s + 1].unit0 <= u) ++s;
    U.load(A.seg[s], u - A.seg[s].unit0, A.seg[s].m && (kAdam || !A.seg[s].first));
  }
}

}  // namespace

extern "C" int nnue_cross_entropy(const float* logits, const int64_t* labels, int B, int C, float grad_scale,
                                  float* sample_loss, float* loss, float* d_logits, nnue_stream_t stream) {
  NNUE_REQUIRE(logits && labels && sample_loss && loss, NNUE_E_ARG, "nnue_cross_entropy: null pointer");
  NNUE_REQUIRE(B > 0 && C > 0, NNUE_E_ARG, "nnue_cross_entropy: B=%d C=%d must be positive", B, C);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cross_entropy_kernel, dim3((B + 3) / 4), dim3(256), 0, s, logits, labels, B, C,
                     grad_scale / (float)B, sample_loss, d_logits);
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, sample_loss, B, loss);
  return nnue_launch_status("nnue_cross_entropy");
}

constexpr int kSteRideBlocks = 1024;  // room for the second-stage workgroups of a deferred STE sum (fps * 28 <= 4096)

extern "C" int64_t nnue_sgd_scratch(int64_t count) {
  (void)count;
  return (kNormBlocks + kSteRideBlocks) * (int64_t)sizeof(float);
}

extern "C" int nnue_sqnorm_partials(const float* grads, int64_t count, float* partial, int nparts, nnue_stream_t stream) {
  NNUE_REQUIRE(grads && partial, NNUE_E_ARG, "nnue_sqnorm_partials: null pointer");
  NNUE_REQUIRE(count > 0 && nparts > 0 && nparts <= 65536, NNUE_E_ARG, "nnue_sqnorm_partials: count=%lld nparts=%d out of range",
               (long long)count, nparts);
  hipLaunchKernelGGL(sqnorm_stage1, dim3(nparts), dim3(256), 0, static_cast<hipStream_t>(stream), grads, count, 1.0f, partial, (int64_t)0,
                     (int64_t)0);
  return nnue_launch_status("nnue_sqnorm_partials");
}

// ---- the flat entry points: nnue_sgd_step, nnue_adam_step, nnue_adam_step_ext and their _clip and _ema siblings ----
namespace {

// The weight clip and the weight average as the caller of a flat entry point gave them (include/nnue_hip.h, "weight clip",
// "weight average"): clip_ranges holds n_ranges pairs (lo, hi) of element indices.  {} is "off", what the plain entry points pass;
// the _clip ones fill the first three fields, the _ema ones all six.
struct FlatOptions {
  float weight_clip = 0.0f;
  const int64_t* clip_ranges = nullptr;
  int n_ranges = 0;
  float* ema = nullptr;
  float ema_omd = 0.0f;
  const float* ema_omd_dev = nullptr;
};

// ... and as the kernels take them.  clip_on: a kernel with the clamp is to be launched (a bound of 0 or no range with an element
// in it: the plain kernel, and fc stays empty -- the Adam kernel's plain arm).  by4: every boundary is a multiple of 4 (what the
// float4 kernel needs).  ema == NULL is "off", whatever the rate says: fe.e is NULL, the kernel's plain arm / instantiation;
// otherwise the rate given by value must lie in (0, 1], and a device scalar replaces it unseen, as lr_dev replaces lr.
struct FlatPacked {
  FlatClip fc;
  FlatEma fe;
  bool clip_on, by4;
};

int flat_options_of(const char* who, const FlatOptions& o, int64_t count, FlatPacked* out) {
  *out = FlatPacked{FlatClip{}, FlatEma{nullptr, 0.0f, nullptr}, false, true};
  NNUE_REQUIRE(o.weight_clip >= 0.0f && o.weight_clip <= 3.4028234e38f, NNUE_E_ARG, "%s: weight_clip = %g must be finite and not negative", who,
               (double)o.weight_clip);
  NNUE_REQUIRE(o.n_ranges >= 0 && o.n_ranges <= 4 && (o.n_ranges == 0 || o.clip_ranges), NNUE_E_ARG,
               "%s: the weight clip takes 0 .. 4 ranges, got %d", who, o.n_ranges);
  FlatClip fc{};
  fc.bound = o.weight_clip;
  for (int r = 0; r < o.n_ranges; ++r) {
    const int64_t lo = o.clip_ranges[2 * r], hi = o.clip_ranges[2 * r + 1];
    NNUE_REQUIRE(lo >= 0 && lo <= hi && hi <= count, NNUE_E_ARG, "%s: clip range %d = [%lld, %lld) does not lie in [0, %lld]", who, r,
                 (long long)lo, (long long)hi, (long long)count);
    fc.lo[r] = lo;
    fc.hi[r] = hi;
    if (lo < hi && o.weight_clip > 0.0f) out->clip_on = true;
    if (lo < hi && (lo % 4 != 0 || hi % 4 != 0)) out->by4 = false;
  }
  if (out->clip_on) out->fc = fc;
  if (o.ema) {
    NNUE_REQUIRE(o.ema_omd_dev || (o.ema_omd > 0.0f && o.ema_omd <= 1.0f), NNUE_E_ARG, "%s: ema_omd = %g must lie in (0, 1]", who,
                 (double)o.ema_omd);
    out->fe = FlatEma{o.ema, o.ema_omd, o.ema_omd_dev};
  }
  return NNUE_OK;
}

// A producer's share of a flat step: its sums of squares `partial` of grads[lo, hi), which the norm launch then skips, and --
// with applied_elsewhere -- the update of that range, for which the apply launch leaves the clip coefficient in coef_out.  The
// first six fields are the entry point's arguments ({}: no producer); ext_range_of checks them, empties the range where there
// are no partials and fills the rest: the hole [skip_lo, skip_hi) of the apply launch and the elements it updates.
struct ExtRange {
  const float* partial;
  int count;
  int64_t lo, hi;
  float* coef_out;
  int applied_elsewhere;
  int64_t skip_lo, skip_hi, live;
};

int ext_range_of(const char* who, int64_t count, ExtRange* x) {
  NNUE_REQUIRE(!x->applied_elsewhere || (x->partial && x->coef_out), NNUE_E_ARG,
               "%s: ext_applied_elsewhere needs the producer's partials and coef_out", who);
  if (x->partial) {
    NNUE_REQUIRE(x->count > 0 && x->count <= 65536 && x->lo >= 0 && x->lo < x->hi && x->hi <= count && x->lo % 4 == 0 &&
                     (x->hi % 4 == 0 || x->hi == count),
                 NNUE_E_ARG, "%s: producer partials need 0 < count <= 65536 and a range [lo, hi) of multiples of 4 inside grads", who);
  } else {
    x->lo = x->hi = 0;
    x->count = 0;
  }
  x->skip_lo = x->applied_elsewhere ? x->lo : 0;
  x->skip_hi = x->applied_elsewhere ? x->hi : 0;
  x->live = count - (x->skip_hi - x->skip_lo);
  return NNUE_OK;
}

// norm workgroups: 16 floats per thread while that still leaves fewer than kNormBlocks (a small model's apply kernel
// then re-derives the norm from a few hundred partials instead of 1024)
int norm_blocks(int64_t count) {
  const int64_t nb = (count + 4095) / 4096;
  return nb < 64 ? 64 : (nb > kNormBlocks ? kNormBlocks : (int)nb);
}
// apply workgroups: up to four elements per thread before the grid is capped
int apply_blocks(int64_t live) {
  const int64_t blocks = (live + 1023) / 1024;
  return blocks < 1 ? 1 : (blocks > 2048 ? 2048 : (int)blocks);
}

int sgd_step_impl(const char* who, float* params, float* grads, float* momentum_buf, int64_t count, float lr, float momentum,
                  float weight_decay, float max_norm, float grad_scale, int first_step, float* norm_out, void* scratch,
                  int64_t scratch_bytes, const float* ste_partial, int ste_chunks, int ste_fps, float* ste_d_thr, float* ste_d_weight,
                  ExtRange x, const float* lr_dev, const FlatOptions& opts, nnue_stream_t stream) {
  NNUE_REQUIRE(params && grads && scratch, NNUE_E_ARG, "%s: null pointer", who);
  NNUE_REQUIRE(count > 0, NNUE_E_ARG, "%s: count must be positive", who);
  NNUE_REQUIRE(momentum == 0.0f || momentum_buf, NNUE_E_ARG, "%s: momentum %g needs a momentum buffer", who, momentum);
  NNUE_REQUIRE(scratch_bytes >= nnue_sgd_scratch(count), NNUE_E_SCRATCH, "%s: scratch %lld < %lld bytes", who,
               (long long)scratch_bytes, (long long)nnue_sgd_scratch(count));
  FlatPacked f;
  if (const int rc = flat_options_of(who, opts, count, &f)) return rc;
  if (const int rc = ext_range_of(who, count, &x)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(scratch);
  const int nb = norm_blocks(count);
  int nparts = nb;
  if (ste_partial) {
    // the deferred sums own the first `skip` elements of grads: [d_thr | d_weight] in either order, nothing else
    NNUE_REQUIRE(ste_d_thr && ste_d_weight && ste_chunks > 0 && ste_fps > 0 && ste_fps * 28 <= 4 * kSteRideBlocks, NNUE_E_ARG,
                 "%s: deferred STE sums need d_thr, d_weight, chunks > 0 and fps * 28 <= %d", who, 4 * kSteRideBlocks);
    const float* lo = ste_d_thr < ste_d_weight ? ste_d_thr : ste_d_weight;
    const float* hi_t = ste_d_thr + ste_fps;
    const float* hi_w = ste_d_weight + (size_t)ste_fps * 27;
    const float* hi = hi_t > hi_w ? hi_t : hi_w;
    const int64_t skip = nnue_round_up(hi - grads, 4);
    NNUE_REQUIRE((!x.partial || x.lo >= skip) && lo == grads && skip <= count && skip <= nnue_round_up(ste_fps, 4) + nnue_round_up((int64_t)ste_fps * 27, 4) + 8, NNUE_E_ARG,
                 "%s: deferred STE outputs must be the first elements of grads", who);
    const int s2_blocks = (ste_fps * 28 + 3) / 4;
    // padding between / after the two outputs is never written by the sums: it enters neither the norm nor is it read
    // before the update multiplies it -- keep it zero (the flat gradient buffer's padding is zero-initialised)
    hipLaunchKernelGGL(sqnorm_stage1_ste, dim3(nb + s2_blocks), dim3(256), 0, s, grads, count, grad_scale, partial, ste_partial,
                       ste_chunks, ste_fps, ste_d_thr, ste_d_weight, s2_blocks, skip, x.lo, x.hi, nb);
    nparts = nb + s2_blocks;
  } else if (max_norm > 0.0f || norm_out || x.coef_out) {
    hipLaunchKernelGGL(sqnorm_stage1, dim3(nb), dim3(256), 0, s, grads, count, grad_scale, partial, x.lo, x.hi);
  }
  float* mom = momentum == 0.0f ? nullptr : momentum_buf;
  static const char* novec = std::getenv("NNUE_SGD_SCALAR");
  const bool vec = !(novec && novec[0] == '1') && x.live <= (16ll << 20) && count % 4 == 0 && x.skip_lo % 4 == 0 && x.skip_hi % 4 == 0 &&
                   nnue_aligned16(params) && nnue_aligned16(grads) && (!mom || nnue_aligned16(mom)) && (!f.clip_on || f.by4) &&
                   (!f.fe.e || nnue_aligned16(f.fe.e));
  const int64_t vb = (x.live / 4 + 511) / 512;  // the float4 kernel: two passes per thread
  const int vec_blocks = vb < 1 ? 1 : (vb > 2048 ? 2048 : (int)vb);
  return with_clip_ema(f.clip_on, f.fe.e != nullptr, [&](auto clip, auto ema) {
    constexpr bool kClip = decltype(clip)::value, kEma = decltype(ema)::value;
    auto go = [&](auto kernel, int grid) {  // (the two forms take the same arguments)
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, params, grads, mom, count, lr, momentum, weight_decay, max_norm, grad_scale,
                         first_step, partial, nparts, norm_out, x.partial, x.count, x.coef_out, x.skip_lo, x.skip_hi, lr_dev, f.fc, f.fe);
    };
    if (vec) go(sgd_apply_vec_kernel<kClip, kEma>, vec_blocks);
    else go(sgd_apply_kernel<kClip, kEma>, apply_blocks(x.live));
    return nnue_launch_status(who);
  });
}

// nnue_adam_step (kExt = false: x is {}, and the norm launch keeps the kNormBlocks workgroups it always had) and nnue_adam_step_ext.
template <bool kExt>
int adam_step_impl(const char* who, float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                   float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale, float* norm_out,
                   void* scratch, int64_t scratch_bytes, ExtRange x, const float* lr_dev, const FlatOptions& opts, nnue_stream_t stream) {
  NNUE_REQUIRE(params && grads && exp_avg && exp_avg_sq && step_counter && scratch, NNUE_E_ARG, "%s: null pointer", who);
  NNUE_REQUIRE(count > 0, NNUE_E_ARG, "%s: count must be positive", who);
  NNUE_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f, NNUE_E_ARG,
               "%s: betas must be in [0,1) and eps > 0", who);
  NNUE_REQUIRE(scratch_bytes >= nnue_sgd_scratch(count), NNUE_E_SCRATCH, "%s: scratch %lld < %lld bytes", who,
               (long long)scratch_bytes, (long long)nnue_sgd_scratch(count));
  if (const int rc = ext_range_of(who, count, &x)) return rc;
  FlatPacked f;
  if (const int rc = flat_options_of(who, opts, count, &f)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(scratch);
  const int nb = kExt ? norm_blocks(count) : kNormBlocks;
  // (always launched: it also advances the step counter)
  hipLaunchKernelGGL(sqnorm_stage1_count<kExt>, dim3(nb), dim3(256), 0, s, grads, count, grad_scale, partial, step_counter, x.lo, x.hi);
  hipLaunchKernelGGL(adam_apply_ext_kernel<kExt>, dim3(apply_blocks(x.live)), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, count, lr,
                     beta1, beta2, eps, weight_decay, max_norm, grad_scale, step_counter, partial, nb, norm_out, x.partial, x.count, x.coef_out,
                     x.skip_lo, x.skip_hi, lr_dev, f.fc, f.fe);
  return nnue_launch_status(who);
}
}  // namespace

extern "C" int nnue_sgd_step(float* params, float* grads, float* momentum_buf, int64_t count, float lr, float momentum,
                             float weight_decay, float max_norm, float grad_scale, int first_step, float* norm_out,
                             void* scratch, int64_t scratch_bytes, const float* ste_partial, int ste_chunks, int ste_fps,
                             float* ste_d_thr, float* ste_d_weight, const float* ext_partial, int ext_count, int64_t ext_lo,
                             int64_t ext_hi, float* coef_out, int ext_applied_elsewhere, const float* lr_dev, nnue_stream_t stream) {
  return sgd_step_impl("nnue_sgd_step", params, grads, momentum_buf, count, lr, momentum, weight_decay, max_norm, grad_scale, first_step, norm_out,
                       scratch, scratch_bytes, ste_partial, ste_chunks, ste_fps, ste_d_thr, ste_d_weight,
                       ExtRange{ext_partial, ext_count, ext_lo, ext_hi, coef_out, ext_applied_elsewhere}, lr_dev, {}, stream);
}

extern "C" int nnue_sgd_step_clip(float* params, float* grads, float* momentum_buf, int64_t count, float lr, float momentum,
                                  float weight_decay, float max_norm, float grad_scale, int first_step, float* norm_out,
                                  void* scratch, int64_t scratch_bytes, const float* ste_partial, int ste_chunks, int ste_fps,
                                  float* ste_d_thr, float* ste_d_weight, const float* ext_partial, int ext_count, int64_t ext_lo,
                                  int64_t ext_hi, float* coef_out, int ext_applied_elsewhere, const float* lr_dev, float weight_clip,
                                  const int64_t* clip_ranges, int n_clip_ranges, nnue_stream_t stream) {
  return sgd_step_impl("nnue_sgd_step_clip", params, grads, momentum_buf, count, lr, momentum, weight_decay, max_norm, grad_scale, first_step,
                       norm_out, scratch, scratch_bytes, ste_partial, ste_chunks, ste_fps, ste_d_thr, ste_d_weight,
                       ExtRange{ext_partial, ext_count, ext_lo, ext_hi, coef_out, ext_applied_elsewhere}, lr_dev,
                       {weight_clip, clip_ranges, n_clip_ranges}, stream);
}

extern "C" int nnue_sgd_step_ema(float* params, float* grads, float* momentum_buf, int64_t count, float lr, float momentum,
                                 float weight_decay, float max_norm, float grad_scale, int first_step, float* norm_out,
                                 void* scratch, int64_t scratch_bytes, const float* ste_partial, int ste_chunks, int ste_fps,
                                 float* ste_d_thr, float* ste_d_weight, const float* ext_partial, int ext_count, int64_t ext_lo,
                                 int64_t ext_hi, float* coef_out, int ext_applied_elsewhere, const float* lr_dev, float weight_clip,
                                 const int64_t* clip_ranges, int n_clip_ranges, float* ema, float ema_omd, const float* ema_omd_dev,
                                 nnue_stream_t stream) {
  return sgd_step_impl("nnue_sgd_step_ema", params, grads, momentum_buf, count, lr, momentum, weight_decay, max_norm, grad_scale, first_step,
                       norm_out, scratch, scratch_bytes, ste_partial, ste_chunks, ste_fps, ste_d_thr, ste_d_weight,
                       ExtRange{ext_partial, ext_count, ext_lo, ext_hi, coef_out, ext_applied_elsewhere}, lr_dev,
                       {weight_clip, clip_ranges, n_clip_ranges, ema, ema_omd, ema_omd_dev}, stream);
}

extern "C" int nnue_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                              float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                              float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev, nnue_stream_t stream) {
  return adam_step_impl<false>("nnue_adam_step", params, grads, exp_avg, exp_avg_sq, step_counter, count, lr, beta1, beta2, eps, weight_decay,
                               max_norm, grad_scale, norm_out, scratch, scratch_bytes, ExtRange{}, lr_dev, {}, stream);
}

extern "C" int nnue_adam_step_clip(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                                   float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                                   float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev, float weight_clip,
                                   const int64_t* clip_ranges, int n_clip_ranges, nnue_stream_t stream) {
  return adam_step_impl<false>("nnue_adam_step_clip", params, grads, exp_avg, exp_avg_sq, step_counter, count, lr, beta1, beta2, eps, weight_decay,
                               max_norm, grad_scale, norm_out, scratch, scratch_bytes, ExtRange{}, lr_dev,
                               {weight_clip, clip_ranges, n_clip_ranges}, stream);
}

extern "C" int nnue_adam_step_ema(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                                  float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev, float weight_clip,
                                  const int64_t* clip_ranges, int n_clip_ranges, float* ema, float ema_omd, const float* ema_omd_dev,
                                  nnue_stream_t stream) {
  return adam_step_impl<false>("nnue_adam_step_ema", params, grads, exp_avg, exp_avg_sq, step_counter, count, lr, beta1, beta2, eps, weight_decay,
                               max_norm, grad_scale, norm_out, scratch, scratch_bytes, ExtRange{}, lr_dev,
                               {weight_clip, clip_ranges, n_clip_ranges, ema, ema_omd, ema_omd_dev}, stream);
}

extern "C" int nnue_adam_step_ext(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                                  float* norm_out, void* scratch, int64_t scratch_bytes, const float* ext_partial, int ext_count,
                                  int64_t ext_lo, int64_t ext_hi, float* coef_out, int ext_applied_elsewhere, const float* lr_dev,
                                  nnue_stream_t stream) {
  return adam_step_impl<true>("nnue_adam_step_ext", params, grads, exp_avg, exp_avg_sq, step_counter, count, lr, beta1, beta2, eps, weight_decay,
                              max_norm, grad_scale, norm_out, scratch, scratch_bytes,
                              ExtRange{ext_partial, ext_count, ext_lo, ext_hi, coef_out, ext_applied_elsewhere}, lr_dev, {}, stream);
}

extern "C" int nnue_adam_step_ext_clip(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                                       float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                                       float* norm_out, void* scratch, int64_t scratch_bytes, const float* ext_partial, int ext_count,
                                       int64_t ext_lo, int64_t ext_hi, float* coef_out, int ext_applied_elsewhere, const float* lr_dev,
                                       float weight_clip, const int64_t* clip_ranges, int n_clip_ranges, nnue_stream_t stream) {
  return adam_step_impl<true>("nnue_adam_step_ext_clip", params, grads, exp_avg, exp_avg_sq, step_counter, count, lr, beta1, beta2, eps,
                              weight_decay, max_norm, grad_scale, norm_out, scratch, scratch_bytes,
                              ExtRange{ext_partial, ext_count, ext_lo, ext_hi, coef_out, ext_applied_elsewhere}, lr_dev,
                              {weight_clip, clip_ranges, n_clip_ranges}, stream);
}

extern "C" int nnue_adam_step_ext_ema(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                                      float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                                      float* norm_out, void* scratch, int64_t scratch_bytes, const float* ext_partial, int ext_count,
                                      int64_t ext_lo, int64_t ext_hi, float* coef_out, int ext_applied_elsewhere, const float* lr_dev,
                                      float weight_clip, const int64_t* clip_ranges, int n_clip_ranges, float* ema, float ema_omd,
                                      const float* ema_omd_dev, nnue_stream_t stream) {
  return adam_step_impl<true>("nnue_adam_step_ext_ema", params, grads, exp_avg, exp_avg_sq, step_counter, count, lr, beta1, beta2, eps,
                              weight_decay, max_norm, grad_scale, norm_out, scratch, scratch_bytes,
                              ExtRange{ext_partial, ext_count, ext_lo, ext_hi, coef_out, ext_applied_elsewhere}, lr_dev,
                              {weight_clip, clip_ranges, n_clip_ranges, ema, ema_omd, ema_omd_dev}, stream);
}

// The stand-alone pass of the weight average (include/nnue_hip.h, "weight average"): ema <- ema_update(ema, params, omd) over
// count elements.  16-byte accesses where both pointers are 16-byte aligned (the < 4 elements behind the last whole float4 go
// one per thread), 4-byte accesses otherwise.
extern "C" int nnue_ema_update(float* ema, const float* params, int64_t count, float omd, const float* ema_omd_dev, nnue_stream_t stream) {
  NNUE_REQUIRE(ema && params, NNUE_E_ARG, "nnue_ema_update: null pointer");
  NNUE_REQUIRE(count > 0, NNUE_E_ARG, "nnue_ema_update: count must be positive");
  NNUE_REQUIRE(ema_omd_dev || (omd > 0.0f && omd <= 1.0f), NNUE_E_ARG, "nnue_ema_update: omd = %g must lie in (0, 1]", (double)omd);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = nnue_aligned16(ema) && nnue_aligned16(params) && count >= 4;
  const int64_t work = vec ? count / 4 + 3 : count;  // threads' worth of work: float4s and up to three tail elements
  int64_t blocks = (work + 1023) / 1024;             // (up to four passes per thread before the grid is capped)
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  if (vec) hipLaunchKernelGGL(ema_update_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, ema, params, count, omd, ema_omd_dev);
  else hipLaunchKernelGGL(ema_update_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, ema, params, count, omd, ema_omd_dev);
  return nnue_launch_status("nnue_ema_update");
}

extern "C" int nnue_confusion_accumulate(const float* logits, const int64_t* labels, int B, int C, uint64_t* confusion,
                                         nnue_stream_t stream) {
  NNUE_REQUIRE(logits && labels && confusion, NNUE_E_ARG, "nnue_confusion_accumulate: null pointer");
  NNUE_REQUIRE(B > 0 && C > 0, NNUE_E_ARG, "nnue_confusion_accumulate: B=%d C=%d must be positive", B, C);
  const int K = C == 1 ? 2 : C;
  hipLaunchKernelGGL(confusion_kernel, dim3((B + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), logits, labels, B, C, K,
                     reinterpret_cast<unsigned long long*>(confusion));
  return nnue_launch_status("nnue_confusion_accumulate");
}

// ---- multi-tensor entry points ----
namespace {

int64_t multi_chunks(int64_t count) { return (count + kMultiChunk - 1) / kMultiChunk; }

// Validates every segment, then packs the tables (kMultiSegs segments per launch) and launches all norm launches before
// all apply launches on `stream`.  m / v / steps / first / a / b / eps may be NULL where the form does not use them.
// Args: MultiArgs, or MultiArgsEma for a list that keeps a weight average (ema[i] / omd[i] per segment; ema[i] NULL: off there).
template <bool kAdam, class Args = MultiArgs>
int multi_step(const char* what, float* const* params, float* const* grads, float* const* m, float* const* v, int32_t* const* steps,
               const int64_t* counts, int n, const float* lr, const float* a, const float* b, const float* eps, const float* wd,
               const int32_t* first, const float* clip, float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes,
               const float* lr_dev, nnue_stream_t stream, float* const* ema = nullptr, const float* omd = nullptr) {
  constexpr int kCap = Args::kCap;
  NNUE_REQUIRE(n > 0, NNUE_E_ARG, "%s: n = %d must be positive", what, n);
  NNUE_REQUIRE(params && grads && counts && lr && a && wd && scratch && (kAdam ? (m && v && steps && b && eps) : first != nullptr),
               NNUE_E_ARG, "%s: null pointer", what);
  int64_t nparts = 0;
  for (int i = 0; i < n; ++i) {
    NNUE_REQUIRE(params[i] && grads[i], NNUE_E_ARG, "%s: null pointer (segment %d)", what, i);
    NNUE_REQUIRE(counts[i] > 0 && counts[i] <= ((int64_t)1 << 40), NNUE_E_ARG, "%s: count %lld of segment %d out of range", what,
                 (long long)counts[i], i);
    if (kAdam) {
      NNUE_REQUIRE(m[i] && v[i] && steps[i], NNUE_E_ARG, "%s: null pointer (segment %d)", what, i);
      NNUE_REQUIRE(a[i] >= 0.f && a[i] < 1.f && b[i] >= 0.f && b[i] < 1.f && eps[i] > 0.f, NNUE_E_ARG,
                   "%s: betas must be in [0,1) and eps > 0 (segment %d)", what, i);
    } else {
      NNUE_REQUIRE(a[i] == 0.0f || (m && m[i]), NNUE_E_ARG, "%s: momentum %g needs a momentum buffer (segment %d)", what, a[i], i);
    }
    NNUE_REQUIRE(!clip || (clip[i] >= 0.0f && clip[i] <= 3.4028234e38f), NNUE_E_ARG, "%s: weight_clip = %g of segment %d must be finite and not negative",
                 what, clip ? (double)clip[i] : 0.0, i);
    if constexpr (Args::kEma)
      NNUE_REQUIRE(!ema[i] || (omd && omd[i] > 0.0f && omd[i] <= 1.0f), NNUE_E_ARG, "%s: ema_omd = %g of segment %d must lie in (0, 1]", what,
                   omd ? (double)omd[i] : 0.0, i);
    nparts += multi_chunks(counts[i]);
  }
  NNUE_REQUIRE(nparts < ((int64_t)1 << 28), NNUE_E_ARG, "%s: %lld elements in all: too many", what, (long long)nparts * kMultiChunk);
  NNUE_REQUIRE(scratch_bytes >= nnue_multi_optim_scratch(counts, n), NNUE_E_SCRATCH, "%s: scratch %lld < %lld bytes", what,
               (long long)scratch_bytes, (long long)nnue_multi_optim_scratch(counts, n));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool need_norm = max_norm > 0.0f || norm_out;
  Args A{};
  A.partial = static_cast<float*>(scratch);
  A.lr_dev = lr_dev;
  A.nparts = (int32_t)nparts;
  A.need_norm = need_norm;
  A.max_norm = max_norm;
  auto pack = [&](int base, int part_base) {  // segments [base, base + kCap) into A
    A.seg_base = base;
    A.part_base = part_base;
    A.n = n - base < kCap ? n - base : kCap;
    A.chunks = A.units = 0;
    for (int i = 0; i < A.n; ++i) {
      const int j = base + i;
      MultiSeg& S = A.seg[i];
      const bool has_m = kAdam || a[j] != 0.0f;
      S = MultiSeg{params[j], grads[j], has_m ? m[j] : nullptr, kAdam ? v[j] : nullptr, kAdam ? steps[j] : nullptr, counts[j],
                   A.chunks, A.units, lr[j], a[j], kAdam ? b[j] : 0.0f, wd[j], kAdam ? eps[j] : 0.0f, kAdam ? 0 : first[j],
                   clip ? clip[j] : 0.0f};
      if constexpr (Args::kEma) {
        A.e[i] = ema[j];
        A.omd[i] = ema[j] ? omd[j] : 0.0f;
      }
      A.chunks += (int32_t)multi_chunks(counts[j]);
      A.units += (int32_t)((counts[j] + kMultiUnit - 1) / kMultiUnit);
    }
  };
  if (need_norm || kAdam) {
    for (int base = 0, part = 0; base < n; base += kCap) {
      pack(base, part);
      part += A.chunks;
      A.norm_out = nullptr;
      hipLaunchKernelGGL(multi_sqnorm_kernel<Args>, dim3(need_norm ? A.chunks : 1), dim3(256), 0, s, A);
    }
  }
  for (int base = 0; base < n; base += kCap) {
    pack(base, 0);
    A.norm_out = base == 0 ? norm_out : nullptr;
    hipLaunchKernelGGL((multi_apply_kernel<kAdam, Args>), dim3(A.units < kMultiApplyBlocks ? A.units : kMultiApplyBlocks), dim3(256), 0, s, A);
  }
  return nnue_launch_status(what);
}

}  // namespace

extern "C" int64_t nnue_multi_optim_scratch(const int64_t* counts, int n) {
  if (!counts || n <= 0) return 0;
  int64_t parts = 0;
  for (int i = 0; i < n; ++i) parts += counts[i] > 0 ? multi_chunks(counts[i]) : 0;
  return nnue_round_up(parts * (int64_t)sizeof(float), 256);
}

extern "C" int nnue_multi_sgd_step(float* const* params, float* const* grads, float* const* momentum_bufs, const int64_t* counts, int n,
                                   const float* lr, const float* momentum, const float* weight_decay, const int32_t* first_step,
                                   float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev,
                                   nnue_stream_t stream) {
  return multi_step<false>("nnue_multi_sgd_step", params, grads, momentum_bufs, nullptr, nullptr, counts, n, lr, momentum, nullptr,
                           nullptr, weight_decay, first_step, nullptr, max_norm, norm_out, scratch, scratch_bytes, lr_dev, stream);
}

extern "C" int nnue_multi_sgd_step_clip(float* const* params, float* const* grads, float* const* momentum_bufs, const int64_t* counts, int n,
                                        const float* lr, const float* momentum, const float* weight_decay, const int32_t* first_step,
                                        const float* weight_clip, float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes,
                                        const float* lr_dev, nnue_stream_t stream) {
  return multi_step<false>("nnue_multi_sgd_step_clip", params, grads, momentum_bufs, nullptr, nullptr, counts, n, lr, momentum, nullptr,
                           nullptr, weight_decay, first_step, weight_clip, max_norm, norm_out, scratch, scratch_bytes, lr_dev, stream);
}

extern "C" int nnue_multi_adam_step(float* const* params, float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                                    int32_t* const* step_counters, const int64_t* counts, int n, const float* lr, const float* beta1,
                                    const float* beta2, const float* eps, const float* weight_decay, float max_norm, float* norm_out,
                                    void* scratch, int64_t scratch_bytes, const float* lr_dev, nnue_stream_t stream) {
  return multi_step<true>("nnue_multi_adam_step", params, grads, exp_avgs, exp_avg_sqs, step_counters, counts, n, lr, beta1, beta2, eps,
                          weight_decay, nullptr, nullptr, max_norm, norm_out, scratch, scratch_bytes, lr_dev, stream);
}

extern "C" int nnue_multi_adam_step_clip(float* const* params, float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                                         int32_t* const* step_counters, const int64_t* counts, int n, const float* lr, const float* beta1,
                                         const float* beta2, const float* eps, const float* weight_decay, const float* weight_clip,
                                         float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev,
                                         nnue_stream_t stream) {
  return multi_step<true>("nnue_multi_adam_step_clip", params, grads, exp_avgs, exp_avg_sqs, step_counters, counts, n, lr, beta1, beta2, eps,
                          weight_decay, nullptr, weight_clip, max_norm, norm_out, scratch, scratch_bytes, lr_dev, stream);
}

// The multi-tensor forms with a weight average per segment (include/nnue_hip.h, "weight average").  A list without one (ema NULL,
// or NULL in every segment) is the _clip form's call, launch for launch.
namespace {
bool multi_has_ema(float* const* ema, int n) {
  for (int i = 0; ema && i < n; ++i)
    if (ema[i]) return true;
  return false;
}
}  // namespace

extern "C" int nnue_multi_sgd_step_ema(float* const* params, float* const* grads, float* const* momentum_bufs, const int64_t* counts, int n,
                                       const float* lr, const float* momentum, const float* weight_decay, const int32_t* first_step,
                                       const float* weight_clip, float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes,
                                       const float* lr_dev, float* const* ema, const float* ema_omd, nnue_stream_t stream) {
  if (n > 0 && multi_has_ema(ema, n))
    return multi_step<false, MultiArgsEma>("nnue_multi_sgd_step_ema", params, grads, momentum_bufs, nullptr, nullptr, counts, n, lr, momentum,
                                           nullptr, nullptr, weight_decay, first_step, weight_clip, max_norm, norm_out, scratch, scratch_bytes,
                                           lr_dev, stream, ema, ema_omd);
  return multi_step<false>("nnue_multi_sgd_step_ema", params, grads, momentum_bufs, nullptr, nullptr, counts, n, lr, momentum, nullptr,
                           nullptr, weight_decay, first_step, weight_clip, max_norm, norm_out, scratch, scratch_bytes, lr_dev, stream);
}

extern "C" int nnue_multi_adam_step_ema(float* const* params, float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                                        int32_t* const* step_counters, const int64_t* counts, int n, const float* lr, const float* beta1,
                                        const float* beta2, const float* eps, const float* weight_decay, const float* weight_clip,
                                        float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev,
                                        float* const* ema, const float* ema_omd, nnue_stream_t stream) {
  if (n > 0 && multi_has_ema(ema, n))
    return multi_step<true, MultiArgsEma>("nnue_multi_adam_step_ema", params, grads, exp_avgs, exp_avg_sqs, step_counters, counts, n, lr, beta1,
                                          beta2, eps, weight_decay, nullptr, weight_clip, max_norm, norm_out, scratch, scratch_bytes, lr_dev,
                                          stream, ema, ema_omd);
  return multi_step<true>("nnue_multi_adam_step_ema", params, grads, exp_avgs, exp_avg_sqs, step_counters, counts, n, lr, beta1, beta2, eps,
                          weight_decay, nullptr, weight_clip, max_norm, norm_out, scratch, scratch_bytes, lr_dev, stream);
}

namespace {

// One wavefront, lane 0 does the work: the step's rate out of a host-made table, the position one further (saturating).
__global__ void __launch_bounds__(64) lr_schedule_step_kernel(const float* __restrict__ table, int n, int32_t* __restrict__ position,
                                                              float* __restrict__ lr_out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int32_t pos = position[0];
  const int32_t i = pos < 0 ? 0 : (pos > n - 1 ? n - 1 : pos);
  lr_out[0] = table[i];
  position[0] = pos < INT32_MAX ? pos + 1 : INT32_MAX;
}

}  // namespace

extern "C" int nnue_lr_schedule_step(const float* table, int64_t n, int32_t* position, float* lr_out, nnue_stream_t stream) {
  NNUE_REQUIRE(table && position && lr_out, NNUE_E_ARG, "nnue_lr_schedule_step: null pointer");
  NNUE_REQUIRE(n > 0 && n <= (int64_t)INT32_MAX, NNUE_E_ARG, "nnue_lr_schedule_step: n=%lld must be in 1..2^31-1", (long long)n);
  hipLaunchKernelGGL(lr_schedule_step_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), table, (int)n, position, lr_out);
  return nnue_launch_status("nnue_lr_schedule_step");
}

// ---------------------------------------------------------------- soft targets (behind everything else: no kernel above moves)
namespace {
// cross_entropy_kernel on soft targets (include/nnue_hip.h, "soft targets"): one wave per sample, one more wave sum.
// GRAD: d_logits is wanted.  (A template also for the code object's sake: instantiations follow every plain kernel and the
// templates used above, so this one stands last.)
template <bool GRAD>
__global__ __launch_bounds__(256) void cross_entropy_soft_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                 SoftTargets st, int B, int C, float scale_over_b,
                                                                 float* __restrict__ sample_loss, float* __restrict__ d_logits) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const float* __restrict__ z = logits + (size_t)b * C;
  float mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, z[c]);
  mx = wave_max(mx);
  float se = 0.f, csum = 0.f;
  for (int c = lane; c < C; c += 64) {
    se += expf(z[c] - mx);
    csum += mx - z[c];
  }
  se = wave_sum(se);
  csum = wave_sum(csum);
  const int64_t y = labels[b], y2 = st.labels_b ? st.labels_b[b] : y;
  const float lam = st.labels_b ? st.lam[b] : 1.0f;
  const bool ok = nnue_soft_counts(y, y2, lam, C);
  if (lane == 0)
    sample_loss[b] = ok ? nnue_ce_soft_sample_loss(mx, z[y], z[y2 >= 0 && y2 < C ? y2 : y], se, csum, lam, st.eps, C) : 0.0f;
  if constexpr (GRAD) {
    const float inv = 1.0f / se;
    for (int c = lane; c < C; c += 64) {
      // the explicit fma is the contraction the compiler picks for cross_entropy_kernel's p - onehot (t = 1, 0: the same bits)
      const float g = fmaf(expf(z[c] - mx), inv, -nnue_soft_target(c == y, c == y2, lam, st.eps, C));
      d_logits[(size_t)b * C + c] = ok ? g * scale_over_b : 0.0f;
    }
  }
}
}  // namespace

extern "C" int nnue_cross_entropy_soft(const float* logits, const int64_t* labels, const int64_t* labels_b, const float* lam, float eps,
                                       int B, int C, float grad_scale, float* sample_loss, float* loss, float* d_logits,
                                       nnue_stream_t stream) {
  NNUE_REQUIRE(logits && labels && sample_loss && loss, NNUE_E_ARG, "nnue_cross_entropy_soft: null pointer");
  NNUE_REQUIRE(B > 0 && C > 0, NNUE_E_ARG, "nnue_cross_entropy_soft: B=%d C=%d must be positive", B, C);
  NNUE_REQUIRE(eps >= 0.0f && eps < 1.0f, NNUE_E_ARG, "nnue_cross_entropy_soft: eps = %g is outside [0, 1)", (double)eps);
  NNUE_REQUIRE(lam || !labels_b, NNUE_E_ARG, "nnue_cross_entropy_soft: labels_b without lam");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const SoftTargets st{labels_b, labels_b ? lam : nullptr, eps};
  if (d_logits)
    hipLaunchKernelGGL(cross_entropy_soft_kernel<true>, dim3((B + 3) / 4), dim3(256), 0, s, logits, labels, st, B, C, grad_scale / (float)B,
                       sample_loss, d_logits);
  else
    hipLaunchKernelGGL(cross_entropy_soft_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, s, logits, labels, st, B, C, grad_scale / (float)B,
                       sample_loss, d_logits);
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, sample_loss, B, loss);
  return nnue_launch_status("nnue_cross_entropy_soft");
}

// ---------------------------------------------------------------- distillation (behind the soft loss: no kernel above moves)
namespace {
// cross_entropy_soft_kernel with the teacher term (include/nnue_hip.h, "soft targets"): one wave per sample, the per-element
// arithmetic of common.h.  GRAD: d_logits is wanted; the loss does not depend on it.
template <bool GRAD>
__global__ __launch_bounds__(256) void cross_entropy_distill_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                    DistillTargets dt, int B, int C, float scale_over_b,
                                                                    float* __restrict__ sample_loss, float* __restrict__ d_logits) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const float* __restrict__ z = logits + (size_t)b * C;
  const float* __restrict__ u = dt.teacher + (size_t)b * C;
  const float T = dt.temperature;
  float mx = -INFINITY, mu = -INFINITY;
  for (int c = lane; c < C; c += 64) {
    mx = fmaxf(mx, z[c]);
    mu = fmaxf(mu, u[c]);
  }
  mx = wave_max(mx);
  mu = wave_max(mu);
  float se = 0.f, csum = 0.f, sU = 0.f, sT = 0.f, ksum = 0.f;
  for (int c = lane; c < C; c += 64) {
    se += expf(z[c] - mx);
    csum += mx - z[c];
    const float eu = nnue_distill_exp(u[c], mu, T);
    sU += eu;
    sT += nnue_distill_exp(z[c], mx, T);
    ksum = nnue_distill_kl_acc(ksum, eu, z[c], mx, u[c], mu);
  }
  se = wave_sum(se);
  csum = wave_sum(csum);
  sU = wave_sum(sU);
  sT = wave_sum(sT);
  ksum = wave_sum(ksum);
  const int64_t y = labels[b], y2 = dt.labels_b ? dt.labels_b[b] : y;
  const float lam = dt.labels_b ? dt.lam[b] : 1.0f;
  const bool ok = nnue_soft_counts(y, y2, lam, C);
  if (lane == 0) {
    const float ls = ok ? nnue_ce_soft_sample_loss(mx, z[y], z[y2 >= 0 && y2 < C ? y2 : y], se, csum, lam, dt.eps, C) : 0.0f;
    sample_loss[b] = ok ? nnue_distill_sample_loss(ls, sT, sU, ksum, dt.alpha, T) : 0.0f;
  }
  if constexpr (GRAD) {
    const float inv = 1.0f / se, inv_sT = 1.0f / sT, inv_sU = 1.0f / sU;
    for (int c = lane; c < C; c += 64) {
      const float soft = fmaf(expf(z[c] - mx), inv, -nnue_soft_target(c == y, c == y2, lam, dt.eps, C));
      const float g = nnue_distill_dlogit(soft, nnue_distill_exp(z[c], mx, T), inv_sT, nnue_distill_exp(u[c], mu, T), inv_sU, dt.alpha, T,
                                          scale_over_b);
      d_logits[(size_t)b * C + c] = ok ? g : 0.0f;
    }
  }
}
}  // namespace

extern "C" int nnue_cross_entropy_distill(const float* logits, const int64_t* labels, const int64_t* labels_b, const float* lam, float eps,
                                          int B, int C, float grad_scale, float* sample_loss, float* loss, float* d_logits,
                                          const float* teacher, float alpha, float temperature, nnue_stream_t stream) {
  NNUE_REQUIRE(alpha >= 0.0f && alpha <= 1.0f, NNUE_E_ARG, "nnue_cross_entropy_distill: alpha = %g is outside [0, 1]", (double)alpha);
  NNUE_REQUIRE(temperature > 0.0f && temperature < INFINITY, NNUE_E_ARG,
               "nnue_cross_entropy_distill: temperature = %g must be finite and positive", (double)temperature);
  NNUE_REQUIRE(teacher || alpha == 0.0f, NNUE_E_ARG, "nnue_cross_entropy_distill: alpha > 0 without teacher logits");
  // alpha == 0 is the soft call: the same launches, the teacher is not read
  if (alpha == 0.0f) return nnue_cross_entropy_soft(logits, labels, labels_b, lam, eps, B, C, grad_scale, sample_loss, loss, d_logits, stream);
  NNUE_REQUIRE(logits && labels && sample_loss && loss, NNUE_E_ARG, "nnue_cross_entropy_distill: null pointer");
  NNUE_REQUIRE(B > 0 && C > 0, NNUE_E_ARG, "nnue_cross_entropy_distill: B=%d C=%d must be positive", B, C);
  NNUE_REQUIRE(eps >= 0.0f && eps < 1.0f, NNUE_E_ARG, "nnue_cross_entropy_distill: eps = %g is outside [0, 1)", (double)eps);
  NNUE_REQUIRE(lam || !labels_b, NNUE_E_ARG, "nnue_cross_entropy_distill: labels_b without lam");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DistillTargets dt;
  dt.labels_b = labels_b, dt.lam = labels_b ? lam : nullptr, dt.eps = eps;
  dt.teacher = teacher, dt.alpha = alpha, dt.temperature = temperature;
  if (d_logits)
    hipLaunchKernelGGL(cross_entropy_distill_kernel<true>, dim3((B + 3) / 4), dim3(256), 0, s, logits, labels, dt, B, C, grad_scale / (float)B,
                       sample_loss, d_logits);
  else
    hipLaunchKernelGGL(cross_entropy_distill_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, s, logits, labels, dt, B, C,
                       grad_scale / (float)B, sample_loss, d_logits);
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, sample_loss, B, loss);
  return nnue_launch_status("nnue_cross_entropy_distill");
}
