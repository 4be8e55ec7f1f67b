// The per-element arithmetic of the optimizers, one text for every kernel that applies an update: the flat and the
// multi-tensor kernels (optim_kernels.hip), the weight-gradient product's read-modify-write epilogues and the fused
// update + next-forward pass (ftm_kernels.hip, update_forward.h).
#pragma once

// The per-element arithmetic of clip_grad_norm_ + SGD (train.py:363-366, :457-464), shared by the flat and the multi-tensor
// kernels: g <- gs*g + wd*w; m <- first ? g : momentum*m + g (has_m: momentum != 0); returns w - lr*m.
__device__ __forceinline__ float sgd_update(float w, float g, float m_old, float& m_new, float gs, float lr, float momentum,
                                            float wd, bool has_m, bool first) {
  float gi = fmaf(wd, w, g * gs);
  if (has_m) gi = first ? gi : fmaf(momentum, m_old, gi);
  m_new = gi;
  return w - lr * gi;
}

// ... and of clip_grad_norm_ + Adam (train.py:363-366, :465-470): L2 weight decay folded into the gradient, the moments
// updated in place, the bias corrections of step t precomputed by adam_bias_correction.
struct AdamBias {
  float step_size, inv_sqrt_bc2;
};
__device__ __forceinline__ AdamBias adam_bias_correction(float lr, float beta1, float beta2, int t) {
  const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
  return {(float)((double)lr / bc1), (float)(1.0 / sqrt(bc2))};
}
__device__ __forceinline__ float adam_update(float w, float g, float& m, float& v, float gs, AdamBias bc, float beta1, float beta2,
                                             float eps, float wd) {
  const float gi = fmaf(wd, w, g * gs);
  m = beta1 * m + (1.0f - beta1) * gi;
  v = beta2 * v + (1.0f - beta2) * gi * gi;
  return w - bc.step_size * (m / (sqrtf(v) * bc.inv_sqrt_bc2 + eps));
}

// The post-update weight clip (nnue.py:528-539, _clip_weights; include/nnue_hip.h, "weight clip"): what torch.clamp_(-c, c)
// leaves, bit for bit -- a NaN stays a NaN and -0.0 stays -0.0, which fminf / fmaxf would not keep.  Every kernel that applies
// an update to a clipped tensor calls it on the value sgd_update / adam_update / adam_update_fused returned, before the store;
// the optimizer's state is formed from the un-clamped arithmetic and never clamped.
__device__ __forceinline__ float clip_weight(float w, float c) { return w > c ? c : (w < -c ? -c : w); }

// The moving average of the weights (include/nnue_hip.h, "weight average"): e <- e + omd (w_new - e), one rounding of the
// difference and one of the fused multiply-add, omd = float32(1 - float64(decay)).  w_new is the value the launch stores -- after
// the update and after clip_weight where the clip is on -- so a convex combination of clamped weights stays inside the bound.
// Every kernel that applies an update calls it last; nothing of a step reads the average, and the optimizer's state never
// sees it.  Nothing here is left to the compiler's contraction: the stand-alone pass and every fused form give the same bits.
__device__ __forceinline__ float ema_update(float e, float w_new, float omd) { return fmaf(omd, w_new - e, e); }

// adam_update with every fused multiply-add written out -- the form -ffp-contract=on gives that text (the multiply on the
// left of a sum is the fused one).  Under the build's default contraction the compiler fuses a * b + c * d wherever the
// caller's context lets it (measured: v = beta2 v + (1 - beta2) g g came out as one fma in the product's epilogue and as
// mul, mul, add in the fused update + forward pass, one ulp apart), so kernels whose results must agree BIT FOR BIT --
// those two -- take this one: nothing in it is left for the contraction to decide.  Within a rounding per term of adam_update.
__device__ __forceinline__ float adam_update_fused(float w, float g, float& m, float& v, float gs, AdamBias bc, float beta1, float beta2,
                                                   float eps, float wd) {
  const float gi = fmaf(wd, w, g * gs);
  m = fmaf(beta1, m, (1.0f - beta1) * gi);
  v = fmaf(beta2, v, ((1.0f - beta2) * gi) * gi);
  return fmaf(-bc.step_size, m / fmaf(sqrtf(v), bc.inv_sqrt_bc2, eps), w);
}
