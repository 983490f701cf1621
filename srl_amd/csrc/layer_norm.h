// The row arithmetic of LayerNorm (torch.nn.LayerNorm over the last dimension, eps = 1e-5), once.  No kernels, no layout, no
// reductions, no loads or stores: every caller brings a row's elements in its own way and sums across lanes in its own way (a
// wavefront butterfly, an LPR-wide one, sum16, the accumulator layout's __shfl_xor(.., 32), a workgroup through LDS, one thread
// per row); only the per-element and per-row expressions are here.
//
//   forward    mean = sum x / D,  q = sum (x - mean)^2,  rstd = rsqrt(q / D + eps)
//              xhat = (x - mean) * rstd,  y = fma(xhat, gamma, beta)
//   backward   g = dy * gamma,  s1 = sum g,  s2 = sum g * xhat,  m1 = s1 / D,  m2 = s2 / D
//              dx = rstd * (g - m1 - xhat * m2)       (times the derivative of the activation in front, by the caller)
//              dgamma += dy * xhat,  dbeta += dy      (summed over the rows)
//
// Every caller evaluates exactly these expressions, in this operand order and grouping; the products that feed a sum
// (g * xhat, dy * xhat) enter it through one explicit fused multiply-add, whatever the compiler's contraction setting.  The whole-observation statistics (the observation
// LayerNorm in front of the first convolution) come from exact or float64 sums and take the float64 form ln_rstd_f64.
//
// Included by nn_ops.hip, ln_heads.hip, ln_heads_wide.hip, entity_attn.hip, obs_ring.hip and mlp_small.hip (and through it by mlp_mfma.h and
// mlp_sig.h).
#pragma once
#include "srl_common.h"

namespace {

constexpr float kLnEps = 1e-5f;  // nn.LayerNorm default, used everywhere in the reference

// q: the row's sum of (x - mean)^2
__device__ __forceinline__ float ln_rstd(float centered_sumsq, int D) { return rsqrtf(centered_sumsq / (float)D + kLnEps); }
// var: the (biased) variance itself, in float64
__device__ __forceinline__ float ln_rstd_f64(double var) { return (float)(1.0 / sqrt(var + (double)kLnEps)); }

__device__ __forceinline__ float ln_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float ln_affine(float xhat, float gamma, float beta) { return fmaf(xhat, gamma, beta); }

// One element's terms of the backward sums: the row's s1, s2 (whoever forms dx) and the columns' dgamma, dbeta (whoever owns the
// column).  A caller that keeps the two in different threads takes the half it needs; the row half returns g for a caller that
// holds it in a register until dx.
__device__ __forceinline__ float ln_bwd_row_sums(float dy, float gamma, float xhat, float& s1, float& s2) {
  const float g = dy * gamma;
  s1 += g;
  s2 = fmaf(g, xhat, s2);
  return g;
}
__device__ __forceinline__ void ln_bwd_param_sums(float dy, float xhat, float& pg, float& pb) {
  pg = fmaf(dy, xhat, pg);
  pb += dy;
}
__device__ __forceinline__ float ln_bwd_accumulate(float dy, float gamma, float xhat, float& s1, float& s2, float& pg, float& pb) {
  ln_bwd_param_sums(dy, xhat, pg, pb);
  return ln_bwd_row_sums(dy, gamma, xhat, s1, s2);
}

// m1 = s1 / D, m2 = s2 / D of the whole row; from g = dy * gamma as the sums returned it, or from its factors
__device__ __forceinline__ float ln_dx(float g, float xhat, float m1, float m2, float rstd) { return rstd * (g - m1 - xhat * m2); }
__device__ __forceinline__ float ln_dx(float dy, float gamma, float xhat, float m1, float m2, float rstd) {
  return ln_dx(dy * gamma, xhat, m1, m2, rstd);
}

}  // namespace
