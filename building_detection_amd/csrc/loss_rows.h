// The per-row forms of the three pointwise losses on the C-class head, shared by multiclass.hip (sg_lossn_*) and
// hard_mining.hip (sg_loss_mined_*): one class's coefficient a_c, its term of the row sum and its derivative factor.
//   row sum  r = sum_c a_c f(p_c) log(p_c + eps),   f = 1 (cross-entropy) or (1 - p)^2 (the focal kinds);   l = -r
//   dr/dp_c = a_c g(p_c),   g = 1 / (p + eps)  or  -2 (1 - p) log(p + eps) + (1 - p)^2 / (p + eps)
#pragma once
#include "sg_common.h"

constexpr float SG_LOSS_EPS = 1e-7f;  // tf.keras.backend.epsilon()

// a_c of the three losses; w = y_true[:, C:2C] (edge focal only, which the entry points take with y_cols == 2C alone)
__device__ __forceinline__ float loss_coeff(int kind, float alpha, float y, float w) {
  if (kind == SG_LOSS_CE2) return y;
  if (kind == SG_LOSS_FOCAL) return alpha * y;
  return alpha * w * y;
}

__device__ __forceinline__ float loss_row_term(int kind, float a, float p) {
  const float f = kind == SG_LOSS_CE2 ? 1.f : (1.f - p) * (1.f - p);
  return a * f * logf(p + SG_LOSS_EPS);
}

__device__ __forceinline__ float loss_row_grad(int kind, float p) {
  if (kind == SG_LOSS_CE2) return 1.f / (p + SG_LOSS_EPS);
  const float q = 1.f - p;
  return -2.f * q * logf(p + SG_LOSS_EPS) + q * q / (p + SG_LOSS_EPS);
}
