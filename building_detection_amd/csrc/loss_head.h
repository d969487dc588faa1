// What the four units of the C-class loss head share: multiclass.hip (sg_lossn_*), region_loss.hip, hard_mining.hip and
// lovasz.hip.  Each piece exists once, here; the kernels stay in their own files, and so do their row loops ("load p, y, w of
// a row, add up loss_row_term"): they are written against the scalar forms below.  As helpers that take the row's arrays they
// made the compiler merge a row's dword loads into multi-dword loads at 4-byte alignment and pack two classes' products (which
// un-fuses the sum's multiply-add unless it is spelled fmaf): sg_lossn_* + 19 %, sg_loss_mined_* + 24 %, sg_loss_lovasz_* + 5 %
// at C = 5 and 4 M rows.
//   ClassVec, SG_CLASS_FOR, SG_CLASS_DISPATCH   a per-class vector, the predicated class loop, the nine instantiations
//   loss_coeff, loss_row_term, loss_row_grad    the per-row forms of the three pointwise losses
//       row sum  r = sum_c a_c f(p_c) log(p_c + eps),   f = 1 (cross-entropy) or (1 - p)^2 (the focal kinds);   l = -r
//       dr/dp_c = a_c g(p_c),   g = 1 / (p + eps)  or  -2 (1 - p) log(p + eps) + (1 - p)^2 / (p + eps)
//   row_first_max, clamp_bits                   a row's truth class (first maximum), a key's clamp to [0, 1] on the bits
//   block_sum_256, block_sum_double, put_loss_terms      the workgroup sums (their order of additions is part of the results'
//                                                        bits) and the three loss scalars {L, L_point, L_other}
//   loss_head_ok, loss_weights_ok, class_vec, nonneg, loss_bwd_blocks   the host checks of a descriptor's head fields
#pragma once
#include <float.h>
#include "sg_common.h"

constexpr float SG_LOSS_EPS = 1e-7f;  // tf.keras.backend.epsilon()

struct ClassVec {
  float v[SG_MAX_CLASSES];
};

// inside a kernel template <int CM, bool EX>: CM is the unrolled trip count; EX says that C == CM is known at compile time
#define SG_CLASS_FOR(c) _Pragma("unroll") for (int c = 0; c < CM; ++c) if (EX || c < C)

// LAUNCH(CM, EX) for the instantiation that serves C: the exact forms for C = 2 ... 8, the bounded ones for C <= 16 and C <= 32
#define SG_CLASS_DISPATCH(C, LAUNCH) \
  do {                               \
    switch (C) {                     \
      case 2: LAUNCH(2, true); break; \
      case 3: LAUNCH(3, true); break; \
      case 4: LAUNCH(4, true); break; \
      case 5: LAUNCH(5, true); break; \
      case 6: LAUNCH(6, true); break; \
      case 7: LAUNCH(7, true); break; \
      case 8: LAUNCH(8, true); break; \
      default:                       \
        if ((C) <= 16) { LAUNCH(16, false); } else { LAUNCH(32, false); } \
    }                                \
  } while (0)

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

// first maximum while scanning upwards (strict >): ties go to the lowest index, as tf.argmax does
template <int CM, bool EX>
__device__ __forceinline__ int row_first_max(const float (&v)[CM], int C) {
  float best = v[0];
  int q = 0;
  SG_CLASS_FOR(c) if (c > 0 && v[c] > best) {
    best = v[c];
    q = c;
  }
  return q;
}

// NaN / negative / -0 -> +0, above 1 -> 1.  On the bits, so that no floating-point mode touches a denormal: a set sign bit or
// a NaN lies above +inf's pattern
__device__ __forceinline__ uint32_t clamp_bits(float p) {
  const uint32_t b = __float_as_uint(p);
  return b > 0x7f800000u ? 0u : (b < 0x3f800000u ? b : 0x3f800000u);
}

// the workgroup's (256 threads) sum of v: a wave's 64 by xor-shuffles, then the four waves in wave order.  Valid in thread 0
template <typename T>
__device__ __forceinline__ T block_sum_256(T v, T* sm) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  T t = 0;
  if (threadIdx.x == 0) t = sm[0] + sm[1] + sm[2] + sm[3];
  return t;
}

// the same in double, every thread adding the four wave sums
__device__ __forceinline__ double block_sum_double(double v, double* sm) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// out = {L, L_point, L_other}, L = point_weight * lp + other_weight * lo; kind < 0: no pointwise term
__device__ __forceinline__ void put_loss_terms(float* __restrict__ out, int kind, float point_weight, double lp, float other_weight,
                                               double lo) {
  out[0] = (float)((kind >= 0 ? (double)point_weight * lp : 0.0) + (double)other_weight * lo);
  out[1] = (float)lp;
  out[2] = (float)lo;
}

inline bool nonneg(float v) { return v >= 0.f && v <= FLT_MAX; }  // finite and >= 0 (a NaN fails both)

// C, y_cols, the pointwise kind (-1 = none where `none_ok`) and, where given, the finite class weights of a focal kind.
// kind_name, alpha_name: what the caller's interface calls the two.  0, or SG_EINVAL with the error text set
inline int loss_head_ok(const char* who, int C, int y_cols, int kind, bool none_ok, const char* kind_name, const float* alpha,
                        const char* alpha_name) {
  SG_CHECK_ARG(C >= 2 && C <= SG_MAX_CLASSES, "%s: C = %d outside [2, %d]", who, C, SG_MAX_CLASSES);
  SG_CHECK_ARG(y_cols == C || y_cols == 2 * C, "%s: y_true has %d columns, not C = %d or 2C", who, y_cols, C);
  SG_CHECK_ARG(kind >= (none_ok ? -1 : SG_LOSS_CE2) && kind <= SG_LOSS_EDGE_FOCAL, "%s: unknown %s %d", who, kind_name, kind);
  SG_CHECK_ARG(kind != SG_LOSS_EDGE_FOCAL || y_cols == 2 * C, "%s: edge_focal_loss needs y_true[..., 2C]", who);
  if (alpha && kind > SG_LOSS_CE2)
    for (int c = 0; c < C; ++c)
      SG_CHECK_ARG(alpha[c] >= -FLT_MAX && alpha[c] <= FLT_MAX, "%s: %s[%d] is not finite", who, alpha_name, c);
  return 0;
}

// the weights of a pointwise term and of the term `other_name` beside it: finite, >= 0 and not both 0
inline int loss_weights_ok(const char* who, int kind, float point_weight, float other_weight, const char* other_name) {
  SG_CHECK_ARG(nonneg(point_weight) && nonneg(other_weight), "%s: point_weight = %g, %s = %g must be finite and >= 0", who,
               point_weight, other_name, other_weight);
  if (kind < 0) SG_CHECK_ARG(other_weight > 0.f, "%s: %s = 0 without a pointwise term", who, other_name);
  else SG_CHECK_ARG(point_weight > 0.f || other_weight > 0.f, "%s: point_weight and %s are both 0", who, other_name);
  return 0;
}

// the class weights a kernel takes by value: alpha[:C] for the focal kinds, ones otherwise and past C
inline ClassVec class_vec(int kind, int C, const float* alpha) {
  ClassVec al;
  for (int c = 0; c < SG_MAX_CLASSES; ++c) al.v[c] = (kind > SG_LOSS_CE2 && c < C) ? alpha[c] : 1.f;
  return al;
}

// workgroups of a backward pass over `rows` rows
inline unsigned loss_bwd_blocks(int64_t rows) { return ew_blocks(rows, 8192); }
