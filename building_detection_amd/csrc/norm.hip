// BatchNormalization (Keras defaults) for NHWC [rows][C]: training forward/backward and inference.
// HBM-bound: forward = one statistics pass (read x) + one apply pass (read x, write y); backward = one
// reduction pass (read x, dy[, y]) + one apply pass.  Statistics use a per-channel pivot (the first row) so
// the single-pass variance  E[(x-K)^2] - E[x-K]^2  does not cancel, and are combined in fp64.
#include "sg_reduce.h"

namespace {

// The per-element expressions, each written once: what makes mask modes 1 and 2, and the flat and column forms, bit-identical
__device__ __forceinline__ float bn_affine(float x, float mean, float invstd, float gamma, float beta) {
  return fmaf((x - mean) * invstd, gamma, beta);
}
// MODE: 0 = no fused ReLU, 1 = ReLU mask read from y, 2 = ReLU mask recomputed from x (gamma, beta given)
template <int MODE, int V>
__device__ __forceinline__ void bn_mask(float (&g)[V], const float (&x)[V], const float (&y)[V], const float (&mean)[V],
                                        const float (&invstd)[V], const float (&gamma)[V], const float (&beta)[V]) {
  if constexpr (MODE == 2) {
#pragma unroll
    for (int i = 0; i < V; ++i) g[i] = bn_affine(x[i], mean[i], invstd[i], gamma[i], beta[i]) > 0.f ? g[i] : 0.f;
  } else if constexpr (MODE == 1) {
#pragma unroll
    for (int i = 0; i < V; ++i) g[i] = y[i] > 0.f ? g[i] : 0.f;
  }
}
__device__ __forceinline__ float bn_dx(float x, float g, float mean, float invstd, float gamma, float dgamma, float dbeta, float inv_n) {
  const float xh = (x - mean) * invstd;
  return gamma * invstd * (g - dbeta * inv_n - xh * dgamma * inv_n);
}

template <typename T>
struct BnStatsOp {
  static constexpr int NOUT = 2;
  const T* __restrict__ x;
  int C;
  int64_t rows;
  float* moving_mean;
  float* moving_var;
  float* save_mean;
  float* save_invstd;
  float momentum, eps;
  int unbiased;

  template <int V>
  __device__ __forceinline__ void accum(int, int64_t r, int c, float (&acc)[2][V]) const {
    float k[V], v[V];
    ldv<V>(x + c, k);  // pivot = row 0
    ldv<V>(x + r * C + c, v);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float d = v[i] - k[i];
      acc[0][i] += d;
      acc[1][i] = fmaf(d, d, acc[1][i]);
    }
  }
  __device__ __forceinline__ void finalize(int, int c, const double (&s)[2]) const {
    const double n = (double)rows;
    const double m1 = s[0] / n;
    const double mean = (double)ld1<T>(x + c) + m1;
    double var = s[1] / n - m1 * m1;
    if (var < 0.0) var = 0.0;
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    const double var_u = (unbiased && rows > 1) ? var * (n / (n - 1.0)) : var;
    moving_mean[c] = (float)((double)moving_mean[c] * momentum + mean * (1.0 - (double)momentum));
    moving_var[c] = (float)((double)moving_var[c] * momentum + var_u * (1.0 - (double)momentum));
  }
};

// MODE as in bn_mask.  Compile-time, and the per-channel parameters are loaded once per thread (BnCtx): the row loop is two
// loads (three in mode 1) and arithmetic, four rows in flight.
template <int V>
struct BnCtx {
  float mv[V], iv[V], gm[V], bt[V];
};

template <typename T, int MODE>
struct BnBwdOp {
  static constexpr int NOUT = 2;  // sum dy, sum dy * xhat
  const T* __restrict__ x;
  const T* __restrict__ y;
  const T* __restrict__ dy;
  const float* __restrict__ mean;
  const float* __restrict__ invstd;
  const float* __restrict__ gamma;  // with beta: the ReLU mask is recomputed from x instead of read from y
  const float* __restrict__ beta;
  float* dgamma;
  float* dbeta;
  int C;

  template <int V>
  __device__ __forceinline__ BnCtx<V> begin(int, int c) const {
    BnCtx<V> k;
    ldv<V>(mean + c, k.mv);
    ldv<V>(invstd + c, k.iv);
    if constexpr (MODE == 2) {
      ldv<V>(gamma + c, k.gm);
      ldv<V>(beta + c, k.bt);
    }
    return k;
  }
  template <int V>
  __device__ __forceinline__ void accum(int, int64_t r, int c, float (&acc)[2][V], const BnCtx<V>& k) const {
    float xv[V], gv[V], yv[V];
    ldv<V>(x + r * C + c, xv);
    ldv<V>(dy + r * C + c, gv);
    if constexpr (MODE == 1) ldv<V>(y + r * C + c, yv);
    bn_mask<MODE>(gv, xv, yv, k.mv, k.iv, k.gm, k.bt);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      acc[0][i] += gv[i];
      acc[1][i] = fmaf(gv[i], (xv[i] - k.mv[i]) * k.iv[i], acc[1][i]);
    }
  }
  __device__ __forceinline__ void finalize(int, int c, const double (&s)[2]) const {
    dbeta[c] = (float)s[0];
    dgamma[c] = (float)s[1];
  }
};

// ---- dy that is the input gradient of a thin 1x1 convolution (Cout = CO <= 4: the softmax head, the sSE gate), never written out ----
// dy[r][c] = sum_o g[r][o] * w[c][o] is evaluated where the backward consumes it, with thin_dgrad_kernel's own expression
// (csrc/conv_thin.hip), so the sums and dx have the bits of thin dgrad + sg_bn_train_bwd without the C-wide tensor.  fp32 storage.
// The value is the result of explicit fmaf calls, which the compiler does not contract into their uses: it reaches them as the rounded
// fp32 the other path stores.  (No asm fence: inline asm is convergent, and the reducer's row loop is then not unrolled.)
template <int V, int CO>
__device__ __forceinline__ void thin_w(const float* __restrict__ w, int c, float (&wv)[V][CO]) {
#pragma unroll
  for (int k = 0; k < V; ++k)
#pragma unroll
    for (int o = 0; o < CO; ++o) wv[k][o] = w[(c + k) * CO + o];
}
template <int V, int CO>
__device__ __forceinline__ void thin_dy(const float* __restrict__ g, const float (&wv)[V][CO], float (&dy)[V]) {
  float gv[CO];
#pragma unroll
  for (int o = 0; o < CO; ++o) gv[o] = g[o];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    float a = 0.f;
#pragma unroll
    for (int o = 0; o < CO; ++o) a = fmaf(gv[o], wv[k][o], a);
    dy[k] = a;
  }
}

template <int V, int CO>
struct BnThinCtx {
  BnCtx<V> k;
  float wv[V][CO];
};

// BnBwdOp on that source (MODE 0 or 2: the mask is recomputed from x)
template <int MODE, int CO>
struct BnBwdThinOp {
  static constexpr int NOUT = 2;
  const float* __restrict__ x;
  const float* __restrict__ g;   // [rows][y_ld], CO live columns
  const float* __restrict__ w;   // [C][CO]
  const float* __restrict__ mean;
  const float* __restrict__ invstd;
  const float* __restrict__ gamma;
  const float* __restrict__ beta;
  float* dgamma;
  float* dbeta;
  int C, y_ld;

  template <int V>
  __device__ __forceinline__ BnThinCtx<V, CO> begin(int, int c) const {
    BnThinCtx<V, CO> q;
    ldv<V>(mean + c, q.k.mv);
    ldv<V>(invstd + c, q.k.iv);
    if constexpr (MODE == 2) {
      ldv<V>(gamma + c, q.k.gm);
      ldv<V>(beta + c, q.k.bt);
    }
    thin_w<V, CO>(w, c, q.wv);
    return q;
  }
  template <int V>
  __device__ __forceinline__ void accum(int, int64_t r, int c, float (&acc)[2][V], const BnThinCtx<V, CO>& q) const {
    float xv[V], gv[V], yv[V];
    ldv<V>(x + r * C + c, xv);
    thin_dy<V, CO>(g + r * y_ld, q.wv, gv);
    bn_mask<MODE>(gv, xv, yv, q.k.mv, q.k.iv, q.k.gm, q.k.bt);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      acc[0][i] += gv[i];
      acc[1][i] = fmaf(gv[i], (xv[i] - q.k.mv[i]) * q.k.iv[i], acc[1][i]);
    }
  }
  __device__ __forceinline__ void finalize(int, int c, const double (&s)[2]) const {
    dbeta[c] = (float)s[0];
    dgamma[c] = (float)s[1];
  }
};

template <int V, typename T>
__global__ void bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                const float* __restrict__ invstd, const float* __restrict__ gamma,
                                const float* __restrict__ beta, T* __restrict__ y, int64_t rows, int C, int relu,
                                float eps, int infer, FastDiv fd_cv) {
  const uint32_t cv = C / V;
  const uint32_t total = (uint32_t)(rows * cv);
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = fd_div(i, fd_cv);
    const int c = (int)(i - (uint32_t)r * cv) * V;
    float xv[V], mv[V], iv[V], gv[V], bv[V], o[V];
    ldv<V>(x + r * C + c, xv);
    ldv<V>(mean + c, mv);
    ldv<V>(invstd + c, iv);  // inference: this is the moving variance
    ldv<V>(gamma + c, gv);
    ldv<V>(beta + c, bv);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float is = infer ? rsqrtf(iv[k] + eps) : iv[k];
      float t = bn_affine(xv[k], mv[k], is, gv[k], bv[k]);
      if (relu) t = fmaxf(t, 0.f);
      o[k] = t;
    }
    stv<V>(y + r * C + c, o);
  }
}

// MODE as in BnBwdOp (compile-time: no load behind a branch)
template <int V, typename T, int MODE>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ y,
                                    const T* __restrict__ dy, const float* __restrict__ mean,
                                    const float* __restrict__ invstd, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, const float* __restrict__ dgamma,
                                    const float* __restrict__ dbeta, T* __restrict__ dx, int64_t rows, int C,
                                    FastDiv fd_cv) {
  const uint32_t cv = C / V;
  const uint32_t total = (uint32_t)(rows * cv);
  const uint32_t stride = gridDim.x * blockDim.x;
  const float inv_n = 1.0f / (float)rows;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = fd_div(i, fd_cv);
    const int c = (int)(i - (uint32_t)r * cv) * V;
    float xv[V], gv[V], mv[V], iv[V], gam[V], dg[V], db[V], o[V];
    ldv<V>(x + r * C + c, xv);
    ldv<V>(dy + r * C + c, gv);
    ldv<V>(mean + c, mv);
    ldv<V>(invstd + c, iv);
    ldv<V>(gamma + c, gam);
    ldv<V>(dgamma + c, dg);
    ldv<V>(dbeta + c, db);
    // bn_mask and bn_dx written out: through the helpers this kernel alone (V = 4, 8) comes out in another instruction order
    if constexpr (MODE == 2) {
      float bt[V];
      ldv<V>(beta + c, bt);
#pragma unroll
      for (int k = 0; k < V; ++k) gv[k] = bn_affine(xv[k], mv[k], iv[k], gam[k], bt[k]) > 0.f ? gv[k] : 0.f;
    } else if constexpr (MODE == 1) {
      float yv[V];
      ldv<V>(y + r * C + c, yv);
#pragma unroll
      for (int k = 0; k < V; ++k) gv[k] = yv[k] > 0.f ? gv[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float xh = (xv[k] - mv[k]) * iv[k];
      o[k] = gam[k] * iv[k] * (gv[k] - db[k] * inv_n - xh * dg[k] * inv_n);
    }
    stv<V>(dx + r * C + c, o);
  }
}

// Column-block forms of the two kernels above (round 3): a thread keeps ONE chunk of V channels and walks down the rows, so
// the per-channel parameters are loaded once per thread instead of once per element.  With bf16 storage a 16-byte access is
// 8 channels and the flat kernels issued 10 (apply) / 14 (backward) 16-byte parameter loads per 16 bytes of tensor: 20.8 /
// 29.8 us for the 24 MB tensors of the middle flow against a copy's 11.8 us (profiles/r03_bw_bench.txt) - bound by the
// load issue, not by bytes.  The flat index space is kept (a wave touches 1 KB of consecutive addresses: 16 chunk lanes x 16
// row lanes with 256-byte runs measured 3.4 instead of 4.6 TB/s in fp32), but the number of threads is a multiple of the
// chunks per row, so a thread's grid stride is a whole number of rows and its channel chunk never changes.  Four (backward:
// two) rows in flight per thread, taken from consecutive periods so that the workgroups in flight sweep one window of the tensor.  Same per-element expressions, so results are bit-identical to the flat kernels.
template <int V, typename T>
__global__ __launch_bounds__(256) void bn_apply_cols_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, T* __restrict__ y, int64_t rows,
                                                            int C, int relu, float eps, int infer, int prow, FastDiv fd_cv) {
  // blockIdx.x: block within a period of prow whole rows; blockIdx.y: group of four consecutive periods
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, cv = (uint32_t)(C / V);
  const uint32_t r0 = fd_div(i0, fd_cv);
  const int c = (int)(i0 - r0 * cv) * V;
  float mv[V], is[V], gv[V], bv[V];
  ldv<V>(mean + c, mv);
  ldv<V>(invstd + c, is);  // inference: this is the moving variance
  ldv<V>(gamma + c, gv);
  ldv<V>(beta + c, bv);
  if (infer) {
#pragma unroll
    for (int k = 0; k < V; ++k) is[k] = rsqrtf(is[k] + eps);
  }
  auto one = [&](const float (&xv)[V], int64_t r) {
    float o[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float t = bn_affine(xv[k], mv[k], is[k], gv[k], bv[k]);
      if (relu) t = fmaxf(t, 0.f);
      o[k] = t;
    }
    stv<V>(y + r * C + c, o);
  };
  const int64_t stride = prow, gstep = (int64_t)gridDim.y * 4 * prow;
  for (int64_t r = (int64_t)blockIdx.y * 4 * prow + r0; r < rows; r += gstep) {
    if (r + 3 * stride < rows) {
      float x0[V], x1[V], x2[V], x3[V];
      ldv<V>(x + r * C + c, x0);
      ldv<V>(x + (r + stride) * C + c, x1);
      ldv<V>(x + (r + 2 * stride) * C + c, x2);
      ldv<V>(x + (r + 3 * stride) * C + c, x3);
      one(x0, r); one(x1, r + stride); one(x2, r + 2 * stride); one(x3, r + 3 * stride);
    } else {
      for (int64_t q = r; q < rows; q += stride) {
        float x0[V];
        ldv<V>(x + q * C + c, x0);
        one(x0, q);
      }
    }
  }
}
constexpr int BN_APPLY_PERIODS = 4;   // bn_cols_grid's `unroll`: the periods of prow rows a group (blockIdx.y) owns per trip - four consecutive ones

template <int V, typename T, int MODE>
__global__ __launch_bounds__(256) void bn_bwd_apply_cols_kernel(const T* __restrict__ x, const T* __restrict__ y,
                                                                const T* __restrict__ dy, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ dgamma,
                                                                const float* __restrict__ dbeta, T* __restrict__ dx, int64_t rows,
                                                                int C, int prow, FastDiv fd_cv) {
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, cv = (uint32_t)(C / V);
  const uint32_t r0 = fd_div(i0, fd_cv);
  const int c = (int)(i0 - r0 * cv) * V;
  float mv[V], iv[V], gam[V], dg[V], db[V], bt[V];
  ldv<V>(mean + c, mv);
  ldv<V>(invstd + c, iv);
  ldv<V>(gamma + c, gam);
  ldv<V>(dgamma + c, dg);
  ldv<V>(dbeta + c, db);
  if constexpr (MODE == 2) ldv<V>(beta + c, bt);
  const float inv_n = 1.0f / (float)rows;
  auto one = [&](const float (&xv)[V], float (&gv)[V], const float (&yv)[V], int64_t r) {
    float o[V];
    bn_mask<MODE>(gv, xv, yv, mv, iv, gam, bt);
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = bn_dx(xv[k], gv[k], mv[k], iv[k], gam[k], dg[k], db[k], inv_n);
    stv<V>(dx + r * C + c, o);
  };
  // (two rows a whole grid apart: measured 2 - 5 % faster here than two adjacent periods, the opposite of the forward kernel)
  const int64_t stride = (int64_t)gridDim.y * prow, gstep = 2 * stride;
  for (int64_t r = (int64_t)blockIdx.y * prow + r0; r < rows; r += gstep) {
    if (r + stride < rows) {
      float x0[V], x1[V], g0[V], g1[V], y0[V], y1[V];
      ldv<V>(x + r * C + c, x0);
      ldv<V>(x + (r + stride) * C + c, x1);
      ldv<V>(dy + r * C + c, g0);
      ldv<V>(dy + (r + stride) * C + c, g1);
      if constexpr (MODE == 1) {
        ldv<V>(y + r * C + c, y0);
        ldv<V>(y + (r + stride) * C + c, y1);
      }
      one(x0, g0, y0, r);
      one(x1, g1, y1, r + stride);
    } else {
      float x0[V], g0[V], y0[V];
      ldv<V>(x + r * C + c, x0);
      ldv<V>(dy + r * C + c, g0);
      if constexpr (MODE == 1) ldv<V>(y + r * C + c, y0);
      one(x0, g0, y0, r);
    }
  }
}
constexpr int BN_BWD_PERIODS = 1;   // ONE: this kernel's two rows lie a whole grid apart, so a group owns a single period per trip

// bn_bwd_apply_kernel / bn_bwd_apply_cols_kernel with dy from the thin source (BnBwdThinOp): same index space, same expressions
template <int V, int MODE, int CO>
__global__ void bn_bwd_apply_thin_kernel(const BnBwdThinOp<MODE, CO> q, float* __restrict__ dx, int64_t rows, FastDiv fd_cv) {
  const int C = q.C;
  const uint32_t cv = C / V;
  const uint32_t total = (uint32_t)(rows * cv);
  const uint32_t stride = gridDim.x * blockDim.x;
  const float inv_n = 1.0f / (float)rows;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = fd_div(i, fd_cv);
    const int c = (int)(i - (uint32_t)r * cv) * V;
    float xv[V], gv[V], mv[V], iv[V], gam[V], dg[V], db[V], o[V], wv[V][CO];
    ldv<V>(q.x + r * C + c, xv);
    thin_w<V, CO>(q.w, c, wv);
    thin_dy<V, CO>(q.g + r * q.y_ld, wv, gv);
    ldv<V>(q.mean + c, mv);
    ldv<V>(q.invstd + c, iv);
    ldv<V>(q.gamma + c, gam);
    ldv<V>(q.dgamma + c, dg);
    ldv<V>(q.dbeta + c, db);
    if constexpr (MODE == 2) {
      float bt[V];
      ldv<V>(q.beta + c, bt);
#pragma unroll
      for (int k = 0; k < V; ++k) gv[k] = bn_affine(xv[k], mv[k], iv[k], gam[k], bt[k]) > 0.f ? gv[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float xh = (xv[k] - mv[k]) * iv[k];
      o[k] = gam[k] * iv[k] * (gv[k] - db[k] * inv_n - xh * dg[k] * inv_n);
    }
    stv<V>(dx + r * C + c, o);
  }
}

template <int V, int MODE, int CO>
__global__ __launch_bounds__(256) void bn_bwd_apply_cols_thin_kernel(const BnBwdThinOp<MODE, CO> q, float* __restrict__ dx,
                                                                     int64_t rows, int prow, FastDiv fd_cv) {
  const int C = q.C;
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, cv = (uint32_t)(C / V);
  const uint32_t r0 = fd_div(i0, fd_cv);
  const int c = (int)(i0 - r0 * cv) * V;
  float mv[V], iv[V], gam[V], dg[V], db[V], bt[V], wv[V][CO];
  ldv<V>(q.mean + c, mv);
  ldv<V>(q.invstd + c, iv);
  ldv<V>(q.gamma + c, gam);
  ldv<V>(q.dgamma + c, dg);
  ldv<V>(q.dbeta + c, db);
  if constexpr (MODE == 2) ldv<V>(q.beta + c, bt);
  thin_w<V, CO>(q.w, c, wv);
  const float inv_n = 1.0f / (float)rows;
  auto one = [&](const float (&xv)[V], float (&gv)[V], int64_t r) {
    float o[V];
    bn_mask<MODE>(gv, xv, xv, mv, iv, gam, bt);   // (MODE 0 / 2 never read the y operand)
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = bn_dx(xv[k], gv[k], mv[k], iv[k], gam[k], dg[k], db[k], inv_n);
    stv<V>(dx + r * C + c, o);
  };
  const int64_t stride = (int64_t)gridDim.y * prow, gstep = 2 * stride;
  for (int64_t r = (int64_t)blockIdx.y * prow + r0; r < rows; r += gstep) {
    if (r + stride < rows) {
      float x0[V], x1[V], g0[V], g1[V];
      ldv<V>(q.x + r * C + c, x0);
      ldv<V>(q.x + (r + stride) * C + c, x1);
      thin_dy<V, CO>(q.g + r * q.y_ld, wv, g0);
      thin_dy<V, CO>(q.g + (r + stride) * q.y_ld, wv, g1);
      one(x0, g0, r);
      one(x1, g1, r + stride);
    } else {
      float x0[V], g0[V];
      ldv<V>(q.x + r * C + c, x0);
      thin_dy<V, CO>(q.g + r * q.y_ld, wv, g0);
      one(x0, g0, r);
    }
  }
}

// y = [relu]( f_a(a) + f_b(b) ), f = BatchNormalization's apply (training: saved mean / invstd; inference: moving mean /
// variance) for an operand whose parameter pointers are given, the identity otherwise: the residual add of an Xception block
// applies the normalisation of the branch (and of the 1x1 shortcut) it sums, so that tensor is never written and read again
// (sg_add2_bn; one of BatchNormalization's two forward passes for those layers).  Column-stationary like bn_apply_cols_kernel;
// the same expression, so with fp32 storage the result has the bits of bn_apply + add_n.
struct Add2BnArgs {
  const float* mean[2];
  const float* invstd[2];
  const float* gamma[2];
  const float* beta[2];
  int relu_op[2];   // the operand's BatchNormalization has a fused ReLU (Res34's blocks activate before they add)
};

template <int V, typename T>
__global__ __launch_bounds__(256) void add2_bn_kernel(const T* __restrict__ a, const T* __restrict__ b, const Add2BnArgs q,
                                                      T* __restrict__ y, int64_t rows, int C, int relu, float eps, int infer,
                                                      int prow, FastDiv fd_cv) {
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, cv = (uint32_t)(C / V);
  const uint32_t r0 = fd_div(i0, fd_cv);
  const int c = (int)(i0 - r0 * cv) * V;
  float mv[2][V], is[2][V], gv[2][V], bv[2][V];
  const bool on[2] = {q.mean[0] != nullptr, q.mean[1] != nullptr};
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    if (on[o]) {
      ldv<V>(q.mean[o] + c, mv[o]);
      ldv<V>(q.invstd[o] + c, is[o]);
      ldv<V>(q.gamma[o] + c, gv[o]);
      ldv<V>(q.beta[o] + c, bv[o]);
      if (infer) {
#pragma unroll
        for (int k = 0; k < V; ++k) is[o][k] = rsqrtf(is[o][k] + eps);
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) { mv[o][k] = 0.f; is[o][k] = 1.f; gv[o][k] = 1.f; bv[o][k] = 0.f; }
    }
  }
  auto one = [&](const float (&xa)[V], const float (&xb)[V], int64_t r) {
    float o[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float ta = on[0] ? bn_affine(xa[k], mv[0][k], is[0][k], gv[0][k], bv[0][k]) : xa[k];
      float tb = on[1] ? bn_affine(xb[k], mv[1][k], is[1][k], gv[1][k], bv[1][k]) : xb[k];
      if (q.relu_op[0]) ta = fmaxf(ta, 0.f);
      if (q.relu_op[1]) tb = fmaxf(tb, 0.f);
      float t = ta + tb;
      if (relu) t = fmaxf(t, 0.f);
      o[k] = t;
    }
    stv<V>(y + r * C + c, o);
  };
  const int64_t stride = prow, gstep = (int64_t)gridDim.y * 2 * prow;
  for (int64_t r = (int64_t)blockIdx.y * 2 * prow + r0; r < rows; r += gstep) {
    if (r + stride < rows) {
      float a0[V], a1[V], b0[V], b1[V];
      ldv<V>(a + r * C + c, a0);
      ldv<V>(a + (r + stride) * C + c, a1);
      ldv<V>(b + r * C + c, b0);
      ldv<V>(b + (r + stride) * C + c, b1);
      one(a0, b0, r);
      one(a1, b1, r + stride);
    } else {
      float a0[V], b0[V];
      ldv<V>(a + r * C + c, a0);
      ldv<V>(b + r * C + c, b0);
      one(a0, b0, r);
    }
  }
}
constexpr int BN_ADD2_PERIODS = 2;   // two consecutive periods

// ---- who chooses the kernels: plan_bn() ---------------------------------------------------------------------------------
// One BnPlan per call, a pure function of (CU count, storage type, rows, C, pass, operands aligned) and the SG_BN_COLS / SG_SEG_FUSED /
// SG_FINALIZE_LANES switches.  The six entry points refuse and launch from it, sg_bn_ws_bytes adds its bytes up and sg_bn_plan hands it
// out (include/segengine.h: sg_bn_plan_t), so a query and a launch cannot disagree (tests/_bn_cases.py compares each with its mirror).
struct BnPlan : sg_bn_plan_t { SegPlan seg; int refused; };   // seg: the reduction (seg_V .. seg_S are its copy); refused: add2's code

// grid of the column-stationary kernels: gx = the blocks of one period (b0 x 256 threads = prow whole rows), gy = groups of
// `unroll` consecutive periods; a thread walks groups gridDim.y apart.  Returns false when no such grid of a sensible size
// exists (the flat kernels take the launch).
inline bool bn_cols_grid(int num_cus, int64_t rows, int cv, int unroll, sg_bn_plan_t& pl) {
  int g = 256, a = cv;
  while (a) { const int t_ = g % a; g = a; a = t_; }   // g = gcd(256, cv)
  const int64_t b0 = cv / g;
  if (b0 > 16384) return false;
  pl.prow = 256 / g;
  int64_t k = sg_cdiv((int64_t)8 * num_cus, b0);
  const int64_t maxk = sg_cdiv(rows, (int64_t)unroll * pl.prow);
  if (k > maxk) k = maxk;
  if (k > 65535) k = 65535;
  if (k < 1) k = 1;
  pl.gx = (int)b0; pl.gy = (int)k;
  return true;
}

inline BnPlan plan_bn(int num_cus, int dtype, int64_t rows, int C, int pass, bool aligned) {
  BnPlan pl = {};
  const bool vec = aligned && C % 4 == 0, add2 = pass == SG_BN_ADD2;   // sg_add2_bn has column kernels only, whatever SG_BN_COLS
  pl.V = (vec && dtype == SG_BF16 && C % 8 == 0) ? 8 : (vec ? 4 : 1);   // bf16: 8 channels = one 16-byte access
  const int unroll = add2 ? BN_ADD2_PERIODS : ((pass == SG_BN_BWD || pass == SG_BN_BWD_APPLY) ? BN_BWD_PERIODS : BN_APPLY_PERIODS);
  pl.cols = vec && (add2 || sg_switch<SW_BN_COLS>()) && bn_cols_grid(num_cus, rows, C / pl.V, unroll, pl);
  if (!pl.cols && add2) { pl = {}; pl.refused = SG_EUNSUPPORTED; }
  else if (!pl.cols) { pl.gx = (int)ew_blocks(rows * (C / pl.V), 8192); pl.gy = 1; }
  if (pass == SG_BN_FWD || pass == SG_BN_BWD) {
    pl.seg = seg_plan<2>(num_cus, 1, rows, C, vec, dtype == SG_BF16);
    pl.seg_V = pl.seg.V; pl.seg_TX = pl.seg.TX; pl.seg_TY = pl.seg.TY; pl.seg_gx = pl.seg.gx; pl.seg_S = pl.seg.S;
    pl.fused = seg_fused_alone(pl.seg.S);
    pl.fin_lanes = pl.fused ? 0 : seg_finalize_lanes(pl.seg.S);
    pl.ws_bytes = pl.seg.part_bytes;
  }
  return pl;
}

// every entry point's and the query's first checks (chunked: sg_add2_bn walks 2^31 elements and more in row chunks) ...
inline int bn_check(const sg_ctx* ctx, int dtype, int64_t rows, int C, bool chunked, const char* who) {
  SG_CHECK_ARG(ctx && (dtype == SG_F32 || dtype == SG_BF16), "%s: bad ctx/dtype", who);
  SG_CHECK_ARG(rows > 0 && C > 0, "%s: bad argument", who);
  SG_CHECK_ARG(chunked || rows * C < (1ll << 31), "%s: tensor exceeds 2^31 elements", who);
  return 0;
}

// ... and their last: the plan's refusal, then the workspace the plan asks for
inline int bn_refuse(const BnPlan& pl, const char* who, const void* ws, size_t ws_bytes) {
  if (pl.refused) {
    sg_set_error("%s: needs C %% 4 == 0, 16-byte aligned tensors and a column grid; apply the BatchNormalization and add instead", who);
    return pl.refused;
  }
  if (pl.ws_bytes && (!ws || ws_bytes < pl.ws_bytes)) {
    sg_set_error("%s: workspace %zu < %zu", who, ws_bytes, pl.ws_bytes);
    return SG_EWORKSPACE;
  }
  return 0;
}

// The template forms, named once: the plan's five <V, column form> (there is no scalar column kernel) and the backward's mask mode
template <class F>
inline void bn_with_form(const BnPlan& pl, F&& fn) {
  constexpr std::integral_constant<int, 8> v8{}; constexpr std::integral_constant<int, 4> v4{};
  if (pl.V == 8) pl.cols ? fn(v8, std::true_type{}) : fn(v8, std::false_type{});
  else if (pl.V == 4) pl.cols ? fn(v4, std::true_type{}) : fn(v4, std::false_type{});
  else fn(std::integral_constant<int, 1>{}, std::false_type{});
}
template <class F>
inline int bn_with_mode(int relu, const void* beta, F&& fn) {   // with beta the ReLU mask is recomputed from x instead of read from y
  if (!relu) return fn(std::integral_constant<int, 0>{});
  return beta ? fn(std::integral_constant<int, 2>{}) : fn(std::integral_constant<int, 1>{});
}

// launch what the plan says: bn_apply_cols_kernel or bn_apply_kernel (infer: `invstd` holds the moving variance)
template <typename T>
int launch_bn_apply(hipStream_t st, const BnPlan& pl, const T* x, const float* mean, const float* invstd, const float* gamma,
                    const float* beta, T* y, int64_t rows, int C, int relu, float eps, int infer) {
  const FastDiv fd = make_fastdiv((uint32_t)(C / pl.V));
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  bn_with_form(pl, [&](auto v, auto cols) {
    constexpr int V = decltype(v)::value;
    if constexpr (decltype(cols)::value)
      hipLaunchKernelGGL((bn_apply_cols_kernel<V, T>), grid, dim3(256), 0, st, x, mean, invstd, gamma, beta, y, rows, C, relu, eps,
                         infer, pl.prow, fd);
    else
      hipLaunchKernelGGL((bn_apply_kernel<V, T>), grid, dim3(256), 0, st, x, mean, invstd, gamma, beta, y, rows, C, relu, eps, infer, fd);
  });
  SG_LAUNCH_CHECK(pl.cols ? "bn_apply_cols_kernel" : "bn_apply_kernel");
  return 0;
}

// dx of a training-mode BatchNormalization from its finished column sums (dbeta = sum g, dgamma = sum g * xhat) on the operands
// of q: the apply pass of sg_bn_train_bwd, also entered on its own by sg_bn_train_bwd_apply
template <typename T, int MODE>
int launch_bn_bwd_apply(hipStream_t st, const BnPlan& pl, const BnBwdOp<T, MODE>& q, T* dx, int64_t rows) {
  const FastDiv fd = make_fastdiv((uint32_t)(q.C / pl.V));
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  bn_with_form(pl, [&](auto v, auto cols) {
    constexpr int V = decltype(v)::value;
    if constexpr (decltype(cols)::value)
      hipLaunchKernelGGL((bn_bwd_apply_cols_kernel<V, T, MODE>), grid, dim3(256), 0, st, q.x, q.y, q.dy, q.mean, q.invstd, q.gamma,
                         q.beta, q.dgamma, q.dbeta, dx, rows, q.C, pl.prow, fd);
    else
      hipLaunchKernelGGL((bn_bwd_apply_kernel<V, T, MODE>), grid, dim3(256), 0, st, q.x, q.y, q.dy, q.mean, q.invstd, q.gamma, q.beta,
                         q.dgamma, q.dbeta, dx, rows, q.C, fd);
  });
  SG_LAUNCH_CHECK(pl.cols ? "bn_bwd_apply_cols_kernel" : "bn_bwd_apply_kernel");
  return 0;
}

template <int MODE, int CO>
int launch_bn_bwd_apply_thin(hipStream_t st, const BnPlan& pl, const BnBwdThinOp<MODE, CO>& q, float* dx, int64_t rows) {
  const FastDiv fd = make_fastdiv((uint32_t)(q.C / pl.V));
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  bn_with_form(pl, [&](auto v, auto cols) {
    constexpr int V = decltype(v)::value;
    if constexpr (V == 8) return;   // (bf16 storage only: refused before any launch)
    else if constexpr (decltype(cols)::value)
      hipLaunchKernelGGL((bn_bwd_apply_cols_thin_kernel<V, MODE, CO>), grid, dim3(256), 0, st, q, dx, rows, pl.prow, fd);
    else
      hipLaunchKernelGGL((bn_bwd_apply_thin_kernel<V, MODE, CO>), grid, dim3(256), 0, st, q, dx, rows, fd);
  });
  SG_LAUNCH_CHECK(pl.cols ? "bn_bwd_apply_cols_thin_kernel" : "bn_bwd_apply_thin_kernel");
  return 0;
}

// rows per launch of sg_add2_bn: its kernel indexes with 32 bits, so a tensor of 2^31 elements or more (the BatchNormalization
// in front of this add has already handed its RAW input on: there is no unfused form to fall back to) is walked in row chunks
// below that, each an even number of rows so that a chunk starts 16-byte aligned with bf16 storage too.  Element-wise: same bits.
inline int64_t add2_chunk_rows(int64_t rows, int C) { return rows * C < (1ll << 31) ? rows : (((1ll << 31) - 1) / C) & ~1ll; }

// sg_bn_apply (given mean / invstd) and sg_bn_infer (moving mean / variance, eps under the root in the kernel)
int bn_apply_entry(const char* who, sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* x, const void* gamma,
                   const void* beta, const void* mean, const void* invstd, void* y, int relu, float eps, int infer) {
  if (int e = bn_check(ctx, dtype, rows, C, false, who)) return e;
  SG_CHECK_ARG(x && gamma && beta && mean && invstd && y, "%s: bad argument", who);
  const BnPlan pl = plan_bn(ctx->num_cus, dtype, rows, C, SG_BN_APPLY, sg_all_aligned16({x, y}));
  SG_DTYPE_SWITCH(dtype, who, {
    return launch_bn_apply<T>((hipStream_t)stream, pl, (const T*)x, (const float*)mean, (const float*)invstd, (const float*)gamma,
                              (const float*)beta, (T*)y, rows, C, relu, eps, infer);
  });
  return 0;
}

}  // namespace

extern "C" {

int sg_bn_plan(const sg_ctx* ctx, int dtype, int64_t rows, int C, int pass, int aligned, sg_bn_plan_t* out) {
  SG_CHECK_ARG(out, "sg_bn_plan: null out");
  *out = sg_bn_plan_t{};
  SG_CHECK_ARG(pass >= SG_BN_FWD && pass <= SG_BN_ADD2, "sg_bn_plan: bad pass");
  if (int e = bn_check(ctx, dtype, rows, C, pass == SG_BN_ADD2, "sg_bn_plan")) return e;
  if (pass == SG_BN_ADD2) rows = add2_chunk_rows(rows, C);
  SG_CHECK_ARG(rows > 0, "sg_bn_plan: a single row exceeds 2^31 elements");
  const BnPlan pl = plan_bn(ctx->num_cus, dtype, rows, C, pass, aligned != 0);
  if (int e = bn_refuse(pl, "sg_bn_plan", out, pl.ws_bytes)) return e;   // (a query brings no workspace: that check passes)
  *out = pl;
  return 0;
}

// the largest ws_bytes over what the query cannot know - the storage type and whether the operands will be aligned - + 256
size_t sg_bn_ws_bytes(const sg_ctx* ctx, int64_t rows, int C) {
  if (!ctx) return 0;
  size_t m = 0;
  for (int dtype : {SG_F32, SG_BF16})
    for (bool aligned : {false, true}) m = std::max(m, plan_bn(ctx->num_cus, dtype, rows, C, SG_BN_FWD, aligned).ws_bytes);
  return m + 256;
}

int sg_bn_train_fwd(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* x, const void* gamma, const void* beta,
                    void* moving_mean, void* moving_var, void* y, void* save_mean, void* save_invstd, float momentum, float eps,
                    int relu, int unbiased_update, void* ws, size_t ws_bytes) {
  if (int e = bn_check(ctx, dtype, rows, C, false, "sg_bn_train_fwd")) return e;
  SG_CHECK_ARG(x && gamma && beta && moving_mean && moving_var && y && save_mean && save_invstd, "sg_bn_train_fwd: bad argument");
  const BnPlan pl = plan_bn(ctx->num_cus, dtype, rows, C, SG_BN_FWD, sg_all_aligned16({x, y}));
  if (int e = bn_refuse(pl, "sg_bn_train_fwd", ws, ws_bytes)) return e;
  SG_DTYPE_SWITCH(dtype, "sg_bn_train_fwd", {
    const BnStatsOp<T> op = {(const T*)x, C, rows, (float*)moving_mean, (float*)moving_var, (float*)save_mean, (float*)save_invstd,
                             momentum, eps, unbiased_update};
    if (int e = seg_reduce_launch(op, pl.seg, 1, rows, C, (float*)ws, (hipStream_t)stream, "bn_stats")) return e;
    return launch_bn_apply<T>((hipStream_t)stream, pl, op.x, op.save_mean, op.save_invstd, (const float*)gamma, (const float*)beta, (T*)y, rows, C, relu,
                              eps, 0);
  });
  return 0;
}

int sg_bn_train_bwd(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* x, const void* y, const void* dy,
                    const void* gamma, const void* beta, const void* save_mean, const void* save_invstd, void* dx, void* dgamma,
                    void* dbeta, int relu, void* ws, size_t ws_bytes) {
  if (int e = bn_check(ctx, dtype, rows, C, false, "sg_bn_train_bwd")) return e;
  SG_CHECK_ARG(x && dy && gamma && save_mean && save_invstd && dx && dgamma && dbeta, "sg_bn_train_bwd: bad argument");
  SG_CHECK_ARG(!relu || y || beta, "sg_bn_train_bwd: relu set but neither y nor beta given");
  const BnPlan pl = plan_bn(ctx->num_cus, dtype, rows, C, SG_BN_BWD, sg_all_aligned16({x, dy, dx, relu ? y : nullptr}));
  if (int e = bn_refuse(pl, "sg_bn_train_bwd", ws, ws_bytes)) return e;
  SG_DTYPE_SWITCH(dtype, "sg_bn_train_bwd", {
    return bn_with_mode(relu, beta, [&](auto m) -> int {
      const BnBwdOp<T, decltype(m)::value> op = {(const T*)x, (const T*)y, (const T*)dy, (const float*)save_mean, (const float*)save_invstd,
                                                 (const float*)gamma, (const float*)beta, (float*)dgamma, (float*)dbeta, C};
      if (int e = seg_reduce_launch(op, pl.seg, 1, rows, C, (float*)ws, (hipStream_t)stream, "bn_bwd_reduce")) return e;
      return launch_bn_bwd_apply((hipStream_t)stream, pl, op, (T*)dx, rows);
    });
  });
  return 0;
}

int sg_bn_train_bwd_apply(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* x, const void* dy, const void* gamma,
                          const void* beta, const void* save_mean, const void* save_invstd, const void* dgamma, const void* dbeta,
                          void* dx, int relu) {
  if (int e = bn_check(ctx, dtype, rows, C, false, "sg_bn_train_bwd_apply")) return e;
  SG_CHECK_ARG(x && dy && gamma && save_mean && save_invstd && dx && dgamma && dbeta, "sg_bn_train_bwd_apply: bad argument");
  SG_CHECK_ARG(!relu || beta, "sg_bn_train_bwd_apply: relu needs beta (the mask is recomputed from x)");
  const BnPlan pl = plan_bn(ctx->num_cus, dtype, rows, C, SG_BN_BWD_APPLY, sg_all_aligned16({x, dy, dx}));
  SG_DTYPE_SWITCH(dtype, "sg_bn_train_bwd_apply", {
    return bn_with_mode(relu, beta, [&](auto m) -> int {   // (the finished sums are only read: the casts drop a const the kernels put back)
      const BnBwdOp<T, decltype(m)::value> op = {(const T*)x, nullptr, (const T*)dy, (const float*)save_mean, (const float*)save_invstd,
                                                 (const float*)gamma, (const float*)beta, (float*)dgamma, (float*)dbeta, C};
      return launch_bn_bwd_apply((hipStream_t)stream, pl, op, (T*)dx, rows);
    });
  });
  return 0;
}

// fp32 storage only: under bf16 the thin dgrad rounds dy through the storage type, which these kernels do not
int sg_bn_train_bwd_thin_ok(const sg_ctx* ctx, int dtype, int64_t rows, int C, int CO, int y_ld) {
  return ctx && dtype == SG_F32 && rows > 0 && C > 0 && rows * C < (1ll << 31) && CO >= 1 && CO <= 4 && y_ld >= CO &&
         rows * y_ld < (1ll << 31);
}

int sg_bn_train_bwd_thin(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, int CO, int y_ld, const void* x, const void* g,
                         const void* w, const void* gamma, const void* beta, const void* save_mean, const void* save_invstd, void* dx,
                         void* dgamma, void* dbeta, int relu, void* ws, size_t ws_bytes) {
  if (int e = bn_check(ctx, dtype, rows, C, false, "sg_bn_train_bwd_thin")) return e;
  SG_CHECK_ARG(x && g && w && gamma && save_mean && save_invstd && dx && dgamma && dbeta, "sg_bn_train_bwd_thin: bad argument");
  SG_CHECK_ARG(!relu || beta, "sg_bn_train_bwd_thin: relu needs beta (the mask is recomputed from x)");
  if (!sg_bn_train_bwd_thin_ok(ctx, dtype, rows, C, CO, y_ld)) {
    sg_set_error("sg_bn_train_bwd_thin: needs fp32 storage and 1 <= CO <= 4, CO <= y_ld; run the thin dgrad and sg_bn_train_bwd instead");
    return SG_EUNSUPPORTED;
  }
  // the plan of the materialised call (dy there is a dense tensor of x's shape, aligned like dx): same grids, same order of sums
  const BnPlan pl = plan_bn(ctx->num_cus, dtype, rows, C, SG_BN_BWD, sg_all_aligned16({x, dx}));
  if (int e = bn_refuse(pl, "sg_bn_train_bwd_thin", ws, ws_bytes)) return e;
  auto run = [&](auto m, auto co) -> int {
    const BnBwdThinOp<decltype(m)::value, decltype(co)::value> op = {
        (const float*)x, (const float*)g, (const float*)w, (const float*)save_mean, (const float*)save_invstd, (const float*)gamma,
        (const float*)beta, (float*)dgamma, (float*)dbeta, C, y_ld};
    if (int e = seg_reduce_launch(op, pl.seg, 1, rows, C, (float*)ws, (hipStream_t)stream, "bn_bwd_thin_reduce")) return e;
    return launch_bn_bwd_apply_thin((hipStream_t)stream, pl, op, (float*)dx, rows);
  };
  auto with_co = [&](auto m) -> int {
    switch (CO) {
      case 1: return run(m, std::integral_constant<int, 1>{});
      case 2: return run(m, std::integral_constant<int, 2>{});
      case 3: return run(m, std::integral_constant<int, 3>{});
      default: return run(m, std::integral_constant<int, 4>{});
    }
  };
  return relu ? with_co(std::integral_constant<int, 2>{}) : with_co(std::integral_constant<int, 0>{});
}

int sg_bn_apply(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* x, const void* gamma,
                const void* beta, const void* mean, const void* invstd, void* y, int relu) {
  return bn_apply_entry("sg_bn_apply", ctx, stream, dtype, rows, C, x, gamma, beta, mean, invstd, y, relu, 0.f, 0);
}

int sg_bn_infer(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* x, const void* gamma,
                const void* beta, const void* moving_mean, const void* moving_var, void* y, float eps, int relu) {
  return bn_apply_entry("sg_bn_infer", ctx, stream, dtype, rows, C, x, gamma, beta, moving_mean, moving_var, y, relu, eps, 1);
}

int sg_add2_bn(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* a, const void* b, const void* a_mean,
               const void* a_invstd, const void* a_gamma, const void* a_beta, const void* b_mean, const void* b_invstd,
               const void* b_gamma, const void* b_beta, void* y, int relu, int infer, float eps, int a_relu, int b_relu) {
  if (int e = bn_check(ctx, dtype, rows, C, true, "sg_add2_bn")) return e;
  SG_CHECK_ARG(a && b && y, "sg_add2_bn: bad argument");
  SG_CHECK_ARG((a_mean != nullptr) == (a_invstd != nullptr && a_gamma != nullptr && a_beta != nullptr) &&
                   (b_mean != nullptr) == (b_invstd != nullptr && b_gamma != nullptr && b_beta != nullptr),
               "sg_add2_bn: an operand's four BatchNormalization parameters come together or not at all");
  const bool aligned = sg_all_aligned16({a, b, y});
  const int64_t chunk_rows = add2_chunk_rows(rows, C);
  SG_CHECK_ARG(chunk_rows > 0, "sg_add2_bn: a single row exceeds 2^31 elements");
  const Add2BnArgs q = {{(const float*)a_mean, (const float*)b_mean}, {(const float*)a_invstd, (const float*)b_invstd},
                        {(const float*)a_gamma, (const float*)b_gamma}, {(const float*)a_beta, (const float*)b_beta},
                        {(a_mean && a_relu) ? 1 : 0, (b_mean && b_relu) ? 1 : 0}};
  SG_DTYPE_SWITCH(dtype, "sg_add2_bn", {
    for (int64_t r0 = 0; r0 < rows; r0 += chunk_rows) {
      const int64_t nr = rows - r0 < chunk_rows ? rows - r0 : chunk_rows;
      const BnPlan pl = plan_bn(ctx->num_cus, dtype, nr, C, SG_BN_ADD2, aligned);
      if (int e = bn_refuse(pl, "sg_add2_bn", nullptr, 0)) return e;   // (whatever the rows: the first chunk refuses, before any launch)
      bn_with_form(pl, [&](auto v, auto cols) {
        constexpr int V = decltype(v)::value;
        if constexpr (decltype(cols)::value)   // (the plan refuses what has no column grid)
          hipLaunchKernelGGL((add2_bn_kernel<V, T>), dim3((unsigned)pl.gx, (unsigned)pl.gy), dim3(256), 0, (hipStream_t)stream,
                             (const T*)a + r0 * C, (const T*)b + r0 * C, q, (T*)y + r0 * C, nr, C, relu, eps, infer, pl.prow,
                             make_fastdiv((uint32_t)(C / V)));
      });
    }
  });
  SG_LAUNCH_CHECK("add2_bn_kernel");
  return 0;
}

}  // extern "C"
