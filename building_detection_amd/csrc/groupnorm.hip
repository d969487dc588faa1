// GroupNormalization (Wu & He 2018; tf.keras.layers.GroupNormalization) for NHWC [N][HW][C]: G groups of Cg = C / G adjacent
// channels, statistics per (image, group) over HW * Cg elements, the same function in training and inference.
// HBM-bound like BatchNormalization (csrc/norm.hip) and built the same way, three launches per direction:
//   forward   1 segment reducer (sg_reduce.h; segment = image): per (n, c) the sums of d and d^2, d = x - pivot, pivot = the
//               channel's first pixel of that image, so the single-pass variance does not cancel
//             2 fold: per (n, g) the row slabs' partial sums are added in fp64 and the Cg channels - each about its own pivot -
//               are combined with the parallel-variance (Chan) update; writes mean and invstd [N * G]
//             3 apply: y = gamma_c (x - mean_ng) invstd_ng + beta_c [ReLU]
//   backward  1 segment reducer: per (n, c) S1 = sum g, S2 = sum g xhat, g = dy masked by the fused ReLU (recomputed from x)
//             2 fold: per (n, g) A = sum_c gamma_c S1 / m, B = sum_c gamma_c S2 / m (m = HW * Cg), per (n, c) the fp64 totals
//             3 apply: dx = invstd_ng (gamma_c g - A_ng - xhat B_ng); its trailing workgroups add the totals over n in fixed
//               order into dgamma_c = sum_n S2, dbeta_c = sum_n S1
// The fold takes the reducer's partial rows itself (the reducer runs without its second stage), so a row split costs no
// fourth launch.  No atomics, no host round trip; every sum has a fixed order that depends on (HW, C, G) only - never on N,
// so an image's result does not depend on the batch it is in.
#include "sg_reduce.h"

namespace {

// The per-element expressions, each written once: forward, backward mask and backward apply agree to the bit
__device__ __forceinline__ float gn_affine(float x, float mean, float invstd, float gamma, float beta) {
  return fmaf((x - mean) * invstd, gamma, beta);
}
template <int RELU, int V>
__device__ __forceinline__ void gn_mask(float (&g)[V], const float (&x)[V], const float (&mean)[V], const float (&invstd)[V],
                                        const float (&gamma)[V], const float (&beta)[V]) {
  if constexpr (RELU) {
#pragma unroll
    for (int i = 0; i < V; ++i) g[i] = gn_affine(x[i], mean[i], invstd[i], gamma[i], beta[i]) > 0.f ? g[i] : 0.f;
  }
}
__device__ __forceinline__ float gn_dx(float x, float g, float mean, float invstd, float gamma, float a_m, float b_m) {
  // no contraction here: the product gamma g is rounded on its own, so that where it equals A / m - one channel per group and
  // one pixel - the difference is exactly 0 and not the product's rounding residue
#pragma clang fp contract(off)
  const float xh = (x - mean) * invstd;
  const float p = gamma * g;
  return invstd * ((p - a_m) - xh * b_m);
}

// per-thread constants of a chunk of V channels of image n: the group statistics of each channel (a group boundary may fall
// inside the chunk: one index per channel) and the per-channel parameters (null pointer: 1 / 0)
template <int V>
struct GnCtx {
  float mv[V], iv[V], gm[V], bt[V];
};
template <int V>
__device__ __forceinline__ void gn_params(const float* __restrict__ gamma, const float* __restrict__ beta, int c, float (&gm)[V],
                                          float (&bt)[V]) {
  if (gamma) ldv<V>(gamma + c, gm);
  else {
#pragma unroll
    for (int k = 0; k < V; ++k) gm[k] = 1.f;
  }
  if (beta) ldv<V>(beta + c, bt);
  else {
#pragma unroll
    for (int k = 0; k < V; ++k) bt[k] = 0.f;
  }
}
template <int V>
__device__ __forceinline__ void gn_group_stats(const float* __restrict__ a, const float* __restrict__ b, int n, int G, int c,
                                               const FastDiv& fd_cg, float (&av)[V], float (&bv)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int64_t q = (int64_t)n * G + fd_div((uint32_t)(c + k), fd_cg);
    av[k] = a[q];
    bv[k] = b[q];
  }
}

// ---- launch 1: the segment reducer's Ops (segment = image; finalize is never reached: the fold takes the partial rows) ----
template <typename T>
struct GnStatsOp {
  static constexpr int NOUT = 2;
  const T* __restrict__ x;
  int C;
  int64_t hw;

  template <int V>
  struct Piv { float k[V]; };
  template <int V>
  __device__ __forceinline__ Piv<V> begin(int seg, int c) const {
    Piv<V> p;
    ldv<V>(x + (int64_t)seg * hw * C + c, p.k);  // pivot = the image's first pixel
    return p;
  }
  template <int V>
  __device__ __forceinline__ void accum(int seg, int64_t r, int c, float (&acc)[2][V], const Piv<V>& p) const {
    float v[V];
    ldv<V>(x + ((int64_t)seg * hw + r) * C + c, v);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float d = v[i] - p.k[i];
      acc[0][i] += d;
      acc[1][i] = fmaf(d, d, acc[1][i]);
    }
  }
  __device__ __forceinline__ void finalize(int, int, const double (&)[2]) const {}
};

template <typename T, int RELU>
struct GnBwdOp {
  static constexpr int NOUT = 2;  // sum g, sum g * xhat
  const T* __restrict__ x;
  const T* __restrict__ dy;
  const float* __restrict__ mean;
  const float* __restrict__ invstd;
  const float* __restrict__ gamma;
  const float* __restrict__ beta;
  int C, G;
  int64_t hw;
  FastDiv fd_cg;

  template <int V>
  __device__ __forceinline__ GnCtx<V> begin(int seg, int c) const {
    GnCtx<V> k;
    gn_group_stats<V>(mean, invstd, seg, G, c, fd_cg, k.mv, k.iv);
    gn_params<V>(gamma, beta, c, k.gm, k.bt);
    return k;
  }
  template <int V>
  __device__ __forceinline__ void accum(int seg, int64_t r, int c, float (&acc)[2][V], const GnCtx<V>& k) const {
    float xv[V], gv[V];
    const int64_t at = ((int64_t)seg * hw + r) * C + c;
    ldv<V>(x + at, xv);
    ldv<V>(dy + at, gv);
    gn_mask<RELU>(gv, xv, k.mv, k.iv, k.gm, k.bt);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      acc[0][i] += gv[i];
      acc[1][i] = fmaf(gv[i], (xv[i] - k.mv[i]) * k.iv[i], acc[1][i]);
    }
  }
  __device__ __forceinline__ void finalize(int, int, const double (&)[2]) const {}
};

// the reducer's first stage alone (fuse = 0, no finalize launch): part[n][z][o][c], z < pl.S
template <class Op>
int gn_reduce_launch(const Op& op, const SegPlan& pl, int N, int64_t hw, int C, float* part, hipStream_t st, const char* name) {
  const size_t lds = (size_t)256 * Op::NOUT * pl.V * sizeof(float);
  const dim3 grid((unsigned)pl.gx, (unsigned)N, (unsigned)pl.S), block((unsigned)pl.TX, (unsigned)pl.TY);
  if (pl.V == 8) hipLaunchKernelGGL((seg_reduce_kernel<Op, 8>), grid, block, lds, st, op, hw, C, pl.S, part, (unsigned*)nullptr, 0);
  else if (pl.V == 4) hipLaunchKernelGGL((seg_reduce_kernel<Op, 4>), grid, block, lds, st, op, hw, C, pl.S, part, (unsigned*)nullptr, 0);
  else hipLaunchKernelGGL((seg_reduce_kernel<Op, 1>), grid, block, lds, st, op, hw, C, pl.S, part, (unsigned*)nullptr, 0);
  SG_LAUNCH_CHECK(name);
  return 0;
}

// ---- launch 2: the folds.  One 256-thread workgroup per (group, image): cw lanes along the group's channels (consecutive
// addresses of a partial row), 256 / cw lanes along the S partial rows.  For each tile of cw channels every lane adds its rows
// z = zl, zl + ZL, .. in fp64, the ZL lane sums of a channel are added in lane order through LDS by the channel's first lane,
// which folds the channel into its running group value; at the end lane 0 folds the cw running values in lane order.
__device__ __forceinline__ void gn_channel_totals(const float* __restrict__ part, int n, int c, int C, int S, int zl, int ZL,
                                                  bool act, double& s0, double& s1) {
  s0 = 0.0;
  s1 = 0.0;
  if (act) {
#pragma unroll 4
    for (int z = zl; z < S; z += ZL) {
      const float* p = part + (((int64_t)n * S + z) * 2) * C + c;
      s0 += (double)p[0];
      s1 += (double)p[C];
    }
  }
}
// red: [256][2] doubles; returns the totals to the lanes with zl == 0
__device__ __forceinline__ void gn_lane_sum(double* red, int tid, int tx, int cw, int ZL, int zl, double& s0, double& s1) {
  __syncthreads();  // the previous tile's reads are over
  red[tid * 2] = s0;
  red[tid * 2 + 1] = s1;
  __syncthreads();
  if (zl == 0) {
    double t0 = red[tx * 2], t1 = red[tx * 2 + 1];
    for (int l = 1; l < ZL; ++l) {
      t0 += red[(l * cw + tx) * 2];
      t1 += red[(l * cw + tx) * 2 + 1];
    }
    s0 = t0;
    s1 = t1;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void gn_fold_stats_kernel(const T* __restrict__ x, const float* __restrict__ part,
                                                            float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                            int64_t hw, int C, int G, int S, int cw, float eps) {
  __shared__ double red[256 * 2];
  __shared__ double run[64 * 3];
  const int g = blockIdx.x, n = blockIdx.y, Cg = C / G;
  const int tid = threadIdx.x, tx = tid % cw, zl = tid / cw, ZL = 256 / cw;
  const double cnt1 = (double)hw;
  double cnt = 0.0, mean = 0.0, m2 = 0.0;   // this lane's channels so far (zl == 0)
  for (int j0 = 0; j0 < Cg; j0 += cw) {
    const bool act = j0 + tx < Cg;
    const int c = g * Cg + j0 + tx;
    double s0, s1;
    gn_channel_totals(part, n, c, C, S, zl, ZL, act, s0, s1);
    gn_lane_sum(red, tid, tx, cw, ZL, zl, s0, s1);
    if (zl == 0 && act) {
      const double d1 = s0 / cnt1;
      const double mc = (double)ld1<T>(x + (int64_t)n * hw * C + c) + d1;
      double m2c = s1 - s0 * d1;
      if (m2c < 0.0) m2c = 0.0;
      const double tot = cnt + cnt1, delta = mc - mean;   // Chan et al.: two sets with their own means
      mean += delta * (cnt1 / tot);
      m2 += m2c + delta * delta * (cnt * cnt1 / tot);
      cnt = tot;
    }
  }
  if (zl == 0) {
    run[tx * 3] = cnt;
    run[tx * 3 + 1] = mean;
    run[tx * 3 + 2] = m2;
  }
  __syncthreads();
  if (tid == 0) {
    for (int l = 1; l < cw; ++l) {
      const double cb = run[l * 3], mb = run[l * 3 + 1], vb = run[l * 3 + 2];
      if (cb > 0.0) {
        const double tot = cnt + cb, delta = mb - mean;
        mean += delta * (cb / tot);
        m2 += vb + delta * delta * (cnt * cb / tot);
        cnt = tot;
      }
    }
    double var = m2 / cnt;   // biased
    if (var < 0.0) var = 0.0;
    save_mean[(int64_t)n * G + g] = (float)mean;
    save_invstd[(int64_t)n * G + g] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// tot: [N][C][2] doubles (S1, S2), ab: [N * G][2] floats (A / m, B / m)
__global__ __launch_bounds__(256) void gn_fold_bwd_kernel(const float* __restrict__ part, const float* __restrict__ gamma,
                                                          double* __restrict__ tot, float* __restrict__ ab, int64_t hw, int C, int G,
                                                          int S, int cw) {
  __shared__ double red[256 * 2];
  __shared__ double run[64 * 2];
  const int g = blockIdx.x, n = blockIdx.y, Cg = C / G;
  const int tid = threadIdx.x, tx = tid % cw, zl = tid / cw, ZL = 256 / cw;
  double a = 0.0, b = 0.0;
  for (int j0 = 0; j0 < Cg; j0 += cw) {
    const bool act = j0 + tx < Cg;
    const int c = g * Cg + j0 + tx;
    double s0, s1;
    gn_channel_totals(part, n, c, C, S, zl, ZL, act, s0, s1);
    gn_lane_sum(red, tid, tx, cw, ZL, zl, s0, s1);
    if (zl == 0 && act) {
      double* t = tot + ((int64_t)n * C + c) * 2;
      t[0] = s0;
      t[1] = s1;
      const double gm = gamma ? (double)gamma[c] : 1.0;
      a += gm * s0;
      b += gm * s1;
    }
  }
  if (zl == 0) {
    run[tx * 2] = a;
    run[tx * 2 + 1] = b;
  }
  __syncthreads();
  if (tid == 0) {
    for (int l = 1; l < cw; ++l) {
      a += run[l * 2];
      b += run[l * 2 + 1];
    }
    const double m = (double)hw * (double)Cg;
    ab[((int64_t)n * G + g) * 2] = (float)(a / m);
    ab[((int64_t)n * G + g) * 2 + 1] = (float)(b / m);
  }
}

// ---- launch 3: the apply kernels, column-stationary within an image (as bn_apply_cols_kernel): the number of threads of a
// period (gridDim.x * 256) is a multiple of the chunks per row, so a thread's chunk of V channels never changes and its
// constants are loaded once.  blockIdx.x: block within a period of prow whole rows; blockIdx.y: row group; blockIdx.z: image.
template <int V, typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, T* __restrict__ y, int64_t hw, int C, int G,
                                                       int relu, int prow, FastDiv fd_cv, FastDiv fd_cg) {
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, cv = (uint32_t)(C / V);
  const uint32_t r0 = fd_div(i0, fd_cv);
  const int c = (int)(i0 - r0 * cv) * V, n = blockIdx.z;
  GnCtx<V> k;
  gn_group_stats<V>(mean, invstd, n, G, c, fd_cg, k.mv, k.iv);
  gn_params<V>(gamma, beta, c, k.gm, k.bt);
  const T* __restrict__ xn = x + (int64_t)n * hw * C + c;
  T* __restrict__ yn = y + (int64_t)n * hw * C + c;
  auto one = [&](const float (&xv)[V], int64_t r) {
    float o[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float t = gn_affine(xv[i], k.mv[i], k.iv[i], k.gm[i], k.bt[i]);
      if (relu) t = fmaxf(t, 0.f);
      o[i] = t;
    }
    stv<V>(yn + r * C, o);
  };
  const int64_t stride = prow, gstep = (int64_t)gridDim.y * 4 * prow;
  for (int64_t r = (int64_t)blockIdx.y * 4 * prow + r0; r < hw; r += gstep) {
    if (r + 3 * stride < hw) {   // four independent 16-byte loads in flight
      float x0[V], x1[V], x2[V], x3[V];
      ldv<V>(xn + r * C, x0);
      ldv<V>(xn + (r + stride) * C, x1);
      ldv<V>(xn + (r + 2 * stride) * C, x2);
      ldv<V>(xn + (r + 3 * stride) * C, x3);
      one(x0, r); one(x1, r + stride); one(x2, r + 2 * stride); one(x3, r + 3 * stride);
    } else {
      for (int64_t q = r; q < hw; q += stride) {
        float x0[V];
        ldv<V>(xn + q * C, x0);
        one(x0, q);
      }
    }
  }
}

template <int V, typename T, int RELU>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ ab, const double* __restrict__ tot,
                                                           T* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           int N, int64_t hw, int C, int G, int prow, int b0, FastDiv fd_cv,
                                                           FastDiv fd_cg) {
  if ((int)blockIdx.x >= b0) {   // the trailing workgroups: dgamma_c = sum_n S2, dbeta_c = sum_n S1, n ascending, in fp64
    const int c = ((int)blockIdx.x - b0) * 256 + (int)threadIdx.x;
    if (blockIdx.y != 0 || blockIdx.z != 0 || c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int n = 0; n < N; ++n) {
      const double* t = tot + ((int64_t)n * C + c) * 2;
      s1 += t[0];
      s2 += t[1];
    }
    if (dbeta) dbeta[c] = (float)s1;
    if (dgamma) dgamma[c] = (float)s2;
    return;
  }
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, cv = (uint32_t)(C / V);
  const uint32_t r0 = fd_div(i0, fd_cv);
  const int c = (int)(i0 - r0 * cv) * V, n = blockIdx.z;
  GnCtx<V> k;
  float am[V], bm[V];
  gn_group_stats<V>(mean, invstd, n, G, c, fd_cg, k.mv, k.iv);
  gn_params<V>(gamma, beta, c, k.gm, k.bt);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int64_t q = (int64_t)n * G + fd_div((uint32_t)(c + i), fd_cg);
    am[i] = ab[q * 2];
    bm[i] = ab[q * 2 + 1];
  }
  const T* __restrict__ xn = x + (int64_t)n * hw * C + c;
  const T* __restrict__ gn = dy + (int64_t)n * hw * C + c;
  T* __restrict__ dn = dx + (int64_t)n * hw * C + c;
  auto one = [&](const float (&xv)[V], float (&gv)[V], int64_t r) {
    float o[V];
    gn_mask<RELU>(gv, xv, k.mv, k.iv, k.gm, k.bt);
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = gn_dx(xv[i], gv[i], k.mv[i], k.iv[i], k.gm[i], am[i], bm[i]);
    stv<V>(dn + r * C, o);
  };
  const int64_t stride = prow, gstep = (int64_t)gridDim.y * 2 * prow;
  for (int64_t r = (int64_t)blockIdx.y * 2 * prow + r0; r < hw; r += gstep) {
    if (r + stride < hw) {
      float x0[V], x1[V], g0[V], g1[V];
      ldv<V>(xn + r * C, x0);
      ldv<V>(xn + (r + stride) * C, x1);
      ldv<V>(gn + r * C, g0);
      ldv<V>(gn + (r + stride) * C, g1);
      one(x0, g0, r);
      one(x1, g1, r + stride);
    } else {
      float x0[V], g0[V];
      ldv<V>(xn + r * C, x0);
      ldv<V>(gn + r * C, g0);
      one(x0, g0, r);
    }
  }
}

// ---- the plan: a pure function of (CU count, storage type, N, HW, C, G, operands aligned); the entry points launch from it and
// sg_gn_ws_bytes adds its bytes up
struct GnPlan {
  int V;            // channels per lane of the apply kernels
  int prow, b0;     // rows per period, blocks per period
  int gy_fwd, gy_bwd;
  int cw;           // the folds' lanes along a group's channels
  SegPlan seg;
  size_t part_bytes, tot_off, ab_off, fwd_bytes, bwd_bytes;
};

inline int gn_row_groups(int num_cus, int N, int64_t hw, int prow, int b0, int unroll) {
  int64_t k = sg_cdiv((int64_t)8 * num_cus, (int64_t)b0 * N);
  const int64_t maxk = sg_cdiv(hw, (int64_t)unroll * prow);
  if (k > maxk) k = maxk;
  if (k > 65535) k = 65535;
  if (k < 1) k = 1;
  return (int)k;
}

inline GnPlan plan_gn(int num_cus, int dtype, int N, int64_t hw, int C, int G, bool aligned) {
  GnPlan pl = {};
  const bool vec = aligned && C % 4 == 0;
  pl.V = (vec && dtype == SG_BF16 && C % 8 == 0) ? 8 : (vec ? 4 : 1);
  int g = 256, a = C / pl.V;
  while (a) { const int t_ = g % a; g = a; a = t_; }   // gcd(256, chunks per row)
  pl.prow = 256 / g;
  pl.b0 = (C / pl.V) / g;
  pl.gy_fwd = gn_row_groups(num_cus, N, hw, pl.prow, pl.b0, 4);
  pl.gy_bwd = gn_row_groups(num_cus, N, hw, pl.prow, pl.b0, 2);
  const int Cg = C / G;
  pl.cw = 1;
  while (pl.cw < Cg && pl.cw < 64) pl.cw <<= 1;
  pl.seg = seg_plan<2>(num_cus, N, hw, C, vec, dtype == SG_BF16);
  pl.part_bytes = pl.seg.part_bytes;
  pl.tot_off = (pl.part_bytes + 15) & ~(size_t)15;
  pl.ab_off = pl.tot_off + (size_t)N * C * 2 * sizeof(double);
  pl.fwd_bytes = pl.part_bytes;
  pl.bwd_bytes = pl.ab_off + (size_t)N * G * 2 * sizeof(float);
  return pl;
}

// every entry point's and the query's checks; an image is indexed with 64 bits, the grid carries N in its y / z dimension
inline int gn_check(const sg_ctx* ctx, int dtype, int N, int64_t hw, int C, int G, const char* who) {
  SG_CHECK_ARG(ctx && (dtype == SG_F32 || dtype == SG_BF16), "%s: bad ctx/dtype", who);
  SG_CHECK_ARG(N >= 1 && N <= 65535 && hw >= 1 && C >= 1, "%s: needs 1 <= N <= 65535, HW >= 1, C >= 1", who);
  SG_CHECK_ARG(G >= 1 && C % G == 0, "%s: %d channels do not divide into %d groups", who, C, G);
  SG_CHECK_ARG((double)N * (double)hw * (double)C < 4.0e18, "%s: tensor too large", who);
  return 0;
}

inline int gn_ws_check(const char* who, const void* ws, size_t ws_bytes, size_t need) {
  if (!ws || ws_bytes < need) {
    sg_set_error("%s: workspace %zu < %zu", who, ws_bytes, need);
    return SG_EWORKSPACE;
  }
  SG_CHECK_ARG(sg_aligned16(ws), "%s: the workspace must be 16-byte aligned", who);
  return 0;
}

template <class F>
inline void gn_with_v(int V, F&& fn) {
  if (V == 8) fn(std::integral_constant<int, 8>{});
  else if (V == 4) fn(std::integral_constant<int, 4>{});
  else fn(std::integral_constant<int, 1>{});
}

}  // namespace

extern "C" {

size_t sg_gn_ws_bytes(const sg_ctx* ctx, int dtype, int N, int64_t hw, int C, int G) {
  if (gn_check(ctx, dtype, N, hw, C, G, "sg_gn_ws_bytes")) return 0;
  size_t m = 0;
  for (bool aligned : {false, true}) m = std::max(m, plan_gn(ctx->num_cus, dtype, N, hw, C, G, aligned).bwd_bytes);
  return m;
}

int sg_gn_fwd(sg_ctx* ctx, void* stream, int dtype, int N, int64_t hw, int C, int G, const void* x, const void* gamma,
              const void* beta, void* y, void* save_mean, void* save_invstd, float eps, int relu, void* ws, size_t ws_bytes) {
  if (int e = gn_check(ctx, dtype, N, hw, C, G, "sg_gn_fwd")) return e;
  SG_CHECK_ARG(x && y && save_mean && save_invstd, "sg_gn_fwd: bad argument");
  const GnPlan pl = plan_gn(ctx->num_cus, dtype, N, hw, C, G, sg_all_aligned16({x, y, gamma, beta}));
  if (int e = gn_ws_check("sg_gn_fwd", ws, ws_bytes, pl.fwd_bytes)) return e;
  const hipStream_t st = (hipStream_t)stream;
  const FastDiv fd_cv = make_fastdiv((uint32_t)(C / pl.V)), fd_cg = make_fastdiv((uint32_t)(C / G));
  SG_DTYPE_SWITCH(dtype, "sg_gn_fwd", {
    const GnStatsOp<T> op = {(const T*)x, C, hw};
    if (int e = gn_reduce_launch(op, pl.seg, N, hw, C, (float*)ws, st, "gn_stats")) return e;
    hipLaunchKernelGGL((gn_fold_stats_kernel<T>), dim3((unsigned)G, (unsigned)N), dim3(256), 0, st, (const T*)x, (const float*)ws,
                       (float*)save_mean, (float*)save_invstd, hw, C, G, pl.seg.S, pl.cw, eps);
    SG_LAUNCH_CHECK("gn_fold_stats_kernel");
    gn_with_v(pl.V, [&](auto v) {
      constexpr int V = decltype(v)::value;
      hipLaunchKernelGGL((gn_apply_kernel<V, T>), dim3((unsigned)pl.b0, (unsigned)pl.gy_fwd, (unsigned)N), dim3(256), 0, st,
                         (const T*)x, (const float*)save_mean, (const float*)save_invstd, (const float*)gamma, (const float*)beta,
                         (T*)y, hw, C, G, relu, pl.prow, fd_cv, fd_cg);
    });
    SG_LAUNCH_CHECK("gn_apply_kernel");
  });
  return 0;
}

int sg_gn_bwd(sg_ctx* ctx, void* stream, int dtype, int N, int64_t hw, int C, int G, const void* x, const void* dy,
              const void* gamma, const void* beta, const void* save_mean, const void* save_invstd, void* dx, void* dgamma,
              void* dbeta, int relu, void* ws, size_t ws_bytes) {
  if (int e = gn_check(ctx, dtype, N, hw, C, G, "sg_gn_bwd")) return e;
  SG_CHECK_ARG(x && dy && save_mean && save_invstd && dx, "sg_gn_bwd: bad argument");
  SG_CHECK_ARG((gamma || !dgamma) && (beta || !dbeta), "sg_gn_bwd: a gradient without its parameter");
  const GnPlan pl = plan_gn(ctx->num_cus, dtype, N, hw, C, G, sg_all_aligned16({x, dy, dx, gamma, beta}));
  if (int e = gn_ws_check("sg_gn_bwd", ws, ws_bytes, pl.bwd_bytes)) return e;
  const hipStream_t st = (hipStream_t)stream;
  const FastDiv fd_cv = make_fastdiv((uint32_t)(C / pl.V)), fd_cg = make_fastdiv((uint32_t)(C / G));
  float* part = (float*)ws;
  double* tot = (double*)((char*)ws + pl.tot_off);
  float* ab = (float*)((char*)ws + pl.ab_off);
  const unsigned tail = (unsigned)sg_cdiv(C, 256);
  auto run = [&](auto tp, auto m) -> int {
    typedef typename decltype(tp)::type T;
    constexpr int RELU = decltype(m)::value;
    const GnBwdOp<T, RELU> op = {(const T*)x, (const T*)dy, (const float*)save_mean, (const float*)save_invstd, (const float*)gamma,
                                 (const float*)beta, C, G, hw, fd_cg};
    if (int e = gn_reduce_launch(op, pl.seg, N, hw, C, part, st, "gn_bwd_reduce")) return e;
    hipLaunchKernelGGL(gn_fold_bwd_kernel, dim3((unsigned)G, (unsigned)N), dim3(256), 0, st, (const float*)part, (const float*)gamma,
                       tot, ab, hw, C, G, pl.seg.S, pl.cw);
    SG_LAUNCH_CHECK("gn_fold_bwd_kernel");
    gn_with_v(pl.V, [&](auto v) {
      constexpr int V = decltype(v)::value;
      hipLaunchKernelGGL((gn_bwd_apply_kernel<V, T, RELU>), dim3((unsigned)pl.b0 + tail, (unsigned)pl.gy_bwd, (unsigned)N), dim3(256),
                         0, st, (const T*)x, (const T*)dy, (const float*)save_mean, (const float*)save_invstd, (const float*)gamma,
                         (const float*)beta, (const float*)ab, (const double*)tot, (T*)dx, (float*)dgamma, (float*)dbeta, N, hw, C, G,
                         pl.prow, pl.b0, fd_cv, fd_cg);
    });
    SG_LAUNCH_CHECK("gn_bwd_apply_kernel");
    return 0;
  };
  SG_DTYPE_SWITCH(dtype, "sg_gn_bwd", {
    struct Tp { typedef T type; };
    return relu ? run(Tp{}, std::integral_constant<int, 1>{}) : run(Tp{}, std::integral_constant<int, 0>{});
  });
  return 0;
}

}  // extern "C"
