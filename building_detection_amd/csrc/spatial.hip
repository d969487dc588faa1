// The depthwise convolution (SeparableConv2D's first half), HBM-bound (NHWC, channels innermost so every access is a
// coalesced run of 16-byte channel chunks): forward / dgrad / wgrad and plan_dw(), which chooses their kernels.  Pooling
// and up-sampling are in resample.hip.
#include <algorithm>
#include <initializer_list>
#include "sg_reduce.h"

namespace {

constexpr int64_t EW_CAP = 16384;   // ew_blocks: workgroups of this file's element-wise launches

template <typename T>
struct DwParams {
  const T* __restrict__ x;       // forward input (or mask source for dgrad)
  const float* __restrict__ w;   // [KH][KW][C] (fp32 master weights whatever the activation storage)
  const T* __restrict__ dy;
  T* __restrict__ out;
  int N, H, W, C, Ho, Wo, KH, KW, stride, dil, pad_t, pad_l, x_ld, y_ld, pre_relu;
  FastDiv fd_cv, fd_w, fd_h;  // decomposition of the flat index: channel chunk, then width, then height
};

// y[n,oh,ow,c] = sum_taps relu?(x[n, oh*s - pt + kh*d, ow*s - pl + kw*d, c]) * w[kh,kw,c]
template <int V, typename T>
__global__ void dw_fwd_kernel(const DwParams<T> p) {
  const uint32_t cv = p.C / V;
  const uint32_t total = (uint32_t)((int64_t)p.N * p.Ho * p.Wo * cv), stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    uint32_t pix, cc, row, ow, n, oh;
    fd_divmod(i, p.fd_cv, pix, cc);
    fd_divmod(pix, p.fd_w, row, ow);
    fd_divmod(row, p.fd_h, n, oh);
    const int c = (int)cc * V;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int kh = 0; kh < p.KH; ++kh) {
      const int ih = (int)oh * p.stride - p.pad_t + kh * p.dil;
      if ((unsigned)ih >= (unsigned)p.H) continue;
      for (int kw = 0; kw < p.KW; ++kw) {
        const int iw = (int)ow * p.stride - p.pad_l + kw * p.dil;
        if ((unsigned)iw >= (unsigned)p.W) continue;
        float xv[V], wv[V];
        ldv<V>(p.x + ((int64_t)(n * p.H + ih) * p.W + iw) * p.x_ld + c, xv);
        ldv<V>(p.w + (kh * p.KW + kw) * p.C + c, wv);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = fmaf(p.pre_relu ? fmaxf(xv[k], 0.f) : xv[k], wv[k], acc[k]);
      }
    }
    stv<V>(p.out + (int64_t)pix * p.y_ld + c, acc);
  }
}

// dx[n,ih,iw,c] = sum_taps dy[n,(ih+pt-kh*d)/s,(iw+pl-kw*d)/s,c] * w[kh,kw,c]   (* [x>0] if pre_relu)
template <int V, typename T>
__global__ void dw_dgrad_kernel(const DwParams<T> p) {
  const uint32_t cv = p.C / V;
  const uint32_t total = (uint32_t)((int64_t)p.N * p.H * p.W * cv), stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    uint32_t pix, cc, row, iw, n, ih;
    fd_divmod(i, p.fd_cv, pix, cc);
    fd_divmod(pix, p.fd_w, row, iw);
    fd_divmod(row, p.fd_h, n, ih);
    const int c = (int)cc * V;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int kh = 0; kh < p.KH; ++kh) {
      int oh = (int)ih + p.pad_t - kh * p.dil;
      if (oh < 0 || oh % p.stride) continue;
      oh /= p.stride;
      if (oh >= p.Ho) continue;
      for (int kw = 0; kw < p.KW; ++kw) {
        int ow = (int)iw + p.pad_l - kw * p.dil;
        if (ow < 0 || ow % p.stride) continue;
        ow /= p.stride;
        if (ow >= p.Wo) continue;
        float gv[V], wv[V];
        ldv<V>(p.dy + ((int64_t)(n * p.Ho + oh) * p.Wo + ow) * p.y_ld + c, gv);
        ldv<V>(p.w + (kh * p.KW + kw) * p.C + c, wv);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = fmaf(gv[k], wv[k], acc[k]);
      }
    }
    if (p.pre_relu) {
      float xv[V];
      ldv<V>(p.x + (int64_t)pix * p.x_ld + c, xv);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = xv[k] > 0.f ? acc[k] : 0.f;
    }
    stv<V>(p.out + (int64_t)pix * p.x_ld + c, acc);
  }
}

// dw[kh,kw,c] = sum_{n,oh,ow} relu?(x[n,ih,iw,c]) * dy[n,oh,ow,c]  — 9 outputs per channel
template <typename T>
struct DwWgradOp {
  static constexpr int NOUT = 9;
  const T* __restrict__ x;
  const T* __restrict__ dy;
  float* dw;
  int H, W, C, Ho, Wo, stride, dil, pad_t, pad_l, x_ld, y_ld, pre_relu;
  FastDiv fd_w, fd_h;
  template <int V>
  __device__ __forceinline__ void accum(int, int64_t r, int c, float (&acc)[9][V]) const {
    uint32_t row, ow, n, oh;
    fd_divmod((uint32_t)r, fd_w, row, ow);
    fd_divmod(row, fd_h, n, oh);
    float gv[V];
    ldv<V>(dy + r * y_ld + c, gv);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = (int)oh * stride - pad_t + kh * dil;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = (int)ow * stride - pad_l + kw * dil;
        // branch-free: a tap outside the image loads pixel (0, 0) of the image and is dropped by a select (nine loads in flight)
        const bool ok = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
        float xv[V];
        ldv<V>(x + ((int64_t)(n * H + (ok ? ih : 0)) * W + (ok ? iw : 0)) * x_ld + c, xv);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float xr = pre_relu ? fmaxf(xv[k], 0.f) : xv[k];
          const float a = fmaf(xr, gv[k], acc[kh * 3 + kw][k]);
          acc[kh * 3 + kw][k] = ok ? a : acc[kh * 3 + kw][k];
        }
      }
    }
  }
  __device__ __forceinline__ void finalize(int, int c, const double (&s)[9]) const {
#pragma unroll
    for (int t = 0; t < 9; ++t) dw[t * C + c] = (float)s[t];
  }
};

// ---- stride-1 3x3 'same' fast paths: each thread owns one 16-byte channel chunk and a run of 4 output columns,
// so the 3 x 6 input window is loaded once (18 loads for 4 outputs instead of 36) and the 9 kernel taps live in
// registers.  Forward and dgrad are the same stencil (dgrad: kernel flipped, dy as input, optional [x > 0] mask).
template <typename T>
struct DwRunParams {
  const T* __restrict__ in;        // x (fwd) or dy (dgrad)
  const float* __restrict__ w;     // [3][3][C]
  const T* __restrict__ mask;      // dgrad with pre_relu: forward input, else null
  const T* res;                    // dgrad: a gradient already collected for the same tensor, added to the result (may be `out`)
  T* out;
  int N, H, W, C, in_ld, out_ld, mask_ld, relu_in, flip;
  // BN = true kernels: the input is the RAW output of the producing convolution and the preceding training-mode
  // BatchNormalization (+ ReLU) is applied as the window is loaded - fmaf((x - mean) * invstd, gamma, beta), the very
  // expression of bn_apply_kernel - so that normalised tensor is never written or read (sg_dwconv2d_fwd with bn)
  const float* __restrict__ bn_gamma;
  const float* __restrict__ bn_beta;
  const float* __restrict__ bn_mean;
  const float* __restrict__ bn_invstd;
  // SUMS = true kernels (dgrad only): `out` is the gradient of a training-mode BatchNormalization's OUTPUT, whose raw input is
  // bs_x.  Besides writing it the kernel sums, per channel, what that layer's backward needs - sum g and sum g * xhat with
  // g = out [masked by the layer's fused ReLU, recomputed from bs_x as sg_bn_train_bwd does] and xhat = (bs_x - mean) * invstd
  // - into bs_part[blockIdx.y][2][C]: the reduction pass of BatchNormalization's backward (two tensor reads) disappears for
  // one more read here (sg_dwconv2d_dgrad with sums)
  const T* __restrict__ bs_x = nullptr;
  const float* __restrict__ bs_mean = nullptr;
  const float* __restrict__ bs_invstd = nullptr;
  const float* __restrict__ bs_gamma = nullptr;
  const float* __restrict__ bs_beta = nullptr;
  float* bs_part = nullptr;
  int bs_ld = 0, bs_relu = 0;
  int lc;                          // lanes per run along the channels (plan_dw)
  int runs_per_row;                // W / 4
  int64_t nruns;                   // N * H * runs_per_row
  FastDiv fd_rpr, fd_h;
};

// RR output rows per run: the (RR + 2) x 6 input window is loaded once for RR x 4 outputs - 4.5 loads per output
// at RR = 1, 2.25 at RR = 4 (fd_h divides by H / RR then).
// RELU / MASK are compile-time and the window is branch-free (rows and columns outside the image load a valid address
// and are zeroed by a select): with the run-time `if (relu_in)` and the `continue` on the row test every load sat in its
// own basic block behind an s_waitcnt vmcnt(0) - 18..36 serialised memory latencies per run.
// (SUMS: two workgroups per SIMD-row instead of three - its 40 more live registers spilled 150 of them under the 168-register
// cap, 590 bytes of scratch per lane, and the kernel lost more than the reduction pass it replaces costs)
template <int RR, typename T, bool RELU, bool MASK, bool BN = false, bool SUMS = false>
__global__ __launch_bounds__(256, SUMS ? 2 : 3) void dw_s1_run_kernel(const DwRunParams<T> p) {
  // p.lc lanes (a power of two <= 64) cover the channel chunks of one run; with few channels (C = 64: 16 chunks)
  // a wave takes several runs instead of idling three quarters of its lanes
  const int lc = p.lc, rpb = 256 / lc;
  const int c_raw = (blockIdx.x * lc + (threadIdx.x & (lc - 1))) * 4;
  if constexpr (!SUMS) {
    if (c_raw >= p.C) return;
  }
  // SUMS: every thread reaches the workgroup's reduction below; a lane past the last channel chunk walks chunk 0 and drops
  // its results
  const bool live = c_raw < p.C;
  const int c = live ? c_raw : 0;
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  f32x4 bmv, biv, bgm, bbt;
  if constexpr (SUMS) {
    bmv = *reinterpret_cast<const f32x4*>(p.bs_mean + c);
    biv = *reinterpret_cast<const f32x4*>(p.bs_invstd + c);
    bgm = *reinterpret_cast<const f32x4*>(p.bs_gamma + c);
    bbt = *reinterpret_cast<const f32x4*>(p.bs_beta + c);
  }
  f32x4 wt[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const f32x4*>(p.w + (p.flip ? 8 - t : t) * p.C + c);
  f32x4 gm, bt, mv, iv;
  if constexpr (BN) {
    gm = *reinterpret_cast<const f32x4*>(p.bn_gamma + c);
    bt = *reinterpret_cast<const f32x4*>(p.bn_beta + c);
    mv = *reinterpret_cast<const f32x4*>(p.bn_mean + c);
    iv = *reinterpret_cast<const f32x4*>(p.bn_invstd + c);
  }
  const int64_t stride = (int64_t)gridDim.y * rpb;
  for (int64_t run = (int64_t)blockIdx.y * rpb + threadIdx.x / lc; run < p.nruns; run += stride) {
    uint32_t rowi, q, n, ohb;
    fd_divmod((uint32_t)run, p.fd_rpr, rowi, q);
    fd_divmod(rowi, p.fd_h, n, ohb);
    const int ow0 = (int)q * 4, oh0 = (int)ohb * RR;
    const bool lok = ow0 > 0, rok = ow0 + 4 < p.W;   // the window's first / last column lies inside the image
    f32x4 acc[RR][4];
#pragma unroll
    for (int rr = 0; rr < RR; ++rr)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[rr][k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < RR + 2; ++a) {
      const int ih = oh0 - 1 + a;
      const bool rowok = (a >= 1 && a <= RR) || (unsigned)ih < (unsigned)p.H;  // the RR middle rows always are
      const T* rowp = p.in + ((int64_t)(n * p.H + (rowok ? ih : oh0)) * p.W + ow0) * p.in_ld + c;
      f32x4 v[6];
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const bool ok = rowok && (b == 0 ? lok : (b == 5 ? rok : true));
        const int db = (b == 0 && !lok) ? 0 : ((b == 5 && !rok) ? 3 : b - 1);   // a valid column when masked
        f32x4 t = ld4<T>(rowp + (int64_t)db * p.in_ld);
        if constexpr (BN) {
#pragma unroll
          for (int e = 0; e < 4; ++e) t[e] = fmaf((t[e] - mv[e]) * iv[e], gm[e], bt[e]);
        }
        v[b] = ok ? t : f32x4{0.f, 0.f, 0.f, 0.f};   // zero padding of the NORMALISED tensor
        if constexpr (RELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[b][e] = fmaxf(v[b][e], 0.f);
        }
      }
      // input row a feeds output row rr = a - ta through kernel row ta (0..2)
#pragma unroll
      for (int ta = 0; ta < 3; ++ta) {
        const int rr = a - ta;
        if (rr < 0 || rr >= RR) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int b = 0; b < 3; ++b) acc[rr][k] += v[k + b] * wt[ta * 3 + b];
      }
    }
#pragma unroll
    for (int rr = 0; rr < RR; ++rr) {
      const int64_t opix = ((int64_t)(n * p.H + oh0 + rr) * p.W + ow0);
      f32x4 m[4], bx[4];
      if constexpr (MASK) {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = ld4<T>(p.mask + (opix + k) * p.mask_ld + c);
      }
      if constexpr (SUMS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) bx[k] = ld4<T>(p.bs_x + (opix + k) * p.bs_ld + c);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        f32x4 o = acc[rr][k];
        if constexpr (MASK) {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = m[k][e] > 0.f ? o[e] : 0.f;
        }
        if (p.res) {   // uniform: the other consumer's gradient of this tensor rides along (sg_dwconv2d_dgrad with res)
          const f32x4 rv = ld4<T>(p.res + (opix + k) * p.out_ld + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += rv[e];
        }
        if constexpr (SUMS) {
          // BnBwdOp's accumulation (norm.hip) on the complete gradient: the fused ReLU's mask from the forward's own fmaf
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float xh = (bx[k][e] - bmv[e]) * biv[e];
            const bool on = !p.bs_relu || fmaf(xh, bgm[e], bbt[e]) > 0.f;
            const float g = on ? o[e] : 0.f;
            s1[e] += g;
            s2[e] = fmaf(g, xh, s2[e]);
          }
        }
        if (SUMS && !live) continue;
        st4<T>(p.out + (opix + k) * p.out_ld + c, o);
      }
    }
  }
  if constexpr (SUMS) {
    // the run slots of this workgroup (threads that share a channel chunk) are added in slot order; the partial row of this
    // workgroup goes to bs_part[blockIdx.y], the rows are added in fp64 by the finalize launch (fixed order: deterministic)
    __shared__ float red[256 * 8];
    float* mine = red + threadIdx.x * 8;
#pragma unroll
    for (int e = 0; e < 4; ++e) { mine[e] = s1[e]; mine[4 + e] = s2[e]; }
    __syncthreads();
    if ((int)threadIdx.x < lc && live) {
      f32x4 t1 = {0.f, 0.f, 0.f, 0.f}, t2 = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < rpb; ++j) {
        const float* q = red + (j * lc + threadIdx.x) * 8;
#pragma unroll
        for (int e = 0; e < 4; ++e) { t1[e] += q[e]; t2[e] += q[4 + e]; }
      }
      float* row = p.bs_part + (int64_t)blockIdx.y * 2 * p.C + c;
      *reinterpret_cast<f32x4*>(row) = t1;
      *reinterpret_cast<f32x4*>(row + p.C) = t2;
    }
  }
}

// wgrad, same window: a "row" of the segmented reducer is a run of RR rows x 4 output pixels.  Branch-free like the
// stencil above (PRE compile-time, rows / columns outside the image masked by a select): 22 loads of a run in flight
// together instead of one at a time.
// BN: x is the raw output of the producing convolution; the training-mode BatchNormalization (+ ReLU, PRE) in front of this
// depthwise convolution is applied on load with bn_apply_kernel's expression (sg_dwconv2d_wgrad with bn), its four per-channel
// parameters loaded once per thread (the reducer's context hook).
template <int V>
struct DwBnCtx {
  float gm[V], bt[V], mv[V], iv[V];
};

template <int RR, typename T, bool PRE, bool BN = false>
struct DwWgradRunOp {
  static constexpr int NOUT = 9;
  const T* __restrict__ x;
  const T* __restrict__ dy;
  float* dw;
  int H, W, C, x_ld, y_ld;
  FastDiv fd_rpr, fd_h;
  const float* __restrict__ bn_gamma;
  const float* __restrict__ bn_beta;
  const float* __restrict__ bn_mean;
  const float* __restrict__ bn_invstd;
  template <int V>
  __device__ __forceinline__ DwBnCtx<V> begin(int, int c) const {
    DwBnCtx<V> k;
    if constexpr (BN) {
      ldv<V>(bn_gamma + c, k.gm);
      ldv<V>(bn_beta + c, k.bt);
      ldv<V>(bn_mean + c, k.mv);
      ldv<V>(bn_invstd + c, k.iv);
    }
    return k;
  }
  template <int V>
  __device__ __forceinline__ void accum(int, int64_t r, int c, float (&acc)[9][V], const DwBnCtx<V>& bn) const {
    if constexpr (V != 4) {
      return;  // the run path is only planned with 16-byte chunks (seg_plan vec_ok = true, C % 4 == 0)
    } else {
    uint32_t rowi, q, n, ohb;
    fd_divmod((uint32_t)r, fd_rpr, rowi, q);
    fd_divmod(rowi, fd_h, n, ohb);
    const int ow0 = (int)q * 4, oh0 = (int)ohb * RR;
    const bool lok = ow0 > 0, rok = ow0 + 4 < W;
    f32x4 g[RR][4];
#pragma unroll
    for (int rr = 0; rr < RR; ++rr) {
      const T* gp = dy + ((int64_t)(n * H + oh0 + rr) * W + ow0) * y_ld + c;
#pragma unroll
      for (int k = 0; k < 4; ++k) g[rr][k] = ld4<T>(gp + (int64_t)k * y_ld);
    }
#pragma unroll
    for (int a = 0; a < RR + 2; ++a) {
      const int ih = oh0 - 1 + a;
      const bool rowok = (a >= 1 && a <= RR) || (unsigned)ih < (unsigned)H;
      const T* rowp = x + ((int64_t)(n * H + (rowok ? ih : oh0)) * W + ow0) * x_ld + c;
      f32x4 v[6];
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const bool ok = rowok && (b == 0 ? lok : (b == 5 ? rok : true));
        const int db = (b == 0 && !lok) ? 0 : ((b == 5 && !rok) ? 3 : b - 1);
        f32x4 t = ld4<T>(rowp + (int64_t)db * x_ld);
        if constexpr (BN) {
#pragma unroll
          for (int e = 0; e < 4; ++e) t[e] = fmaf((t[e] - bn.mv[e]) * bn.iv[e], bn.gm[e], bn.bt[e]);
        }
        v[b] = ok ? t : f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (PRE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[b][e] = fmaxf(v[b][e], 0.f);
        }
      }
#pragma unroll
      for (int ta = 0; ta < 3; ++ta) {
        const int rr = a - ta;  // input row a meets output row rr under kernel row ta
        if (rr < 0 || rr >= RR) continue;
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[ta * 3 + b][e] = fmaf(v[k + b][e], g[rr][k][e], acc[ta * 3 + b][e]);
      }
    }
    }
  }
  __device__ __forceinline__ void finalize(int, int c, const double (&s)[9]) const {
#pragma unroll
    for (int t = 0; t < 9; ++t) dw[t * C + c] = (float)s[t];
  }
};

// wgrad as column strips (round 3; SG_DW_STRIP=0 restores the run reducer above).  The run form loads every x element 4.5
// times and every dy element once per run of 4 pixels (22 loads of 16 bytes for 144 FMAs per lane) and was bound by the
// load issue, not by HBM: 40 us + 8 us finalize for the 95 MB of the 32x32x728 layers (floor 20 us).  Here a lane owns 4
// channels of a strip of 4 columns x HS rows and walks DOWN it with the three x rows of the window in registers: one new
// x row (6 loads) and one dy row (4 loads) per 4 output pixels, both requested one row ahead of their use.  A workgroup is
// 16 channel chunks (256 contiguous bytes per pixel) x 16 strips; the 16 strip partials are added in fixed order through
// LDS, the S workgroup partials by seg_finalize_kernel in fp64 as before (part layout of seg_reduce_kernel, segment 0).
// BN: x is the raw output of the producing convolution and the training-mode BatchNormalization (+ ReLU = PRE) in front of
// this depthwise convolution is applied where a row is consumed, with bn_apply_kernel's expression (SG_BN_DEFER, as
// DwWgradRunOp<.., BN = true>); the zero padding then has to be put back by masks, since BN(0) != 0.
// (BN: held to two waves per SIMD - left to itself the variant takes a few registers more than 256, i.e. ONE wave per SIMD,
// and ran 110 us where the plain kernel takes 50 (profiles/r04_bench_kernel_stats_final.csv))
// OCC2: two waves per SIMD with 12 - 62 spilled registers; measured a loss and no longer instantiated (retired) -
// the parameter stays, it is part of the kernel's name
template <typename T, bool PRE, bool BN, bool OCC2 = false>
__global__ __launch_bounds__(256, OCC2 ? 2 : 1) __attribute__((amdgpu_waves_per_eu(1, 2))) void dw_wgrad_strip_kernel(
    const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part, const int H, const int W, const int C,
    const int x_ld, const int y_ld, const int HS, const int nstrips, const int S, const unsigned x_bytes, const unsigned y_bytes,
    const FastDiv fd_q, const FastDiv fd_hs, const float* __restrict__ bn_gamma, const float* __restrict__ bn_beta,
    const float* __restrict__ bn_mean, const float* __restrict__ bn_invstd) {
  constexpr int TX = 16, TY = 16, EB = (int)sizeof(T);
  constexpr unsigned OOB = 0x80000000u;  // beyond num_records: the hardware returns 0 (image border, no select, no branch)
  typedef typename std::conditional<EB == 4, u32x4_c, u32x2_c>::type raw_t;
  __shared__ float red[TY][TX][36];
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> 4;
  const int c = (blockIdx.x * TX + tx) * 4;
  const int z = blockIdx.y;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = zero;
  const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x), 0, (int)x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(dy), 0, (int)y_bytes, 0x00020000);
  auto ldraw = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned off) -> raw_t {
    if constexpr (EB == 4) return __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
    else return __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, 0);
  };
  // the registers a load fills are touched only where the row is consumed (widening, ReLU): anything done to them at the
  // load would wait for it
  auto widen = [&](const raw_t r, const bool relu) -> f32x4 {
    f32x4 o;
    if constexpr (EB == 4) {
      o = __builtin_bit_cast(f32x4, r);
    } else {
      o = (f32x4){__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16),
                  __uint_as_float(r[1] & 0xffff0000u)};
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
    }
    return o;
  };
  f32x4 gm = zero, bt = zero, mv = zero, iv = zero;
  if constexpr (BN) {
    if (c < C) { gm = ld4<float>(bn_gamma + c); bt = ld4<float>(bn_beta + c); mv = ld4<float>(bn_mean + c); iv = ld4<float>(bn_invstd + c); }
  }
  if (c < C) {
    for (int s = z * TY + ty; s < nstrips; s += S * TY) {
      uint32_t rowi, q, n, hs;
      fd_divmod((uint32_t)s, fd_q, rowi, q);     // strips of one row band lie side by side: neighbours share their halo columns
      fd_divmod(rowi, fd_hs, n, hs);
      const int ow0 = (int)q * 4, h0 = (int)hs * HS;
      const int h1 = h0 + HS < H ? h0 + HS : H;
      const bool lok = ow0 > 0, rok = ow0 + 4 < W;
      const unsigned xpix0 = ((unsigned)n * H * W + ow0), xrow = (unsigned)W * x_ld * EB, grow = (unsigned)W * y_ld * EB;
      const unsigned xoff0 = (xpix0 * x_ld + c) * EB, goff0 = (xpix0 * y_ld + c) * EB;
      // Offsets are sums, never selects around a load (a select feeding a load became control flow, and with more than one
      // basic block per step the FMAs were sunk out of the steps altogether): a column outside the image adds 2^30, a row
      // outside it sets bit 31 - either way the offset is beyond num_records (< 2^30, dw_wgrad_strips_ok) and the load returns 0.
      unsigned coff[6];
#pragma unroll
      for (int b = 0; b < 6; ++b) coff[b] = (unsigned)((b - 1) * x_ld * EB);
      coff[0] = lok ? coff[0] : 0x40000000u;
      coff[5] = rok ? coff[5] : 0x40000000u;
      auto load_x = [&](int ih, raw_t (&v)[6]) {
        const unsigned flag = (unsigned)ih < (unsigned)H ? 0u : OOB;
        const unsigned ro = xoff0 + (unsigned)ih * xrow;
#pragma unroll
        for (int b = 0; b < 6; ++b) v[b] = ldraw(rsrc_x, (ro + coff[b]) | flag);
      };
      auto load_g = [&](int oh, raw_t (&g)[4]) {
        const unsigned flag = oh < h1 ? 0u : OOB;   // the row behind the strip is never used
        const unsigned ro = goff0 + (unsigned)oh * grow;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = ldraw(rsrc_g, (ro + (unsigned)(k * y_ld * EB)) | flag);
      };
      auto rowmac = [&](const int ta, const raw_t (&vr)[6], const f32x4 (&g)[4], const int ih) {
        f32x4 v[6];
        if constexpr (BN) {
          const bool rowok = (unsigned)ih < (unsigned)H;
#pragma unroll
          for (int b = 0; b < 6; ++b) {
            f32x4 t = widen(vr[b], false);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              t[e] = fmaf((t[e] - mv[e]) * iv[e], gm[e], bt[e]);
              if (PRE) t[e] = fmaxf(t[e], 0.f);
            }
            v[b] = (rowok && (b == 0 ? lok : (b == 5 ? rok : true))) ? t : zero;
          }
        } else {
#pragma unroll
          for (int b = 0; b < 6; ++b) v[b] = widen(vr[b], PRE);
        }
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[ta * 3 + b][e] = fmaf(v[k + b][e], g[k][e], acc[ta * 3 + b][e]);
      };
      // four x-row buffers and two dy-row buffers whose roles rotate with the (unrolled) row step: no register copies - a
      // copy of a row that is still in flight would be a use and wait for it (HS and H are multiples of 4: dw_wgrad_strips_ok)
      raw_t X[4][6], G[2][4];
      load_x(h0 - 1, X[0]);
      load_x(h0, X[1]);
      load_x(h0 + 1, X[2]);
      load_g(h0, G[0]);
      auto step = [&](auto I_, int oh) {
        constexpr int I = decltype(I_)::value;
        load_x(oh + 2, X[(I + 3) & 3]);  // one row ahead: consumed by the next step
        load_g(oh + 1, G[(I + 1) & 1]);
        // Two pins per step, or the FMAs of all four steps end up behind the last step's loads (sched_barrier holds the
        // machine scheduler only) and the loads are sunk to their uses: the rows consumed first in this step pass through an
        // asm statement placed behind this step's loads (memory clobber: the loads stay in front of it), the accumulators
        // through one at the end of the step.
        raw_t (&xc)[6] = X[(I + 2) & 3];
        raw_t (&gc)[4] = G[I & 1];
        asm volatile("" : "+v"(xc[0]), "+v"(xc[1]), "+v"(xc[2]), "+v"(xc[3]), "+v"(xc[4]), "+v"(xc[5]), "+v"(gc[0]), "+v"(gc[1]),
                          "+v"(gc[2]), "+v"(gc[3]) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
        f32x4 g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = widen(gc[k], false);
        rowmac(0, X[I & 3], g, oh - 1);
        rowmac(1, X[(I + 1) & 3], g, oh);
        rowmac(2, xc, g, oh + 1);
        asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]),
                          "+v"(acc[7]), "+v"(acc[8]));
        __builtin_amdgcn_sched_barrier(0);
      };
      for (int oh = h0; oh < h1; oh += 4) {
        step(std::integral_constant<int, 0>{}, oh);
        step(std::integral_constant<int, 1>{}, oh + 1);
        step(std::integral_constant<int, 2>{}, oh + 2);
        step(std::integral_constant<int, 3>{}, oh + 3);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[ty][tx][t * 4 + e] = acc[t][e];
  __syncthreads();
  // 16 x 36 sums of 16 terms: thread (ty, tx) finishes outputs ty, ty + 16, .. of chunk tx, strips added in order 0..15
  if (c < C) {
    for (int o = ty; o < 36; o += TY) {
      float sum = 0.f;
#pragma unroll
      for (int y = 0; y < TY; ++y) sum += red[y][tx][o];
      part[((int64_t)z * 9 + (o >> 2)) * C + c + (o & 3)] = sum;
    }
  }
}

// ---- the stencil as column strips (round 4; maps of 64 rows and more - dw_stencil_strips_ok; SG_DW_FSTRIP=0 restores the run kernel) ------
// dw_s1_run_kernel fetches its window once per run of RR x 4 outputs: 3 loads of 16 bytes per output chunk at RR = 2 (the
// four-row window needs more registers than three workgroups per CU leave), and was measured at 38 us (forward with the
// BatchNormalization in the gather) / 47 us (dgrad with the BatchNormalization sums) on the 47.7 MB middle-flow tensors that a
// copy moves in 20.6 us - load-issue bound like the filter gradient before dw_wgrad_strip_kernel.  Here, as there, a lane owns 4
// channels of a strip of 4 columns x HS rows and walks DOWN it with the window's three input rows in registers (transformed once:
// widening, BatchNormalization, ReLU, the zero padding put back): one new input row (6 loads) per 4 outputs, requested one row
// ahead; the epilogue's operands (ReLU mask, collected gradient, the BatchNormalization's raw input) are requested at the top of
// the step.  Rows and columns outside the image are offsets beyond the buffer descriptor (bit 31 / bit 30): no select in front of
// a load.  Same products in the same order as the run kernel (kernel rows 0..2, columns 0..2, one fp32 accumulator per output):
// bit-identical outputs; the BatchNormalization sums are added in another (fixed) order.
template <typename T>
struct DwStripGeom {
  int HS, nstrips;
  unsigned in_bytes;
  FastDiv fd_q, fd_hs;
};

template <typename T, bool RELU, bool MASK, bool BN, bool SUMS>
__global__ __launch_bounds__(256, 2) void dw_strip_kernel(const DwRunParams<T> p, const DwStripGeom<T> gm_) {
  constexpr int TX = 16, TY = 16, EB = (int)sizeof(T);
  constexpr unsigned OOB = 0x80000000u;
  typedef typename std::conditional<EB == 4, u32x4_c, u32x2_c>::type raw_t;
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> 4;
  const int c_raw = (blockIdx.x * TX + tx) * 4;
  if constexpr (!SUMS) {
    if (c_raw >= p.C) return;
  }
  const bool live = c_raw < p.C;   // SUMS: every thread reaches the reduction; a lane past the last chunk walks chunk 0 and drops its results
  const int c = live ? c_raw : 0;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const __amdgpu_buffer_rsrc_t rsrc_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p.in), 0, (int)gm_.in_bytes, 0x00020000);
  auto ldraw = [&](unsigned off) -> raw_t {
    if constexpr (EB == 4) return __builtin_amdgcn_raw_buffer_load_b128(rsrc_in, (int)off, 0, 0);
    else return __builtin_amdgcn_raw_buffer_load_b64(rsrc_in, (int)off, 0, 0);
  };
  auto widen = [&](const raw_t r) -> f32x4 {
    if constexpr (EB == 4) {
      return __builtin_bit_cast(f32x4, r);
    } else {
      return (f32x4){__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16),
                     __uint_as_float(r[1] & 0xffff0000u)};
    }
  };
  f32x4 wt[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const f32x4*>(p.w + (p.flip ? 8 - t : t) * p.C + c);
  f32x4 gm = zero, bt = zero, mv = zero, iv = zero;
  if constexpr (BN) {
    gm = *reinterpret_cast<const f32x4*>(p.bn_gamma + c);
    bt = *reinterpret_cast<const f32x4*>(p.bn_beta + c);
    mv = *reinterpret_cast<const f32x4*>(p.bn_mean + c);
    iv = *reinterpret_cast<const f32x4*>(p.bn_invstd + c);
  }
  f32x4 s1 = zero, s2 = zero, bmv = zero, biv = zero, bgm = zero, bbt = zero;
  if constexpr (SUMS) {
    bmv = *reinterpret_cast<const f32x4*>(p.bs_mean + c);
    biv = *reinterpret_cast<const f32x4*>(p.bs_invstd + c);
    bgm = *reinterpret_cast<const f32x4*>(p.bs_gamma + c);
    bbt = *reinterpret_cast<const f32x4*>(p.bs_beta + c);
  }
  const int HS = gm_.HS;
  for (int s = blockIdx.y * TY + ty; s < gm_.nstrips; s += gridDim.y * TY) {
    uint32_t rowi, q, n, hs;
    fd_divmod((uint32_t)s, gm_.fd_q, rowi, q);       // strips of one row band lie side by side: neighbours share their halo columns
    fd_divmod(rowi, gm_.fd_hs, n, hs);
    const int ow0 = (int)q * 4, h0 = (int)hs * HS;
    const int h1 = h0 + HS < p.H ? h0 + HS : p.H;
    const bool lok = ow0 > 0, rok = ow0 + 4 < p.W;
    const unsigned pix0 = (unsigned)n * p.H * p.W + ow0, inrow = (unsigned)p.W * p.in_ld * EB;
    const unsigned inoff0 = (pix0 * p.in_ld + c) * EB;
    unsigned coff[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) coff[b] = (unsigned)((b - 1) * p.in_ld * EB);
    coff[0] = lok ? coff[0] : 0x40000000u;
    coff[5] = rok ? coff[5] : 0x40000000u;
    auto load_row = [&](int ih, raw_t (&v)[6]) {
      const unsigned flag = ((unsigned)ih < (unsigned)p.H && ih <= h1) ? 0u : OOB;   // (the row behind the halo is never used)
      const unsigned ro = inoff0 + (unsigned)ih * inrow;
#pragma unroll
      for (int b = 0; b < 6; ++b) v[b] = ldraw((ro + coff[b]) | flag);
    };
    // a raw row -> the six window values the products use (the run kernel's expressions, in its order)
    auto transform = [&](const raw_t (&r)[6], f32x4 (&v)[6], int ih) {
      const bool rowok = (unsigned)ih < (unsigned)p.H;
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        f32x4 t = widen(r[b]);
        if constexpr (BN) {
#pragma unroll
          for (int e = 0; e < 4; ++e) t[e] = fmaf((t[e] - mv[e]) * iv[e], gm[e], bt[e]);
          t = (rowok && (b == 0 ? lok : (b == 5 ? rok : true))) ? t : zero;   // zero padding of the NORMALISED tensor
        }
        if constexpr (RELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) t[e] = fmaxf(t[e], 0.f);
        }
        v[b] = t;
      }
    };
    // V[j]: the three transformed rows of the window, roles rotating with the (unrolled by three) row step; R: the raw row in flight
    f32x4 V[3][6];
    raw_t R[6];
    {
      raw_t r0[6], r1[6];
      load_row(h0 - 1, r0);
      load_row(h0, r1);
      load_row(h0 + 1, R);
      transform(r0, V[0], h0 - 1);
      transform(r1, V[1], h0);
    }
    auto step = [&](auto I_, int oh) {
      constexpr int I = decltype(I_)::value;
      // row oh + 1 has arrived (requested one step ago): transform it into the buffer of row oh - 2, then request row oh + 2 into
      // the same raw registers
      transform(R, V[(I + 2) % 3], oh + 1);
      load_row(oh + 2, R);
      const int64_t opix = (int64_t)(n * p.H + oh) * p.W + ow0;
      f32x4 acc[4] = {zero, zero, zero, zero};
#pragma unroll
      for (int ta = 0; ta < 3; ++ta) {
        const f32x4 (&v)[6] = V[(I + ta) % 3];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int b = 0; b < 3; ++b) acc[k] += v[k + b] * wt[ta * 3 + b];
      }
      // the epilogue in two halves of two output pixels (its operands - ReLU mask, collected gradient, the BatchNormalization's raw
      // input - would hold 48 registers if all four were requested together)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        f32x4 m[2], rv[2], bx[2];
        if constexpr (MASK) {
#pragma unroll
          for (int k = 0; k < 2; ++k) m[k] = ld4<T>(p.mask + (opix + 2 * hf + k) * p.mask_ld + c);
        }
        if (p.res) {   // uniform
#pragma unroll
          for (int k = 0; k < 2; ++k) rv[k] = ld4<T>(p.res + (opix + 2 * hf + k) * p.out_ld + c);
        }
        if constexpr (SUMS) {
#pragma unroll
          for (int k = 0; k < 2; ++k) bx[k] = ld4<T>(p.bs_x + (opix + 2 * hf + k) * p.bs_ld + c);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          f32x4 o = acc[2 * hf + k];
          if constexpr (MASK) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = m[k][e] > 0.f ? o[e] : 0.f;
          }
          if (p.res) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += rv[k][e];
          }
          if constexpr (SUMS) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float xh = (bx[k][e] - bmv[e]) * biv[e];
              const bool on = !p.bs_relu || fmaf(xh, bgm[e], bbt[e]) > 0.f;
              const float g = on ? o[e] : 0.f;
              s1[e] += g;
              s2[e] = fmaf(g, xh, s2[e]);
            }
          }
          if (SUMS && !live) continue;
          st4<T>(p.out + (opix + 2 * hf + k) * p.out_ld + c, o);
        }
      }
    };
    for (int oh = h0; oh < h1; oh += 3) {
      step(std::integral_constant<int, 0>{}, oh);
      if (oh + 1 >= h1) break;
      step(std::integral_constant<int, 1>{}, oh + 1);
      if (oh + 2 >= h1) break;
      step(std::integral_constant<int, 2>{}, oh + 2);
    }
  }
  if constexpr (SUMS) {
    // the 16 strip slots of this workgroup are added in slot order; the partial row of this workgroup goes to
    // bs_part[blockIdx.y], the rows are added in fp64 by the finalize launch (fixed order: deterministic)
    __shared__ float red[256 * 8];
    float* mine = red + threadIdx.x * 8;
#pragma unroll
    for (int e = 0; e < 4; ++e) { mine[e] = s1[e]; mine[4 + e] = s2[e]; }
    __syncthreads();
    if (ty == 0 && live) {
      f32x4 t1 = zero, t2 = zero;
      for (int j = 0; j < TY; ++j) {
        const float* qq = red + (j * TX + tx) * 8;
#pragma unroll
        for (int e = 0; e < 4; ++e) { t1[e] += qq[e]; t2[e] += qq[4 + e]; }
      }
      float* row = p.bs_part + (int64_t)blockIdx.y * 2 * p.C + c;
      *reinterpret_cast<f32x4*>(row) = t1;
      *reinterpret_cast<f32x4*>(row + p.C) = t2;
    }
  }
}

// ---- who chooses the depthwise kernel: plan_dw() --------------------------------------------------------------------------------
// One DwPlan per launch, a pure function of (CU count, element size, descriptor, direction, operands aligned, sums requested) and
// the four SG_DW_* switches.  sg_dwconv2d_fwd / _dgrad / _wgrad refuse, fill their parameters and launch from it, the two workspace
// queries add its bytes up and sg_dwconv2d_plan hands it out (include/segengine.h: sg_dw_plan, the fields), so a query and a launch
// cannot disagree (tests/test_depthwise_variants_gpu.py compares every launch's plan with its own mirror of the rules below).
// The stencil directions and the filter gradient have their own rules where both have one, each set by its own measurement:
//   strip height   stencil: 16 rows from H >= 64 (profiles/r04_dw_fstrip_ab.txt); filter gradient: 16 rows from H >= 128, 8 below
//   1 GiB test     stencil: the INPUT's bytes at the storage's element size (in_ld: x_ld forward, y_ld dgrad); filter gradient: the
//                  larger of x_ld / y_ld at 4 bytes an element whatever the storage
//   grid cap       stencil: 16384 / gx workgroup rows; filter gradient: 4 * num_cus / gx partial rows and at most 256
//   rows per run   stencil: 2; run reducer: 2 only above 32768 pixels (profiles/r01_bw_census.txt)
struct DwPlan : sg_dw_plan { SegPlan seg; };   // seg: the segment reducer's launch where it runs (seg_V .. seg_S are its copy)

constexpr int DW_SUMS_MAX_ROWS = 1024;   // partial rows of the BatchNormalization sums that the finalize launch adds per channel

inline bool dw_run_ok(const sg_conv_desc* d) {
  return d->KH == 3 && d->KW == 3 && d->stride == 1 && d->dilation == 1 && d->pad_t == 1 && d->pad_l == 1 &&
         d->Ho == d->H && d->Wo == d->W && (d->W % 4 == 0) && (d->Cin % 4 == 0);
}

// Rows per run, measured (profiles/r01_bw_census.txt): the stencil kernels take 2 rows; the kernel-gradient reduction loses
// more from the shrinking number of runs than it gains on small maps and takes 2 rows only from 64x64 up (64x64x728:
// 248 -> 157 us).  SG_DW_RR = 1 / 2 forces a value.
// (Four rows per run are gone: the four-row stencil window ran at the 168-register cap with 47 - 73 spilled registers - three
// alternating repetitions on one box: 75.90 -> 75.04 ms per step without it, profiles/r04_ab_runs.txt - and the reduction
// went 51 -> 65 us with it.  DESIGN.md, retired.)
inline int dw_rows_per_run(int H, int64_t pixels, bool wgrad) {
  const int force = sg_switch<SW_DW_RR>();  // A/B switch: 1 or 2
  const bool small = pixels <= 32768;
  const int want = force ? force : (wgrad ? (small ? 1 : 2) : 2);
  return (want >= 2 && H % 2 == 0) ? 2 : 1;
}

// dw_strip_kernel instead of dw_s1_run_kernel (dw_run_ok maps; in_ld: x_ld forward, y_ld dgrad)
inline bool dw_stencil_strips_ok(const sg_conv_desc* d, int in_ld, int esize) {
  // SG_DW_FSTRIP: 0 never, 1 (default) maps of 64 rows and more, 2 every map.  Measured (profiles/r04_dw_fstrip_ab.txt): 64x64x256
  // 34.0 -> 30.7 us, 128x128x128 62.0 -> 54.9, 256x256x64 115.0 -> 106.1 (strips of 16 rows); the 32x32 maps of the middle flow run
  // no faster (27.2 -> 31.8 us alone, +-0.1 ms in the step at any strip height): with 1.4 waves per SIMD the strips are
  // latency-bound there, and the run kernel was not load-issue bound to begin with (76 % of copy speed).
  const int on = sg_switch<SW_DW_FSTRIP>();
  const int64_t pix = (int64_t)d->N * d->H * d->W;
  if (!on || (on == 1 && d->H < 64)) return false;
  // byte offsets are 32-bit buffer offsets in which bit 30 / bit 31 mark a column / row outside the image: inputs below 1 GiB
  return d->H % 4 == 0 && d->W % 4 == 0 && pix * in_ld * (int64_t)esize < (1ll << 30);
}

// dw_wgrad_strip_kernel instead of the run reducer
inline bool dw_wgrad_strips_ok(const sg_conv_desc* d) {
  const int on = sg_switch<SW_DW_STRIP>();
  const int xl = d->x_ld ? d->x_ld : d->Cin, yl = d->y_ld ? d->y_ld : d->Cout;
  const int64_t pix = (int64_t)d->N * d->H * d->W;
  // byte offsets are 32-bit buffer offsets in which bit 30 / bit 31 mark a column / row outside the image: tensors below 1 GiB
  return on && dw_run_ok(d) && d->H % 4 == 0 && pix * (xl > yl ? xl : yl) * 4 < (1ll << 30);
}

// the stencil's grid: gy rows of workgroups over `per_wg` runs / strips each; with sums every row writes one partial row
inline void plan_dw_stencil_grid(DwPlan& pl, int per_wg, bool sums) {
  int64_t gy = sg_cdiv(pl.count, per_wg);
  const int64_t cap = sg_cdiv(16384, pl.gx);
  if (gy > cap) gy = cap;
  if (gy < 1) gy = 1;
  if (sums && gy > DW_SUMS_MAX_ROWS) gy = DW_SUMS_MAX_ROWS;
  pl.gy = (int)gy;
}

inline void plan_dw_stencil_run(DwPlan& pl, const sg_conv_desc* d, bool sums) {
  pl.family = SG_DWK_RUN;
  pl.RR = dw_rows_per_run(d->H, (int64_t)d->N * d->H * d->W, false);
  pl.count = d->N * (d->H / pl.RR) * (d->W / 4);
  pl.lc = 1;
  while (pl.lc < d->Cin / 4 && pl.lc < 64) pl.lc <<= 1;
  pl.gx = (int)sg_cdiv(d->Cin / 4, pl.lc);
  plan_dw_stencil_grid(pl, 256 / pl.lc, sums);
}

inline void plan_dw_stencil_strip(DwPlan& pl, const sg_conv_desc* d, bool sums) {
  const int hs_force = sg_switch<SW_DW_FSTRIP_HS>();
  pl.family = SG_DWK_STRIP;
  pl.HS = hs_force > 0 ? hs_force : (d->H >= 64 ? 16 : (d->H >= 16 ? 8 : d->H));
  if (pl.HS % 4 != 0 || pl.HS > d->H) pl.HS = 4;
  pl.nhs = (int)sg_cdiv(d->H, pl.HS);
  pl.count = d->N * pl.nhs * (d->W / 4);
  pl.gx = (int)sg_cdiv(d->Cin / 4, 16);
  plan_dw_stencil_grid(pl, 16, sums);
}

inline void plan_dw_wgrad_strip(DwPlan& pl, int num_cus, const sg_conv_desc* d) {
  pl.family = SG_DWK_STRIP;
  pl.HS = d->H >= 128 ? 16 : (d->H >= 16 ? 8 : d->H);   // multiples of 4 (dw_wgrad_strips_ok: H % 4 == 0); the last band may be 4 short
  pl.nhs = (int)sg_cdiv(d->H, pl.HS);
  pl.count = d->N * pl.nhs * (d->W / 4);
  pl.gx = (int)sg_cdiv(d->Cin / 4, 16);
  int64_t S = sg_cdiv(pl.count, 16);
  const int64_t cap = sg_cdiv((int64_t)4 * num_cus, pl.gx);
  if (S > cap) S = cap;
  if (S > 256) S = 256;  // few-channel maps: the finalize adds the S partial rows with 4 lanes per channel (1024 rows of a
                         // 64-channel map took longer than the strips themselves); a lane walks several strips instead
  if (S < 1) S = 1;
  pl.S = (int)S;
  pl.ws_bytes = (size_t)pl.S * 9 * d->Cin * sizeof(float);
}

// the filter gradient on the segment reducer: DwWgradOp over the pixels (SG_DWK_GENERIC), DwWgradRunOp over the runs (SG_DWK_RUN)
inline void plan_dw_wgrad_seg(DwPlan& pl, int num_cus, int family, int64_t rows, int C, bool vec) {
  pl.family = family;
  pl.seg = seg_plan<9>(num_cus, 1, rows, C, vec);
  pl.seg_V = pl.seg.V; pl.seg_TX = pl.seg.TX; pl.seg_gx = pl.seg.gx; pl.seg_S = pl.S = pl.seg.S;
  pl.ws_bytes = pl.seg.part_bytes;
}

inline DwPlan plan_dw(int num_cus, int esize, const sg_conv_desc* d, int dir, bool aligned, bool sums) {
  DwPlan pl = {};
  const int C = d->Cin, xl = d->x_ld ? d->x_ld : C, yl = d->y_ld ? d->y_ld : d->Cout;
  const bool vec = aligned && C % 4 == 0 && xl % 4 == 0 && yl % 4 == 0;
  const bool fast = vec && dw_run_ok(d);   // only the stride-1 3x3 kernels on 16-byte chunks take a fused operand
  pl.V = vec ? 4 : 1;
  if (dir == SG_DW_WGRAD) {
    const int64_t rows = (int64_t)d->N * d->Ho * d->Wo;
    pl.bn = fast;
    if (fast && dw_wgrad_strips_ok(d)) {
      plan_dw_wgrad_strip(pl, num_cus, d);
    } else if (fast) {
      pl.RR = dw_rows_per_run(d->H, rows, true);
      pl.count = (int)(rows / (4 * pl.RR));
      plan_dw_wgrad_seg(pl, num_cus, SG_DWK_RUN, pl.count, C, true);
    } else plan_dw_wgrad_seg(pl, num_cus, SG_DWK_GENERIC, rows, C, vec);
    return pl;
  }
  if (dir == SG_DW_FWD) pl.bn = fast;
  else pl.res = pl.sums = fast;
  if (!fast) {
    pl.family = SG_DWK_GENERIC; pl.gy = 1;
    pl.gx = (int)ew_blocks((int64_t)d->N * (dir == SG_DW_FWD ? d->Ho * d->Wo : d->H * d->W) * (C / pl.V), EW_CAP);
  } else if (dw_stencil_strips_ok(d, dir == SG_DW_FWD ? xl : yl, esize)) plan_dw_stencil_strip(pl, d, sums);
  else plan_dw_stencil_run(pl, d, sums);
  if (dir == SG_DW_DGRAD && sums) {
    pl.S = fast ? pl.gy : 0;
    pl.ws_bytes = (size_t)DW_SUMS_MAX_ROWS * 2 * (size_t)C * sizeof(float);   // the row cap, whatever gy: known without the grid
  }
  return pl;
}

// The seven <RELU, MASK, BN, SUMS> forms of the stencil an entry point can ask for, named once: dw_s1_run_kernel<1 | 2> and
// dw_strip_kernel are instantiated for these and no others (the forward never has a mask or sums, the dgrad never relu_in or bn).
enum DwForm { DW_PLAIN, DW_RELU, DW_BN, DW_BN_RELU, DW_MASK, DW_SUMS, DW_MASK_SUMS };
constexpr std::true_type dw_y{};
constexpr std::false_type dw_n{};

template <class F>
inline void dw_with_form(DwForm form, F&& fn) {
  switch (form) {   //                   RELU  MASK  BN    SUMS
    case DW_PLAIN:     return fn(dw_n, dw_n, dw_n, dw_n);
    case DW_RELU:      return fn(dw_y, dw_n, dw_n, dw_n);
    case DW_BN:        return fn(dw_n, dw_n, dw_y, dw_n);
    case DW_BN_RELU:   return fn(dw_y, dw_n, dw_y, dw_n);
    case DW_MASK:      return fn(dw_n, dw_y, dw_n, dw_n);
    case DW_SUMS:      return fn(dw_n, dw_n, dw_n, dw_y);
    case DW_MASK_SUMS: return fn(dw_n, dw_y, dw_n, dw_y);
  }
}

// the four <PRE, BN> forms of the two filter-gradient kernels
template <class F>
inline auto dw_with_pre_bn(bool pre, bool bn, F&& fn) {
  if (bn) return pre ? fn(dw_y, dw_y) : fn(dw_n, dw_y);
  return pre ? fn(dw_y, dw_n) : fn(dw_n, dw_n);
}

// launch what the plan says: dw_s1_run_kernel<RR> or dw_strip_kernel in `form`, on the operands in p and the plan's geometry
template <typename T>
int launch_dw_stencil(const DwPlan& pl, DwForm form, const sg_conv_desc* d, DwRunParams<T> p, hipStream_t st) {
  p.N = d->N; p.H = d->H; p.W = d->W; p.C = d->Cin;
  p.lc = pl.lc; p.runs_per_row = d->W / 4; p.nruns = pl.count;
  p.fd_rpr = make_fastdiv((uint32_t)p.runs_per_row); p.fd_h = make_fastdiv((uint32_t)(pl.RR ? d->H / pl.RR : d->H));
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  DwStripGeom<T> g = {};
  if (pl.family == SG_DWK_STRIP) {
    g.HS = pl.HS; g.nstrips = pl.count;
    g.in_bytes = (unsigned)((int64_t)p.N * p.H * p.W * p.in_ld * (int64_t)sizeof(T));
    g.fd_q = make_fastdiv((uint32_t)(p.W / 4)); g.fd_hs = make_fastdiv((uint32_t)pl.nhs);
  }
  dw_with_form(form, [&](auto relu, auto mask, auto bn, auto sums) {
    constexpr bool RELU = decltype(relu)::value, MASK = decltype(mask)::value, BN = decltype(bn)::value, SUMS = decltype(sums)::value;
    if (pl.family == SG_DWK_STRIP) hipLaunchKernelGGL((dw_strip_kernel<T, RELU, MASK, BN, SUMS>), grid, dim3(256), 0, st, p, g);
    else if (pl.RR == 2) hipLaunchKernelGGL((dw_s1_run_kernel<2, T, RELU, MASK, BN, SUMS>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dw_s1_run_kernel<1, T, RELU, MASK, BN, SUMS>), grid, dim3(256), 0, st, p);
  });
  SG_LAUNCH_CHECK(pl.family == SG_DWK_STRIP ? "dw_strip_kernel" : "dw_s1_run_kernel");
  return 0;
}

int dw_check(const sg_ctx* ctx, int dtype, const sg_conv_desc* d, const char* who) {
  SG_CHECK_ARG(ctx && (dtype == SG_F32 || dtype == SG_BF16) && d, "%s: bad ctx/dtype/desc", who);
  SG_CHECK_ARG(d->Cin == d->Cout, "%s: depthwise needs Cin == Cout (depth_multiplier 1)", who);
  SG_CHECK_ARG(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Ho > 0 && d->Wo > 0 && d->KH > 0 && d->KW > 0 &&
                   d->stride > 0 && d->dilation > 0,
               "%s: bad geometry", who);
  const int xl = d->x_ld ? d->x_ld : d->Cin, yl = d->y_ld ? d->y_ld : d->Cout;
  SG_CHECK_ARG((int64_t)d->N * d->H * d->W * xl < (1ll << 31) && (int64_t)d->N * d->Ho * d->Wo * yl < (1ll << 31),
               "%s: tensor exceeds 2^31 elements", who);
  return 0;
}

inline int dw_esize(int dtype) { return dtype == SG_BF16 ? 2 : 4; }

template <typename T>
void dw_fill(DwParams<T>& p, const sg_conv_desc* d) {
  p.N = d->N; p.H = d->H; p.W = d->W; p.C = d->Cin; p.Ho = d->Ho; p.Wo = d->Wo; p.KH = d->KH; p.KW = d->KW;
  p.stride = d->stride; p.dil = d->dilation; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
  p.x_ld = d->x_ld ? d->x_ld : d->Cin;
  p.y_ld = d->y_ld ? d->y_ld : d->Cout;
}

}  // namespace

extern "C" {

int sg_dwconv2d_plan(const sg_ctx* ctx, int dtype, const sg_conv_desc* d, int direction, int aligned, int sums, sg_dw_plan* out) {
  SG_CHECK_ARG(out, "sg_dwconv2d_plan: null out");
  *out = sg_dw_plan{};
  SG_CHECK_ARG(direction >= SG_DW_FWD && direction <= SG_DW_WGRAD && (!sums || direction == SG_DW_DGRAD),
               "sg_dwconv2d_plan: bad direction / sums with another direction than the dgrad");
  int rc = dw_check(ctx, dtype, d, "sg_dwconv2d_plan");
  if (rc) return rc;
  SG_CHECK_ARG(direction != SG_DW_WGRAD || (d->KH == 3 && d->KW == 3), "sg_dwconv2d_plan: only 3x3 depthwise kernels have a filter gradient");
  *out = plan_dw(ctx->num_cus, dw_esize(dtype), d, direction, aligned != 0, sums != 0);
  return 0;
}

int sg_dwconv2d_fwd(sg_ctx* ctx, void* stream, int dtype, const sg_conv_desc* d, const void* x, const void* w, void* y,
                    int pre_relu, const sg_bn_in* bn) {
  int rc = dw_check(ctx, dtype, d, "sg_dwconv2d_fwd");
  if (rc) return rc;
  SG_CHECK_ARG(x && w && y, "sg_dwconv2d_fwd: null tensor");
  if (bn) {
    SG_CHECK_ARG(!pre_relu && !bn->infer, "sg_dwconv2d_fwd: bn with pre_relu (bn->relu has that role) / an inference-mode bn");
    SG_CHECK_ARG(bn->gamma && bn->beta && bn->mean && bn->invstd, "sg_dwconv2d_fwd: bn with a null BatchNormalization parameter");
    pre_relu = bn->relu;
  }
  const sg_bn_in b = bn ? *bn : sg_bn_in{};   // all-null without bn
  const DwPlan pl = plan_dw(ctx->num_cus, dw_esize(dtype), d, SG_DW_FWD,
                            sg_all_aligned16({x, w, y, b.gamma, b.beta, b.mean, b.invstd}), false);
  if (bn && !pl.bn) {
    sg_set_error("sg_dwconv2d_fwd: bn, but only the stride-1 3x3 run kernels (W %% 4 == 0, C %% 4 == 0, 16-byte aligned) fuse the "
                 "BatchNormalization; materialise it instead");
    return SG_EUNSUPPORTED;
  }
  SG_DTYPE_SWITCH(dtype, "sg_dwconv2d_fwd", {
    if (pl.family != SG_DWK_GENERIC) {
      DwRunParams<T> r;
      r.in = (const T*)x; r.w = (const float*)w; r.mask = nullptr; r.res = nullptr; r.out = (T*)y;
      r.bn_gamma = (const float*)b.gamma; r.bn_beta = (const float*)b.beta; r.bn_mean = (const float*)b.mean; r.bn_invstd = (const float*)b.invstd;
      r.in_ld = d->x_ld ? d->x_ld : d->Cin; r.out_ld = d->y_ld ? d->y_ld : d->Cout; r.mask_ld = 0;
      r.relu_in = pre_relu; r.flip = 0;
      // never a mask or sums here (DW_MASK* / DW_SUMS are the dgrad's): pre_relu with bn is refused above, bn->relu takes its place
      return launch_dw_stencil(pl, bn ? (pre_relu ? DW_BN_RELU : DW_BN) : (pre_relu ? DW_RELU : DW_PLAIN), d, r, (hipStream_t)stream);
    }
    DwParams<T> p;
    dw_fill(p, d);
    p.x = (const T*)x; p.w = (const float*)w; p.dy = nullptr; p.out = (T*)y; p.pre_relu = pre_relu;
    p.fd_cv = make_fastdiv((uint32_t)(p.C / pl.V)); p.fd_w = make_fastdiv((uint32_t)p.Wo); p.fd_h = make_fastdiv((uint32_t)p.Ho);
    if (pl.V == 4) hipLaunchKernelGGL((dw_fwd_kernel<4, T>), dim3((unsigned)pl.gx), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((dw_fwd_kernel<1, T>), dim3((unsigned)pl.gx), dim3(256), 0, (hipStream_t)stream, p);
  });
  SG_LAUNCH_CHECK("dw_fwd_kernel");
  return 0;
}

// second stage of the BatchNormalization sums written by the stencil's SUMS forms: seg_finalize_kernel adds the partial rows in
// fp64 (fixed order) and hands the two totals of a channel to this op
struct BnSumsFinalOp {
  static constexpr int NOUT = 2;
  float* dgamma;
  float* dbeta;
  __device__ __forceinline__ void finalize(int, int c, const double (&s)[2]) const {
    dbeta[c] = (float)s[0];
    dgamma[c] = (float)s[1];
  }
};

// what a launch with sums requires (the plan's ws_bytes; alignment and geometry do not enter it) and 256 bytes of slack
size_t sg_dwconv2d_dgrad_bnsums_ws_bytes(const sg_ctx* ctx, const sg_conv_desc* d) {
  if (!ctx || !d) return 0;
  return plan_dw(ctx->num_cus, 4, d, SG_DW_DGRAD, true, true).ws_bytes + 256;
}

int sg_dwconv2d_dgrad(sg_ctx* ctx, void* stream, int dtype, const sg_conv_desc* d, const void* dy, const void* w,
                      const void* x_for_mask, void* dx, int pre_relu, const void* res, const sg_dw_bnsums* sums) {
  int rc = dw_check(ctx, dtype, d, "sg_dwconv2d_dgrad");
  if (rc) return rc;
  SG_CHECK_ARG(dy && w && dx, "sg_dwconv2d_dgrad: null tensor");
  SG_CHECK_ARG(!sums || (sums->x && sums->mean && sums->invstd && sums->gamma && sums->beta && sums->dgamma && sums->dbeta),
               "sg_dwconv2d_dgrad: sums with a null tensor");
  SG_CHECK_ARG(!pre_relu || x_for_mask, "sg_dwconv2d_dgrad: pre_relu needs the forward input");
  const sg_dw_bnsums q = sums ? *sums : sg_dw_bnsums{};   // all-null without sums
  const DwPlan pl = plan_dw(ctx->num_cus, dw_esize(dtype), d, SG_DW_DGRAD,
                            sg_all_aligned16({dy, w, dx, pre_relu ? x_for_mask : nullptr, res, q.x, q.mean, q.invstd, q.gamma, q.beta}),
                            sums != nullptr);
  if ((res && !pl.res) || (sums && !pl.sums)) {
    sg_set_error("sg_dwconv2d_dgrad: res / sums, but only the stride-1 3x3 run kernels (W %% 4 == 0, C %% 4 == 0, 16-byte aligned) add a "
                 "collected gradient or sum for the BatchNormalization; add it afterwards / use sg_bn_train_bwd instead");
    return SG_EUNSUPPORTED;
  }
  if (sums && (!sums->ws || sums->ws_bytes < pl.ws_bytes)) {
    sg_set_error("sg_dwconv2d_dgrad: sums workspace %zu < %zu", sums->ws_bytes, pl.ws_bytes);
    return SG_EWORKSPACE;
  }
  SG_DTYPE_SWITCH(dtype, "sg_dwconv2d_dgrad", {
    if (pl.family != SG_DWK_GENERIC) {  // stride-1 dgrad = the same stencil with the kernel flipped
      DwRunParams<T> r;
      r.in = (const T*)dy; r.w = (const float*)w; r.mask = pre_relu ? (const T*)x_for_mask : nullptr; r.out = (T*)dx; r.res = (const T*)res;
      r.bn_gamma = r.bn_beta = r.bn_mean = r.bn_invstd = nullptr;
      r.in_ld = d->y_ld ? d->y_ld : d->Cout; r.out_ld = r.mask_ld = d->x_ld ? d->x_ld : d->Cin;
      r.relu_in = 0; r.flip = 1;
      if (sums) {
        r.bs_x = (const T*)sums->x; r.bs_ld = d->Cin;   // the BatchNormalization's input is a dense tensor
        r.bs_mean = (const float*)sums->mean; r.bs_invstd = (const float*)sums->invstd;
        r.bs_gamma = (const float*)sums->gamma; r.bs_beta = (const float*)sums->beta; r.bs_relu = sums->relu ? 1 : 0; r.bs_part = (float*)sums->ws;
      }
      // never relu_in or a fused BatchNormalization here (DW_RELU / DW_BN* are the forward's): this entry point has no such operand
      rc = launch_dw_stencil(pl, sums ? (pre_relu ? DW_MASK_SUMS : DW_SUMS) : (pre_relu ? DW_MASK : DW_PLAIN), d, r, (hipStream_t)stream);
      if (rc || !sums) return rc;
      BnSumsFinalOp op;
      op.dgamma = (float*)sums->dgamma; op.dbeta = (float*)sums->dbeta;
      seg_finalize_launch(op, 1, d->Cin, pl.S, (const float*)sums->ws, (hipStream_t)stream);   // pl.S = gy partial rows
      SG_LAUNCH_CHECK("sg_dwconv2d_dgrad sums");
      return 0;
    }
    DwParams<T> p;
    dw_fill(p, d);
    p.x = (const T*)x_for_mask; p.w = (const float*)w; p.dy = (const T*)dy; p.out = (T*)dx; p.pre_relu = pre_relu;
    p.fd_cv = make_fastdiv((uint32_t)(p.C / pl.V)); p.fd_w = make_fastdiv((uint32_t)p.W); p.fd_h = make_fastdiv((uint32_t)p.H);
    if (pl.V == 4) hipLaunchKernelGGL((dw_dgrad_kernel<4, T>), dim3((unsigned)pl.gx), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((dw_dgrad_kernel<1, T>), dim3((unsigned)pl.gx), dim3(256), 0, (hipStream_t)stream, p);
  });
  SG_LAUNCH_CHECK("dw_dgrad_kernel");
  return 0;
}

// An upper bound of plan_dw's ws_bytes over what the query cannot know (+ 256 of slack): whether the operands will be aligned -
// hence DwWgradOp's plan at V = 4 and at V = 1 - and, on a dw_run_ok map, which of the two fast kernels the switches pick - the strips,
// and the run reducer at RR = 1: seg_plan's part_bytes does not decrease as the row count grows (S = min(ceil(4 CUs / gx),
// ceil(rows / (4 TY))) and the one-workgroup rule only lowers small counts), and ceil(rows / 4) >= rows / (4 RR) for RR = 1 and 2.
size_t sg_dwconv2d_wgrad_ws_bytes(const sg_ctx* ctx, const sg_conv_desc* d) {
  if (!ctx || !d) return 0;
  const int64_t rows = (int64_t)d->N * d->Ho * d->Wo;
  DwPlan v4 = {}, v1 = {}, run = {}, strip = {};
  plan_dw_wgrad_seg(v4, ctx->num_cus, SG_DWK_GENERIC, rows, d->Cin, true);
  plan_dw_wgrad_seg(v1, ctx->num_cus, SG_DWK_GENERIC, rows, d->Cin, false);
  plan_dw_wgrad_seg(run, ctx->num_cus, SG_DWK_RUN, sg_cdiv(rows, 4), d->Cin, true);
  if (dw_run_ok(d)) plan_dw_wgrad_strip(strip, ctx->num_cus, d);
  return std::max({v4.ws_bytes, v1.ws_bytes, run.ws_bytes, strip.ws_bytes}) + 256;
}

int sg_dwconv2d_wgrad(sg_ctx* ctx, void* stream, int dtype, const sg_conv_desc* d, const void* x, const void* dy, void* dw,
                      int pre_relu, const sg_bn_in* bn, void* ws, size_t ws_bytes) {
  int rc = dw_check(ctx, dtype, d, "sg_dwconv2d_wgrad");
  if (rc) return rc;
  SG_CHECK_ARG(x && dy && dw, "sg_dwconv2d_wgrad: null tensor");
  if (bn) {
    SG_CHECK_ARG(!pre_relu && !bn->infer, "sg_dwconv2d_wgrad: bn with pre_relu (bn->relu has that role) / an inference-mode bn");
    SG_CHECK_ARG(bn->gamma && bn->beta && bn->mean && bn->invstd, "sg_dwconv2d_wgrad: bn with a null BatchNormalization parameter");
    pre_relu = bn->relu;
  }
  const sg_bn_in b = bn ? *bn : sg_bn_in{};   // all-null without bn
  const DwPlan pl = plan_dw(ctx->num_cus, dw_esize(dtype), d, SG_DW_WGRAD, sg_all_aligned16({x, dy, b.gamma, b.beta, b.mean, b.invstd}), false);
  if (bn && !pl.bn) {
    sg_set_error("sg_dwconv2d_wgrad: bn, but only the stride-1 3x3 run kernels fuse the BatchNormalization; materialise it instead");
    return SG_EUNSUPPORTED;
  }
  SG_CHECK_ARG(d->KH == 3 && d->KW == 3, "sg_dwconv2d_wgrad: only 3x3 depthwise kernels occur on this path");
  if (!ws || ws_bytes < pl.ws_bytes) {
    sg_set_error("sg_dwconv2d_wgrad: workspace %zu < %zu", ws_bytes, pl.ws_bytes);
    return SG_EWORKSPACE;
  }
  const int x_ld = d->x_ld ? d->x_ld : d->Cin, y_ld = d->y_ld ? d->y_ld : d->Cout;
  SG_DTYPE_SWITCH(dtype, "sg_dwconv2d_wgrad", {
    if (pl.family == SG_DWK_STRIP) {
      const dim3 grid((unsigned)pl.gx, (unsigned)pl.S);
      const FastDiv fq = make_fastdiv((uint32_t)(d->W / 4)), fh = make_fastdiv((uint32_t)pl.nhs);
      const unsigned xb_ = (unsigned)((int64_t)d->N * d->H * d->W * x_ld * (int64_t)sizeof(T));
      const unsigned yb_ = (unsigned)((int64_t)d->N * d->H * d->W * y_ld * (int64_t)sizeof(T));
      dw_with_pre_bn(pre_relu, bn != nullptr, [&](auto pre_, auto bn_) {
        constexpr bool PRE_ = decltype(pre_)::value, BN_ = decltype(bn_)::value;
        hipLaunchKernelGGL((dw_wgrad_strip_kernel<T, PRE_, BN_>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)dy,
                           (float*)ws, d->H, d->W, d->Cin, x_ld, y_ld, pl.HS, pl.count, pl.S, xb_, yb_, fq, fh,
                           (const float*)b.gamma, (const float*)b.beta, (const float*)b.mean, (const float*)b.invstd);
      });
      SG_LAUNCH_CHECK("dw_wgrad_strip_kernel");
      DwWgradRunOp<1, T, false> fin;   // finalize() only: dw[t][c] = the fp64 sum of the S partial rows
      fin.dw = (float*)dw; fin.C = d->Cin;
      seg_finalize_launch(fin, 1, d->Cin, pl.S, (const float*)ws, (hipStream_t)stream);
      SG_LAUNCH_CHECK("dw_wgrad_strip finalize");
      return 0;
    }
    if (pl.family == SG_DWK_RUN) {
      auto run = [&](auto ro) -> int {
        ro.x = (const T*)x; ro.dy = (const T*)dy; ro.dw = (float*)dw; ro.H = d->H; ro.W = d->W; ro.C = d->Cin; ro.x_ld = x_ld; ro.y_ld = y_ld;
        ro.bn_gamma = (const float*)b.gamma; ro.bn_beta = (const float*)b.beta; ro.bn_mean = (const float*)b.mean; ro.bn_invstd = (const float*)b.invstd;
        ro.fd_rpr = make_fastdiv((uint32_t)(d->W / 4)); ro.fd_h = make_fastdiv((uint32_t)(d->H / pl.RR));
        return seg_reduce_launch(ro, pl.seg, 1, pl.count, d->Cin, (float*)ws, (hipStream_t)stream, "dw_wgrad_run");
      };
      return dw_with_pre_bn(pre_relu, bn != nullptr, [&](auto pre_, auto bn_) -> int {
        constexpr bool PRE_ = decltype(pre_)::value, BN_ = decltype(bn_)::value;
        return pl.RR == 2 ? run(DwWgradRunOp<2, T, PRE_, BN_>{}) : run(DwWgradRunOp<1, T, PRE_, BN_>{});
      });
    }
    DwWgradOp<T> op;
    op.x = (const T*)x; op.dy = (const T*)dy; op.dw = (float*)dw;
    op.H = d->H; op.W = d->W; op.C = d->Cin; op.Ho = d->Ho; op.Wo = d->Wo; op.stride = d->stride; op.dil = d->dilation;
    op.pad_t = d->pad_t; op.pad_l = d->pad_l; op.x_ld = x_ld; op.y_ld = y_ld;
    op.pre_relu = pre_relu;
    op.fd_w = make_fastdiv((uint32_t)d->Wo); op.fd_h = make_fastdiv((uint32_t)d->Ho);
    return seg_reduce_launch(op, pl.seg, 1, (int64_t)d->N * d->Ho * d->Wo, d->Cin, (float*)ws, (hipStream_t)stream, "dw_wgrad");
  });
  return 0;
}

}  // extern "C"
