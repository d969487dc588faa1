// The streaming kernels of the convolutions (conv_thin.h): the thin 1x1 forward / input-gradient kernels and the three ops of the
// fixed-order segmented reducer that belong to a convolution - the thin filter gradient, the bias gradient, the BatchNormalization
// statistics from per-tile sums.  This is the one convolution unit that includes sg_reduce.h: one arrival-counter ring (seg_counters)
// serves all three.
#include "conv_thin.h"
#include "sg_reduce.h"

using namespace sgconv;

namespace {

// bias gradient = column sums of dy[rows][C] (pixel stride ld), through the fixed-order segmented reducer
template <typename T>
struct ColSumOp {
  static constexpr int NOUT = 1;
  const T* __restrict__ a;
  float* out;
  int ld;
  template <int V>
  __device__ __forceinline__ void accum(int, int64_t r, int c, float (&acc)[1][V]) const {
    float v[V];
    ldv<V>(a + r * ld + c, v);
#pragma unroll
    for (int k = 0; k < V; ++k) acc[0][k] += v[k];
  }
  __device__ __forceinline__ void finalize(int, int c, const double (&s)[1]) const { out[c] = (float)s[0]; }
};

template <typename T>
int launch_colsum_t(int num_cus, const T* dy, int64_t rows, int C, int ld, float* out, float* part, hipStream_t st) {
  const bool vec = (C % 4 == 0) && (ld % 4 == 0) && sg_aligned16(dy);
  const SegPlan pl = seg_plan<1>(num_cus, 1, rows, C, vec);
  ColSumOp<T> op;
  op.a = dy; op.out = out; op.ld = ld;
  return seg_reduce_launch(op, pl, 1, rows, C, part, st, "colsum");
}

// ---- "thin" 1x1 convolutions: Cout <= 4 ----------------------------------------------------------------
// The sSE gate (C -> 1, sigmoid) and the softmax head (32 -> 2 at full resolution) are pixel-wise dot
// products: 2*Cout FLOP per 4 bytes read, bandwidth-bound by two orders of magnitude.  A 128-wide MFMA tile
// would spend 97 % of its columns on zero padding, so they get streaming kernels instead: forward = LP lanes
// per pixel, each lane one 16-byte channel chunk, sub-wave shuffle reduction; dgrad = one 16-byte store per
// thread; wgrad = the segmented column reducer with Cout outputs per channel.
template <int CO, typename TA, typename TY>
__global__ __launch_bounds__(256) void thin_fwd_kernel(const TA* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, TY* __restrict__ y, int64_t P,
                                                       int chunks, int x_ld, int y_ld, int LP, int flags, const BnIn bn) {
  constexpr int PIX = 4;  // pixels per lane group: four independent 16-byte loads in flight
  const int t = threadIdx.x;
  const int gpb = 256 / LP;  // lane groups per block
  const int li = t & (LP - 1), grp = t / LP;
  float acc[PIX][CO];
#pragma unroll
  for (int i = 0; i < PIX; ++i)
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[i][o] = 0.f;
  int64_t pix[PIX];
#pragma unroll
  for (int i = 0; i < PIX; ++i) pix[i] = ((int64_t)blockIdx.x * PIX + i) * gpb + grp;
  for (int c = li; c < chunks; c += LP) {
    float wv[4][CO];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int o = 0; o < CO; ++o) wv[k][o] = w[(4 * c + k) * CO + o];
    f32x4 xv[PIX];
#pragma unroll
    for (int i = 0; i < PIX; ++i) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      xv[i] = pix[i] < P ? ld4<TA>(x + pix[i] * x_ld + 4 * c) : z;
    }
    if (bn.mean) {   // uniform: the BatchNormalization (+ReLU) in front of this layer, applied here
      const f32x4 bm = *reinterpret_cast<const f32x4*>(bn.mean + 4 * c), bi = bn_in_inv(bn, 4 * c);
      const f32x4 bg = *reinterpret_cast<const f32x4*>(bn.gamma + 4 * c), bb = *reinterpret_cast<const f32x4*>(bn.beta + 4 * c);
#pragma unroll
      for (int i = 0; i < PIX; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) xv[i][k] = pix[i] < P ? bn_in_one(xv[i][k], bm[k], bi[k], bg[k], bb[k], bn.relu) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < PIX; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 0; o < CO; ++o) acc[i][o] = fmaf(xv[i][k], wv[k][o], acc[i][o]);
  }
#pragma unroll
  for (int i = 0; i < PIX; ++i)
#pragma unroll
    for (int o = 0; o < CO; ++o)
      for (int off = LP >> 1; off > 0; off >>= 1) acc[i][o] += __shfl_xor(acc[i][o], off, 64);
  if (li == 0) {
#pragma unroll
    for (int i = 0; i < PIX; ++i) {
      if (pix[i] >= P) continue;
#pragma unroll
      for (int o = 0; o < CO; ++o) {
        float v = acc[i][o] + ((flags & SG_EPI_BIAS) ? bias[o] : 0.f);
        if (flags & SG_EPI_RELU) v = fmaxf(v, 0.f);
        st1<TY>(y + pix[i] * y_ld + o, v);
      }
    }
  }
}

template <int CO, typename TA, typename TY>
__global__ __launch_bounds__(256) void thin_dgrad_kernel(const TY* __restrict__ dy, const float* __restrict__ w,
                                                         TA* dx, int64_t total, int chunks, int y_ld, int x_ld,
                                                         const TA* res) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int64_t pix = gid / chunks;
  const int c = (int)(gid - pix * chunks);
  float g[CO];
#pragma unroll
  for (int o = 0; o < CO; ++o) g[o] = ld1<TY>(dy + pix * y_ld + o);
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float a = 0.f;
#pragma unroll
    for (int o = 0; o < CO; ++o) a = fmaf(g[o], w[(4 * c + k) * CO + o], a);
    r[k] = a;
  }
  if (res) {   // uniform: a gradient already collected for the same tensor (sg_conv_opts.res; may be dx itself)
    const f32x4 t = ld4<TA>(res + pix * x_ld + 4 * c);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] += t[k];
  }
  st4<TA>(dx + pix * x_ld + 4 * c, r);
}

template <int CO, typename TA, typename TY>
struct ThinWgradOp {
  static constexpr int NOUT = CO;
  const TA* __restrict__ x;
  const TY* __restrict__ dy;
  float* dw;
  int x_ld, y_ld;
  BnIn bn;   // the BatchNormalization (+ReLU) in front of the layer, applied to x here (mean == nullptr: none)
  template <int V>
  __device__ __forceinline__ void accum(int, int64_t r, int c, float (&acc)[CO][V]) const {
    float v[V];
    ldv<V>(x + r * x_ld + c, v);
    if (bn.mean) {   // uniform
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float is = bn.infer ? rsqrtf(bn.invstd[c + k] + bn.eps) : bn.invstd[c + k];
        v[k] = bn_in_one(v[k], bn.mean[c + k], is, bn.gamma[c + k], bn.beta[c + k], bn.relu);
      }
    }
#pragma unroll
    for (int o = 0; o < CO; ++o) {
      const float g = ld1<TY>(dy + r * y_ld + o);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[o][k] = fmaf(v[k], g, acc[o][k]);
    }
  }
  __device__ __forceinline__ void finalize(int, int c, const double (&s)[CO]) const {
#pragma unroll
    for (int o = 0; o < CO; ++o) dw[c * CO + o] = (float)s[o];
  }
};

template <int NOUT>
size_t thin_part_bytes_t(int num_cus, int64_t P, int Cin) { return seg_plan<NOUT>(num_cus, 1, P, Cin, true).part_bytes; }

template <int CO, typename TA, typename TY>
int thin_fwd_t(const sg_conv_desc* d, const TA* x, const float* w, const float* bias, TY* y, int flags, hipStream_t st,
               const BnIn bn = bn_in_none()) {
  const int64_t P = (int64_t)d->N * d->H * d->W;
  const int chunks = d->Cin / 4;
  int LP = 1;
  while (LP * 2 <= chunks && LP < 64) LP <<= 1;
  const int64_t groups = sg_cdiv(P, (int64_t)4 * (256 / LP));
  hipLaunchKernelGGL((thin_fwd_kernel<CO, TA, TY>), dim3((unsigned)groups), dim3(256), 0, st, x, w, bias, y, P, chunks,
                     d->x_ld ? d->x_ld : d->Cin, d->y_ld ? d->y_ld : d->Cout, LP, flags, bn);
  SG_LAUNCH_CHECK("thin_fwd_kernel");
  return 0;
}

template <int CO, typename TA, typename TY>
int thin_dgrad_t(const sg_conv_desc* d, const TY* dy, const float* w, TA* dx, hipStream_t st, const void* res = nullptr) {
  const int64_t P = (int64_t)d->N * d->H * d->W;
  const int chunks = d->Cin / 4;
  const int64_t total = P * chunks;
  hipLaunchKernelGGL((thin_dgrad_kernel<CO, TA, TY>), dim3((unsigned)sg_cdiv(total, 256)), dim3(256), 0, st, dy, w, dx, total, chunks,
                     d->y_ld ? d->y_ld : d->Cout, d->x_ld ? d->x_ld : d->Cin, (const TA*)res);
  SG_LAUNCH_CHECK("thin_dgrad_kernel");
  return 0;
}

template <int CO, typename TA, typename TY>
int thin_wgrad_t(int num_cus, const sg_conv_desc* d, const TA* x, const TY* dy, float* dw, float* part, hipStream_t st,
                 const BnIn bn = bn_in_none()) {
  const int64_t P = (int64_t)d->N * d->H * d->W;
  const SegPlan pl = seg_plan<CO>(num_cus, 1, P, d->Cin, true);
  ThinWgradOp<CO, TA, TY> op;
  op.x = x; op.dy = dy; op.dw = dw;
  op.bn = bn;
  op.x_ld = d->x_ld ? d->x_ld : d->Cin;
  op.y_ld = d->y_ld ? d->y_ld : d->Cout;
  return seg_reduce_launch(op, pl, 1, P, d->Cin, part, st, "thin_wgrad");
}

// mean / variance over all rows from the per-tile (sum, centred sum of squares) pairs: a segmented column reduction
// over the T tiles (rows of the reducer = tiles), pivoted on tile 0's mean so nothing cancels, combined in fp64, then
// the BatchNormalization bookkeeping of BnStatsOp::finalize.
struct BnTilesOp {
  static constexpr int NOUT = 2;
  const float* __restrict__ stats;  // [T][2][C]
  int C;
  int64_t rows;                     // pixels (not tiles)
  float* moving_mean;
  float* moving_var;
  float* save_mean;
  float* save_invstd;
  float momentum, eps;
  int unbiased;

  template <int V>
  __device__ __forceinline__ void accum(int, int64_t r, int c, float (&acc)[2][V]) const {
    float s1[V], m2[V], s0[V];
    ldv<V>(stats + (2 * r) * C + c, s1);
    ldv<V>(stats + (2 * r + 1) * C + c, m2);
    ldv<V>(stats + c, s0);
    const int64_t left = rows - r * BM;
    const float nt = (float)(left < BM ? left : BM), n0 = (float)(rows < BM ? rows : BM);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float d = s1[i] / nt - s0[i] / n0;  // tile mean minus the pivot (tile 0's mean)
      acc[0][i] = fmaf(nt, d, acc[0][i]);
      acc[1][i] += fmaf(nt * d, d, m2[i]);
    }
  }
  __device__ __forceinline__ void finalize(int, int c, const double (&s)[2]) const {
    const double n = (double)rows, n0 = (double)(rows < BM ? rows : BM);
    const double m1 = s[0] / n;
    const double mean = (double)stats[c] / n0 + m1;
    double var = s[1] / n - m1 * m1;
    if (var < 0.0) var = 0.0;
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    const double var_u = (unbiased && rows > 1) ? var * (n / (n - 1.0)) : var;
    moving_mean[c] = (float)((double)moving_mean[c] * momentum + mean * (1.0 - (double)momentum));
    moving_var[c] = (float)((double)moving_var[c] * momentum + var_u * (1.0 - (double)momentum));
  }
};

#define THIN_SWITCH(co, CALL)      \
  switch (co) {                    \
    case 1: return CALL(1);        \
    case 2: return CALL(2);        \
    case 3: return CALL(3);        \
    default: return CALL(4);       \
  }

}  // namespace

namespace sgconv {

size_t thin_part_bytes(int num_cus, const sg_conv_desc* d) {
  const int64_t P = (int64_t)d->N * d->H * d->W;
  switch (d->Cout) {
    case 1: return thin_part_bytes_t<1>(num_cus, P, d->Cin);
    case 2: return thin_part_bytes_t<2>(num_cus, P, d->Cin);
    case 3: return thin_part_bytes_t<3>(num_cus, P, d->Cin);
    default: return thin_part_bytes_t<4>(num_cus, P, d->Cin);
  }
}

int launch_thin_fwd(const sg_conv_desc* d, bool x_b16, bool y_b16, const void* x, const float* w, const float* bias, void* y, int flags,
                    hipStream_t st, const BnIn& bn) {
  if (!x_b16) {
#define CALL(CO) thin_fwd_t<CO, float, float>(d, (const float*)x, w, bias, (float*)y, flags, st, bn)
    THIN_SWITCH(d->Cout, CALL)
#undef CALL
  } else if (!y_b16) {
#define CALL(CO) thin_fwd_t<CO, bf16_t, float>(d, (const bf16_t*)x, w, bias, (float*)y, flags, st)
    THIN_SWITCH(d->Cout, CALL)
#undef CALL
  } else {
#define CALL(CO) thin_fwd_t<CO, bf16_t, bf16_t>(d, (const bf16_t*)x, w, bias, (bf16_t*)y, flags, st)
    THIN_SWITCH(d->Cout, CALL)
#undef CALL
  }
}

int launch_thin_dgrad(const sg_conv_desc* d, bool x_b16, bool y_b16, const void* dy, const float* w, void* dx, hipStream_t st,
                      const void* res) {
  if (!x_b16) {
#define CALL(CO) thin_dgrad_t<CO, float, float>(d, (const float*)dy, w, (float*)dx, st, res)
    THIN_SWITCH(d->Cout, CALL)
#undef CALL
  } else if (!y_b16) {
#define CALL(CO) thin_dgrad_t<CO, bf16_t, float>(d, (const float*)dy, w, (bf16_t*)dx, st)
    THIN_SWITCH(d->Cout, CALL)
#undef CALL
  } else {
#define CALL(CO) thin_dgrad_t<CO, bf16_t, bf16_t>(d, (const bf16_t*)dy, w, (bf16_t*)dx, st, res)
    THIN_SWITCH(d->Cout, CALL)
#undef CALL
  }
}

int launch_thin_wgrad(int num_cus, const sg_conv_desc* d, bool x_b16, bool y_b16, const void* x, const void* dy, float* dw, float* part,
                      hipStream_t st, const BnIn& bn) {
  if (!x_b16) {
#define CALL(CO) thin_wgrad_t<CO, float, float>(num_cus, d, (const float*)x, (const float*)dy, dw, part, st, bn)
    THIN_SWITCH(d->Cout, CALL)
#undef CALL
  } else if (!y_b16) {
#define CALL(CO) thin_wgrad_t<CO, bf16_t, float>(num_cus, d, (const bf16_t*)x, (const float*)dy, dw, part, st)
    THIN_SWITCH(d->Cout, CALL)
#undef CALL
  } else {
#define CALL(CO) thin_wgrad_t<CO, bf16_t, bf16_t>(num_cus, d, (const bf16_t*)x, (const bf16_t*)dy, dw, part, st)
    THIN_SWITCH(d->Cout, CALL)
#undef CALL
  }
}
#undef THIN_SWITCH

size_t colsum_ws_bytes(int num_cus, int64_t rows, int C) {
  const SegPlan a = seg_plan<1>(num_cus, 1, rows, C, true), b = seg_plan<1>(num_cus, 1, rows, C, false);
  return a.part_bytes > b.part_bytes ? a.part_bytes : b.part_bytes;
}

int launch_colsum(int num_cus, bool b16, const void* dy, int64_t rows, int C, int ld, float* out, float* part, hipStream_t st) {
  if (b16) return launch_colsum_t<bf16_t>(num_cus, (const bf16_t*)dy, rows, C, ld, out, part, st);
  return launch_colsum_t<float>(num_cus, (const float*)dy, rows, C, ld, out, part, st);
}

size_t bn_tiles_ws_bytes(int num_cus, int tiles, int C) {
  return seg_plan<2>(num_cus, 1, tiles, C, true).part_bytes + seg_plan<2>(num_cus, 1, tiles, C, false).part_bytes;
}
static SegPlan bn_tiles_plan(int num_cus, int tiles, int C, const void* stats) {
  const bool vec = (C % 4 == 0) && sg_aligned16(stats);
  return seg_plan<2>(num_cus, 1, tiles, C, vec);
}
size_t bn_tiles_part_bytes(int num_cus, int tiles, int C, const void* stats) { return bn_tiles_plan(num_cus, tiles, C, stats).part_bytes; }

int launch_bn_tiles(int num_cus, const float* stats, int tiles, int C, int64_t rows, float* moving_mean, float* moving_var,
                    float* save_mean, float* save_invstd, float momentum, float eps, int unbiased, float* part, hipStream_t st) {
  BnTilesOp op;
  op.stats = stats; op.C = C; op.rows = rows;
  op.moving_mean = moving_mean; op.moving_var = moving_var;
  op.save_mean = save_mean; op.save_invstd = save_invstd;
  op.momentum = momentum; op.eps = eps; op.unbiased = unbiased;
  return seg_reduce_launch(op, bn_tiles_plan(num_cus, tiles, C, stats), 1, tiles, C, part, st, "bn_tiles");
}

}  // namespace sgconv
