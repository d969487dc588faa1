// HBM-bound kernels that change a map's resolution (NHWC, channels innermost so every access is a coalesced run of 16-byte
// channel chunks): max pooling (plain and with recorded cells), average pooling, nearest and bilinear up-sampling by an
// integer factor, and the resize between arbitrary sizes (bilinear or nearest, up or down).  Each
// is a small op under one of two skeletons: pixel_kernel (one work item = one pixel x V channels) or window_kernel (one
// workgroup = one dx pixel of a large-factor up-sampling gradient).
#include <limits.h>
#include <type_traits>
#include "sg_reduce.h"
#include "resize_coords.h"

namespace {

constexpr int64_t EW_CAP = 16384;   // ew_blocks: workgroups of this file's element-wise launches

// ------------------------------------------------------------------------- generic (pixel, channel chunk) element-wise
// op.apply<V>(pix, n, h, w, c) for every pixel pix = (n, h, w) of an N x H x W grid and every V-wide channel chunk c: the
// output grid for the forward ops, the input grid for the gathers.  An op that reads tables from dynamic LDS has a member
// lds_tables(), which every workgroup runs once before its loop (it ends with a barrier); an op without tables has none.
template <class Op, class = void>
struct has_lds_tables : std::false_type {};
template <class Op>
struct has_lds_tables<Op, std::void_t<decltype(&Op::lds_tables)>> : std::true_type {};

template <class Op, int V>
__global__ void pixel_kernel(const Op op, uint32_t total, FastDiv fd_cv, FastDiv fd_w, FastDiv fd_h) {
  if constexpr (has_lds_tables<Op>::value) op.lds_tables();
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    uint32_t pix, cc, row, w, n, h;
    fd_divmod(i, fd_cv, pix, cc);
    fd_divmod(pix, fd_w, row, w);
    fd_divmod(row, fd_h, n, h);
    op.template apply<V>(pix, n, h, w, (int)cc * V);
  }
}

template <class Op>
int launch_pixels(const Op& op, int N, int H, int W, int C, bool vec, size_t lds_bytes, hipStream_t st, const char* name) {
  const int V = vec ? 4 : 1;
  const int64_t total = (int64_t)N * H * W * (C / V);
  const unsigned blocks = ew_blocks(total, EW_CAP);
  const FastDiv fd_cv = make_fastdiv((uint32_t)(C / V)), fd_w = make_fastdiv((uint32_t)W), fd_h = make_fastdiv((uint32_t)H);
  if (vec) hipLaunchKernelGGL((pixel_kernel<Op, 4>), dim3(blocks), dim3(256), lds_bytes, st, op, (uint32_t)total, fd_cv, fd_w, fd_h);
  else hipLaunchKernelGGL((pixel_kernel<Op, 1>), dim3(blocks), dim3(256), lds_bytes, st, op, (uint32_t)total, fd_cv, fd_w, fd_h);
  SG_LAUNCH_CHECK(name);
  return 0;
}

// the tail of every gradient op: dx = acc, or dx += acc when `accumulate`
template <int V, typename T>
__device__ __forceinline__ void store_grad(T* __restrict__ o, float (&acc)[V], int accumulate) {
  if (accumulate) {
    float t[V];
    ldv<V>(o, t);
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] += t[k];
  }
  stv<V>(o, acc);
}

// ------------------------------------------------------------------ one workgroup per dx pixel (large up-sampling factors)
// Large windows (the ASPP image-pooling branch: 1x1 -> 32x32, 1024 cells per output element): pixel_kernel would give each
// of N*C/4 = 1024 lanes a serial sum of 1024 loads (285 us for 17 MB).  Here a workgroup owns one dx pixel and 8 channel
// chunks, 32 lanes share the pixel's cells - op.cells(n, ih, iw, c, ty, acc) adds lane ty's cells ty, ty + 32, ... in that
// order - and the 32 partial sums are added in fixed order through LDS.  The two up-sampling gradients (UpsampleBwd,
// BilinearBwd) have both forms: apply() under pixel_kernel, cells() here; the op also holds dx, C and accumulate.
constexpr int WIN_TX = 8, WIN_TY = 32;

template <class Op>
__global__ __launch_bounds__(256) void window_kernel(const Op op, FastDiv fd_w, FastDiv fd_h) {
  __shared__ float red[WIN_TY][WIN_TX][4];
  if constexpr (has_lds_tables<Op>::value) op.lds_tables();
  const int tx = threadIdx.x & (WIN_TX - 1), ty = threadIdx.x >> 3;
  const int c = (blockIdx.x * WIN_TX + tx) * 4;
  uint32_t row, iw, n, ih;
  fd_divmod(blockIdx.y, fd_w, row, iw);
  fd_divmod(row, fd_h, n, ih);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (c < op.C) op.cells(n, ih, iw, c, ty, acc);
#pragma unroll
  for (int e = 0; e < 4; ++e) red[ty][tx][e] = acc[e];
  __syncthreads();
  if (ty == 0 && c < op.C) {
    float s[4] = {};
    for (int y = 0; y < WIN_TY; ++y)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += red[y][tx][e];
    store_grad<4>(op.dx + (int64_t)blockIdx.y * op.C + c, s, op.accumulate);
  }
}

// The window kernel's predicate, one for nearest and bilinear: 16-byte channel chunks, at least 64 cells per block of the
// factor (a bilinear dx pixel then has up to 4 sh sw >= 256 taps), and few enough dx pixels for grid.y.
inline bool window_ok(bool vec, int N, int H, int W, int sh, int sw) { return vec && sh * sw >= 64 && (int64_t)N * H * W < 65536; }

template <class Op>
int launch_window(const Op& op, int N, int H, int W, int C, size_t lds_bytes, hipStream_t st, const char* name) {
  hipLaunchKernelGGL((window_kernel<Op>), dim3((unsigned)sg_cdiv(C / 4, WIN_TX), (unsigned)(N * H * W)), dim3(256), lds_bytes, st, op,
                     make_fastdiv((uint32_t)W), make_fastdiv((uint32_t)H));
  SG_LAUNCH_CHECK(name);
  return 0;
}

// ---------------------------------------------------------------------------------------------- pooling
struct PoolGeom {
  int H, W, C, Ho, Wo, k, stride, pad_t, pad_l;
};

template <typename T>
struct PoolParams : PoolGeom {
  const T* __restrict__ x;
  const T* __restrict__ y;
  const T* __restrict__ dy;
  T* __restrict__ out;
};

template <typename T>
struct MaxPoolFwd {
  PoolParams<T> p;
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t oh, uint32_t ow, int c) const {
    float m[V];
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = -INFINITY;
    for (int a = 0; a < p.k; ++a) {
      const int ih = (int)oh * p.stride - p.pad_t + a;
      if ((unsigned)ih >= (unsigned)p.H) continue;
      for (int b = 0; b < p.k; ++b) {
        const int iw = (int)ow * p.stride - p.pad_l + b;
        if ((unsigned)iw >= (unsigned)p.W) continue;
        float xv[V];
        ldv<V>(p.x + ((int64_t)(n * p.H + ih) * p.W + iw) * p.C + c, xv);
#pragma unroll
        for (int k = 0; k < V; ++k) m[k] = fmaxf(m[k], xv[k]);
      }
    }
    stv<V>(p.out + (int64_t)pix * p.C + c, m);
  }
};

// windows (oh, ow) that contain input pixel (ih, iw): oh*s - pt <= ih < oh*s - pt + k, with th = ih + pt, tw = iw + pl
struct PoolWindows {
  int th, tw, oh_lo, oh_hi, ow_lo, ow_hi;
};

__device__ __forceinline__ PoolWindows pool_windows(const PoolGeom& p, int ih, int iw) {
  PoolWindows q;
  q.th = ih + p.pad_t; q.tw = iw + p.pad_l;
  q.oh_hi = q.th / p.stride; q.ow_hi = q.tw / p.stride;
  q.oh_lo = (q.th - p.k + p.stride) / p.stride; q.ow_lo = (q.tw - p.k + p.stride) / p.stride;  // ceil((t-k+1)/s)
  if (q.th - p.k + 1 <= 0) q.oh_lo = 0;
  if (q.tw - p.k + 1 <= 0) q.ow_lo = 0;
  if (q.oh_hi >= p.Ho) q.oh_hi = p.Ho - 1;
  if (q.ow_hi >= p.Wo) q.ow_hi = p.Wo - 1;
  return q;
}

// Gather form (deterministic, no atomics): input element (ih,iw) receives dy of every window in which it is the
// FIRST maximum in window scan order (row-major), which is where TF / Eigen route the gradient.
template <typename T>
struct MaxPoolBwd {
  PoolParams<T> p;
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t ih, uint32_t iw, int c) const {
    float xv[V], acc[V] = {};
    ldv<V>(p.x + (int64_t)pix * p.C + c, xv);
    const PoolWindows q = pool_windows(p, (int)ih, (int)iw);
    for (int oh = q.oh_lo; oh <= q.oh_hi; ++oh) {
      for (int ow = q.ow_lo; ow <= q.ow_hi; ++ow) {
        const int64_t opix = ((int64_t)n * p.Ho + oh) * p.Wo + ow;
        float yv[V], gv[V];
        ldv<V>(p.y + opix * p.C + c, yv);
        ldv<V>(p.dy + opix * p.C + c, gv);
        bool first[V];
#pragma unroll
        for (int k = 0; k < V; ++k) first[k] = (xv[k] == yv[k]);
        // any earlier element of this window (scan order) equal to the max takes precedence
        const int a0 = (int)ih - (oh * p.stride - p.pad_t), b0 = (int)iw - (ow * p.stride - p.pad_l);
        for (int a = 0; a <= a0; ++a) {
          const int jh = oh * p.stride - p.pad_t + a;
          if ((unsigned)jh >= (unsigned)p.H) continue;
          const int bend = (a == a0) ? b0 : p.k;
          for (int b = 0; b < bend; ++b) {
            const int jw = ow * p.stride - p.pad_l + b;
            if ((unsigned)jw >= (unsigned)p.W) continue;
            float ev[V];
            ldv<V>(p.x + ((int64_t)(n * p.H + jh) * p.W + jw) * p.C + c, ev);
#pragma unroll
            for (int k = 0; k < V; ++k) first[k] = first[k] && !(ev[k] == yv[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += first[k] ? gv[k] : 0.f;
      }
    }
    stv<V>(p.out + (int64_t)pix * p.C + c, acc);
  }
};

// Training form (round 3): the forward also writes WHICH cell of the window held the (first) maximum, one byte per output
// element (cell = a * k + b in scan order), and the backward reads that byte and dy instead of x, y and up to eight more x
// values per window: 0.7 GB instead of 1.3 GB of traffic for the 256x256x128 pool of the Xception entry flow and a fraction
// of the loads (MaxPoolBwd: 711 us for a 280 us floor).  Same routing as MaxPoolBwd: strict '>' keeps the first maximum in
// scan order; a window of -inf only (or NaN only) routes to its first valid cell.  (MaxPoolFwd's fmaxf treats a NaN
// differently, and the routing contract rests on this rule, so the two forwards stay two ops.)
template <typename T>
struct MaxPoolFwdIdx {
  PoolParams<T> p;
  unsigned char* __restrict__ idx;
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t oh, uint32_t ow, int c) const {
    float m[V];
    unsigned id[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { m[k] = -INFINITY; id[k] = 255u; }
    for (int a = 0; a < p.k; ++a) {
      const int ih = (int)oh * p.stride - p.pad_t + a;
      if ((unsigned)ih >= (unsigned)p.H) continue;
      for (int b = 0; b < p.k; ++b) {
        const int iw = (int)ow * p.stride - p.pad_l + b;
        if ((unsigned)iw >= (unsigned)p.W) continue;
        float xv[V];
        ldv<V>(p.x + ((int64_t)(n * p.H + ih) * p.W + iw) * p.C + c, xv);
        const unsigned cell = (unsigned)(a * p.k + b);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const bool take = xv[k] > m[k] || id[k] == 255u;
          m[k] = take ? xv[k] : m[k];
          id[k] = take ? cell : id[k];
        }
      }
    }
    stv<V>(p.out + (int64_t)pix * p.C + c, m);
    if constexpr (V == 4) {
      *reinterpret_cast<unsigned*>(idx + (int64_t)pix * p.C + c) = id[0] | (id[1] << 8) | (id[2] << 16) | (id[3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) idx[(int64_t)pix * p.C + c + k] = (unsigned char)id[k];
    }
  }
};

// gather, deterministic: input element (ih, iw) adds dy of every window whose recorded cell is (ih, iw)
template <typename T>
struct MaxPoolBwdIdx {
  PoolParams<T> p;
  const unsigned char* __restrict__ idx;
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t ih, uint32_t iw, int c) const {
    float acc[V] = {};
    const PoolWindows q = pool_windows(p, (int)ih, (int)iw);
    for (int oh = q.oh_lo; oh <= q.oh_hi; ++oh) {
      const unsigned ca = (unsigned)(q.th - oh * p.stride) * (unsigned)p.k;
      for (int ow = q.ow_lo; ow <= q.ow_hi; ++ow) {
        const unsigned cell = ca + (unsigned)(q.tw - ow * p.stride);
        const int64_t o = (((int64_t)n * p.Ho + oh) * p.Wo + ow) * p.C + c;
        float gv[V];
        ldv<V>(p.dy + o, gv);
        if constexpr (V == 4) {
          const unsigned w = *reinterpret_cast<const unsigned*>(idx + o);
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += ((w >> (8 * k)) & 255u) == cell ? gv[k] : 0.f;
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] += (unsigned)idx[o + k] == cell ? gv[k] : 0.f;
        }
      }
    }
    stv<V>(p.out + (int64_t)pix * p.C + c, acc);
  }
};

// AveragePooling2D(k) / GlobalAveragePooling2D as a segmented reduction: segment = output pixel (n,oh,ow),
// rows = kh*kw window cells.
template <typename T>
struct AvgPoolOp {
  static constexpr int NOUT = 1;
  const T* __restrict__ x;
  T* y;
  int H, W, C, Ho, Wo, kh, kw;
  FastDiv fd_howo, fd_wo, fd_kw;
  template <int V>
  __device__ __forceinline__ void accum(int seg, int64_t r, int c, float (&acc)[1][V]) const {
    uint32_t n, rem, oh, ow, a, b;
    fd_divmod((uint32_t)seg, fd_howo, n, rem);
    fd_divmod(rem, fd_wo, oh, ow);
    fd_divmod((uint32_t)r, fd_kw, a, b);
    float xv[V];
    ldv<V>(x + ((int64_t)(n * H + oh * kh + a) * W + ow * kw + b) * C + c, xv);
#pragma unroll
    for (int k = 0; k < V; ++k) acc[0][k] += xv[k];
  }
  __device__ __forceinline__ void finalize(int seg, int c, const double (&s)[1]) const {
    st1<T>(y + (int64_t)seg * C + c, (float)(s[0] / (double)(kh * kw)));
  }
};

template <typename T>
struct AvgPoolBwd {
  const T* __restrict__ dy;
  T* __restrict__ dx;
  int H, W, C, kh, kw, accumulate;
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t ih, uint32_t iw, int c) const {
    const int Ho = H / kh, Wo = W / kw;
    const float sc = 1.0f / (float)(kh * kw);
    const int oh = (int)ih / kh, ow = (int)iw / kw;
    float o[V];
    if (oh < Ho && ow < Wo) {
      ldv<V>(dy + (((int64_t)n * Ho + oh) * Wo + ow) * C + c, o);
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] *= sc;
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = 0.f;
    }
    store_grad<V>(dx + (int64_t)pix * C + c, o, accumulate);
  }
};

// ---------------------------------------------------------------------------------------- nearest up-sampling
template <typename T>
struct UpsampleFwd {
  const T* __restrict__ x;
  T* __restrict__ y;
  int H, W, C, sh, sw, y_ld;
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t oh, uint32_t ow, int c) const {
    float v[V];
    ldv<V>(x + (((int64_t)n * H + oh / sh) * W + ow / sw) * C + c, v);
    stv<V>(y + (int64_t)pix * y_ld + c, v);
  }
};

template <typename T>
struct UpsampleBwd {
  const T* __restrict__ dy;
  T* __restrict__ dx;
  int H, W, C, sh, sw, dy_ld, accumulate;
  FastDiv fd_sw;
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t ih, uint32_t iw, int c) const {
    const int OW = W * sw, OH = H * sh;
    float acc[V] = {};
    for (int a = 0; a < sh; ++a)
      for (int b = 0; b < sw; ++b) {
        float g[V];
        ldv<V>(dy + (((int64_t)n * OH + ih * sh + a) * OW + iw * sw + b) * dy_ld + c, g);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += g[k];
      }
    store_grad<V>(dx + (int64_t)pix * C + c, acc, accumulate);
  }
  __device__ __forceinline__ void cells(uint32_t n, uint32_t ih, uint32_t iw, int c, int ty, f32x4& acc) const {
    const int OW = W * sw, OH = H * sh;
    const T* base = dy + (((int64_t)n * OH + ih * sh) * OW + iw * sw) * dy_ld + c;
#pragma unroll 4
    for (int r = ty; r < sh * sw; r += WIN_TY) {
      uint32_t a, b;
      fd_divmod((uint32_t)r, fd_sw, a, b);
      const f32x4 g = ld4<T>(base + ((int64_t)a * OW + b) * dy_ld);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += g[e];
    }
  }
};

// ---------------------------------------------------------------------------------------- bilinear up-sampling
// tf.image.resize(method='bilinear'), half-pixel centres, integer factor s per axis.  Output o = i * s + p (phase p) sits at
// in = i + t, t = (2p + 1 - s) / (2s) in [-1/2, 1/2):
//   t < 0: lo = max(i - 1, 0), hi = i,                 f = t + 1
//   t > 0: lo = i,             hi = min(i + 1, n - 1), f = t
//   t = 0: lo = hi = i,                                f = 0      (odd s only; s = 1 is a copy)
// so the weights depend on the phase alone and come from a per-axis table built in LDS by every workgroup (one correctly
// rounded division of two small integers per entry; no division per element).
// The tables live in LDS, so a factor is capped (far above any use: the ASPP branch's 32 is the largest known).
#define SG_BILINEAR_MAX_FACTOR 1024

__device__ __forceinline__ float* bilinear_tab() {
  extern __shared__ float tab[];
  return tab;
}

__device__ __forceinline__ float bilinear_phase(int p, int s) {
  const int t2 = 2 * p + 1 - s;
  return (float)(t2 < 0 ? t2 + 2 * s : t2) / (float)(2 * s);
}

__device__ __forceinline__ void bilinear_taps(int i, int p, int s, int n, int& lo, int& hi) {
  const int t2 = 2 * p + 1 - s;
  lo = t2 < 0 ? max(i - 1, 0) : i;
  hi = t2 > 0 ? min(i + 1, n - 1) : i;
}

// One work item = one output pixel x V channels: four loads (the 2 x 2 neighbours, three of them cache hits), columns
// first, then rows (tf's order), one store.
template <typename T>
struct BilinearFwd {
  const T* __restrict__ x;
  T* __restrict__ y;
  int H, W, C, sh, sw, y_ld;
  FastDiv fd_sh, fd_sw;
  __device__ __forceinline__ void lds_tables() const {   // [sh] row phases, then [sw] column phases
    float* tab = bilinear_tab();
    for (int p = threadIdx.x; p < sh + sw; p += blockDim.x) tab[p] = p < sh ? bilinear_phase(p, sh) : bilinear_phase(p - sh, sw);
    __syncthreads();
  }
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t oh, uint32_t ow, int c) const {
    const float* fh = bilinear_tab();
    const float* fw = bilinear_tab() + sh;
    uint32_t ih, ph, iw, pw;
    fd_divmod(oh, fd_sh, ih, ph);
    fd_divmod(ow, fd_sw, iw, pw);
    int h0, h1, w0, w1;
    bilinear_taps((int)ih, (int)ph, sh, H, h0, h1);
    bilinear_taps((int)iw, (int)pw, sw, W, w0, w1);
    const float fy = fh[ph], fx = fw[pw];
    const T* r0 = x + ((int64_t)n * H + h0) * W * C + c;
    const T* r1 = x + ((int64_t)n * H + h1) * W * C + c;
    float tl[V], tr[V], bl[V], br[V], o[V];
    ldv<V>(r0 + (int64_t)w0 * C, tl);
    ldv<V>(r0 + (int64_t)w1 * C, tr);
    ldv<V>(r1 + (int64_t)w0 * C, bl);
    ldv<V>(r1 + (int64_t)w1 * C, br);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float top = fmaf(tr[k] - tl[k], fx, tl[k]), bot = fmaf(br[k] - bl[k], fx, bl[k]);
      o[k] = fmaf(bot - top, fy, top);
    }
    stv<V>(y + (int64_t)pix * y_ld + c, o);
  }
};

// The transpose, as a gather so that no atomics are needed and the order of every sum is fixed (run-to-run bit-identity
// and batch-slice invariance rest on that).  Per axis, dx[i] hears from the outputs o0 + d, o0 = (i - 1) * s + (s + 1) / 2,
// d in [0, 2s - (s & 1)): the upper phases of block i - 1, block i, the lower phases of block i + 1.  Their weight is the
// tent 1 - |in(o) - i| = wt[d], independent of i, except at the borders: outputs clamped onto row 0 / row n - 1 count in
// full.  The table holds the numerators over 2s, each one correctly rounded division.
__device__ __forceinline__ float bilinear_tent(int d, int s) {
  const int orel = d + (s + 1) / 2, blk = orel / s, t2 = 2 * (orel - blk * s) + 1 - s;
  const int num = blk == 0 ? t2 : blk == 1 ? (t2 < 0 ? t2 + 2 * s : 2 * s - t2) : (t2 < 0 ? -t2 : 0);
  return (float)num / (float)(2 * s);
}

__device__ __forceinline__ float bilinear_weight(const float* wt, int d, int o, int i, int n, int s) {
  return ((i == 0 && o < s / 2) || (i == n - 1 && o >= (n - 1) * s + (s + 1) / 2)) ? 1.f : wt[d];
}

// first and one-past-last d of axis position i whose output o0 + d exists
__device__ __forceinline__ void bilinear_span(int i, int n, int s, int& o0, int& d0, int& d1) {
  o0 = (i - 1) * s + (s + 1) / 2;
  d0 = max(0, -o0);
  d1 = min(2 * s - (s & 1), n * s - o0);
}

// apply(): one work item = one dx pixel x V channels; it walks its at most 2 sh x 2 sw outputs rows outer, columns inner.
// cells(): large factors (the ASPP image-pooling branch again: 1x1 -> 32x32) under window_kernel; cell r = row-major index
// in the pixel's span, lane ty takes r = ty, ty + 32, ...
template <typename T>
struct BilinearBwd {
  const T* __restrict__ dy;
  T* __restrict__ dx;
  int H, W, C, sh, sw, dy_ld, accumulate;
  __device__ __forceinline__ void lds_tables() const {   // [2 sh] rows, then [2 sw] columns
    float* tab = bilinear_tab();
    for (int p = threadIdx.x; p < 2 * (sh + sw); p += blockDim.x) tab[p] = p < 2 * sh ? bilinear_tent(p, sh) : bilinear_tent(p - 2 * sh, sw);
    __syncthreads();
  }
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t ih, uint32_t iw, int c) const {
    const float* wth = bilinear_tab();
    const float* wtw = bilinear_tab() + 2 * sh;
    const int OW = W * sw, OH = H * sh;
    int oh0, a0, a1, ow0, b0, b1;
    bilinear_span((int)ih, H, sh, oh0, a0, a1);
    bilinear_span((int)iw, W, sw, ow0, b0, b1);
    float acc[V] = {};
    for (int a = a0; a < a1; ++a) {
      const float wy = bilinear_weight(wth, a, oh0 + a, (int)ih, H, sh);
      const T* rowp = dy + (((int64_t)n * OH + oh0 + a) * OW + ow0) * dy_ld + c;
      for (int b = b0; b < b1; ++b) {
        const float wgt = wy * bilinear_weight(wtw, b, ow0 + b, (int)iw, W, sw);
        float g[V];
        ldv<V>(rowp + (int64_t)b * dy_ld, g);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = fmaf(g[k], wgt, acc[k]);
      }
    }
    store_grad<V>(dx + (int64_t)pix * C + c, acc, accumulate);
  }
  __device__ __forceinline__ void cells(uint32_t n, uint32_t ih, uint32_t iw, int c, int ty, f32x4& acc) const {
    const float* wth = bilinear_tab();
    const float* wtw = bilinear_tab() + 2 * sh;
    const int OW = W * sw, OH = H * sh;
    int oh0, a0, a1, ow0, b0, b1;
    bilinear_span((int)ih, H, sh, oh0, a0, a1);
    bilinear_span((int)iw, W, sw, ow0, b0, b1);
    const int nw = b1 - b0, ncells = (a1 - a0) * nw;
    const T* base = dy + (((int64_t)n * OH + oh0) * OW + ow0) * dy_ld + c;
    int a = a0 + ty / nw, b = b0 + ty % nw;
    for (int r = ty; r < ncells; r += WIN_TY) {
      const float wgt = bilinear_weight(wth, a, oh0 + a, (int)ih, H, sh) * bilinear_weight(wtw, b, ow0 + b, (int)iw, W, sw);
      const f32x4 g = ld4<T>(base + ((int64_t)a * OW + b) * dy_ld);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(g[e], wgt, acc[e]);
      for (b += WIN_TY; b >= b1; b -= nw) ++a;
    }
  }
};

// ---------------------------------------------------------------------------------------- arbitrary-size resize
// sg_resize_fwd / _bwd: any (H, W) -> (OH, OW) with extents up to RS_MAX_EXTENT, by the integer arithmetic of resize_coords.h.
// The per-column (lo, hi, f) of a row depend on neither the row nor the channel, but a table of them would be OW entries of
// eight bytes (up to 128 KB: more than a workgroup's LDS at the largest extent, and a second launch if it lived in a
// workspace), while recomputing them is one multiply-high division by a host-prepared FastDiv and one float division per axis
// per work item, hidden under the four loads.  So the taps are recomputed.  num + den > 0 (num >= n - m > -2m), which makes the
// floor an unsigned division: fl = (num + den) / den - 1.
struct ResizeAxis {
  int n, m;          // input and output extent
  FastDiv fd_2m;     // forward: fl and the nearest source of an output index
  FastDiv fd_2n;     // backward: first() of an input index
  __device__ __forceinline__ RsTap taps(int o) const {
    return rs_taps_from_fl(o, n, m, (int)fd_div((uint32_t)((2 * o + 1) * n + m), fd_2m) - 1);
  }
  __device__ __forceinline__ int nearest(int o) const { return min((int)fd_div((uint32_t)((2 * o + 1) * n), fd_2m), n - 1); }
  __device__ __forceinline__ int first(int k) const { return rs_clamp_first((int)fd_div((uint32_t)rs_first_num(k, n, m), fd_2n), m); }
  __device__ __forceinline__ int nfirst(int i) const { return rs_clamp_first((int)fd_div((uint32_t)rs_nfirst_num(i, n, m), fd_2n), m); }
  // outputs [o0, o1) that can reach input i
  template <int METHOD>
  __device__ __forceinline__ void span(int i, int& o0, int& o1) const {
    if (METHOD == SG_RESIZE_NEAREST) {
      o0 = nfirst(i);
      o1 = nfirst(i + 1);
    } else {
      rs_span_from_first(i, n, m, i == 0 ? 0 : first(i - 1), i == n - 1 ? m : first(i + 1), o0, o1);
    }
  }
};

inline ResizeAxis resize_axis(int n, int m) {
  return ResizeAxis{n, m, make_fastdiv((uint32_t)(2 * m)), make_fastdiv((uint32_t)(2 * n))};
}

// One work item = one output pixel x V channels.  Bilinear: BilinearFwd's four loads and three fmaf, columns first, then rows.
template <typename T, int METHOD>
struct ResizeFwd {
  const T* __restrict__ x;
  T* __restrict__ y;
  int C, y_ld;
  ResizeAxis ah, aw;
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t oh, uint32_t ow, int c) const {
    const int H = ah.n, W = aw.n;
    float o[V];
    if (METHOD == SG_RESIZE_NEAREST) {
      ldv<V>(x + (((int64_t)n * H + ah.nearest((int)oh)) * W + aw.nearest((int)ow)) * C + c, o);
    } else {
      const RsTap th = ah.taps((int)oh), tw = aw.taps((int)ow);
      const float fy = rs_frac(th), fx = rs_frac(tw);
      const T* r0 = x + ((int64_t)n * H + th.lo) * W * C + c;
      const T* r1 = x + ((int64_t)n * H + th.hi) * W * C + c;
      float tl[V], tr[V], bl[V], br[V];
      ldv<V>(r0 + (int64_t)tw.lo * C, tl);
      ldv<V>(r0 + (int64_t)tw.hi * C, tr);
      ldv<V>(r1 + (int64_t)tw.lo * C, bl);
      ldv<V>(r1 + (int64_t)tw.hi * C, br);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float top = fmaf(tr[k] - tl[k], fx, tl[k]), bot = fmaf(br[k] - bl[k], fx, bl[k]);
        o[k] = fmaf(bot - top, fy, top);
      }
    }
    stv<V>(y + (int64_t)pix * y_ld + c, o);
  }
};

// The transpose as a gather: one work item = one dx pixel x V channels walks the outputs of its span, rows outer, columns
// inner, ascending (no atomics; the same bits in every run and for every batch slice).  An empty span (down-sampling) leaves
// dx = 0, or dx as it is under `accumulate`.
template <typename T, int METHOD>
struct ResizeBwd {
  const T* __restrict__ dy;
  T* __restrict__ dx;
  int C, dy_ld, accumulate;
  ResizeAxis ah, aw;
  template <int V>
  __device__ __forceinline__ void apply(uint32_t pix, uint32_t n, uint32_t ih, uint32_t iw, int c) const {
    const int OH = ah.m, OW = aw.m;
    int a0, a1, b0, b1;
    ah.template span<METHOD>((int)ih, a0, a1);
    aw.template span<METHOD>((int)iw, b0, b1);
    T* out = dx + (int64_t)pix * C + c;
    if ((a0 >= a1 || b0 >= b1) && accumulate) return;
    float acc[V] = {};
    for (int a = a0; a < a1; ++a) {
      const float wy = METHOD == SG_RESIZE_NEAREST ? 1.f : rs_weight(ah.taps(a), (int)ih);
      const T* rowp = dy + ((int64_t)n * OH + a) * OW * dy_ld + c;
      for (int b = b0; b < b1; ++b) {
        float g[V];
        ldv<V>(rowp + (int64_t)b * dy_ld, g);
        if (METHOD == SG_RESIZE_NEAREST) {
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] += g[k];
        } else {
          const float wgt = wy * rs_weight(aw.taps(b), (int)iw);
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] = fmaf(g[k], wgt, acc[k]);
        }
      }
    }
    store_grad<V>(out, acc, accumulate);
  }
};

// ------------------------------------------------------------------------------------------------- host checks
// the two sg_resize_* entry points: extents, the wide tensor's pixel stride ld (0 means C), both element counts, the method
int resize_check(const char* who, bool args_ok, int method, int N, int H, int W, int C, int OH, int OW, const char* ld_name, int& ld) {
  SG_CHECK_ARG(args_ok, "%s: null argument", who);
  SG_CHECK_ARG(method == SG_RESIZE_BILINEAR || method == SG_RESIZE_NEAREST, "%s: method %d", who, method);
  SG_CHECK_ARG(N > 0 && C > 0, "%s: N = %d, C = %d", who, N, C);
  SG_CHECK_ARG(H >= 1 && H <= RS_MAX_EXTENT && W >= 1 && W <= RS_MAX_EXTENT && OH >= 1 && OH <= RS_MAX_EXTENT && OW >= 1 &&
                   OW <= RS_MAX_EXTENT,
               "%s: %d x %d -> %d x %d: an extent outside [1, %d]", who, H, W, OH, OW, RS_MAX_EXTENT);
  if (ld == 0) ld = C;
  SG_CHECK_ARG(ld >= C, "%s: %s < C", who, ld_name);
  SG_CHECK_ARG((int64_t)N * H * W * C < (1ll << 31) && (int64_t)N * OH * OW * ld < (1ll << 31), "%s: tensor exceeds 2^31 elements", who);
  return 0;
}

// the four sg_maxpool_* entry points (kmax: the index forms keep the cell in one byte)
int maxpool_check(const char* who, bool args_ok, int N, const PoolGeom& g, int kmax) {
  SG_CHECK_ARG(args_ok, "%s: bad argument", who);
  SG_CHECK_ARG(N > 0 && g.H > 0 && g.W > 0 && g.C > 0 && g.k > 0 && g.k <= kmax && g.stride > 0 && g.Ho > 0 && g.Wo > 0 &&
                   g.pad_t >= 0 && g.pad_l >= 0,
               kmax < INT_MAX ? "%s: bad geometry (windows up to 15 x 15: the cell index is one byte)" : "%s: bad geometry", who);
  SG_CHECK_ARG((int64_t)N * g.H * g.W * g.C < (1ll << 31), "%s: tensor exceeds 2^31 elements", who);
  return 0;
}

int avgpool_check(const char* who, bool args_ok, int N, int H, int W, int C, int kh, int kw) {
  SG_CHECK_ARG(args_ok, "%s: bad argument", who);
  SG_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && kh > 0 && kw > 0 && H >= kh && W >= kw, "%s: bad geometry", who);
  SG_CHECK_ARG((int64_t)N * H * W * C < (1ll << 31), "%s: tensor exceeds 2^31 elements", who);
  return 0;
}

// the four sg_upsample_* entry points: factors (bilinear: at most SG_BILINEAR_MAX_FACTOR), the wide tensor's row stride ld
// (0 means C; `ld_name` for the message) and its size
int upsample_check(const char* who, bool args_ok, int N, int H, int W, int C, int sh, int sw, int max_factor, const char* ld_name,
                   int& ld) {
  SG_CHECK_ARG(args_ok, "%s: bad argument", who);
  SG_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && sh > 0 && sw > 0 && sh <= max_factor && sw <= max_factor, "%s: bad geometry", who);
  if (ld == 0) ld = C;
  SG_CHECK_ARG(ld >= C, "%s: %s < C", who, ld_name);
  SG_CHECK_ARG((int64_t)N * H * sh * W * sw * ld < (1ll << 31), "%s: tensor exceeds 2^31 elements", who);
  return 0;
}

}  // namespace

extern "C" {

int sg_maxpool_fwd(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int k, int stride, int pad_t,
                   int pad_l, int Ho, int Wo, const void* x, void* y) {
  const PoolGeom g = {H, W, C, Ho, Wo, k, stride, pad_t, pad_l};
  if (int rc = maxpool_check("sg_maxpool_fwd", ctx && x && y, N, g, INT_MAX)) return rc;
  const bool vec = (C % 4 == 0) && sg_aligned16(x) && sg_aligned16(y);
  SG_DTYPE_SWITCH(dtype, "sg_maxpool_fwd", {
    const MaxPoolFwd<T> op = {{g, (const T*)x, nullptr, nullptr, (T*)y}};
    return launch_pixels(op, N, Ho, Wo, C, vec, 0, (hipStream_t)stream, "maxpool_fwd");
  });
  return 0;
}

int sg_maxpool_bwd(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int k, int stride, int pad_t,
                   int pad_l, int Ho, int Wo, const void* x, const void* y, const void* dy, void* dx) {
  const PoolGeom g = {H, W, C, Ho, Wo, k, stride, pad_t, pad_l};
  if (int rc = maxpool_check("sg_maxpool_bwd", ctx && x && y && dy && dx, N, g, INT_MAX)) return rc;
  const bool vec = (C % 4 == 0) && sg_aligned16(x) && sg_aligned16(y) && sg_aligned16(dy) && sg_aligned16(dx);
  SG_DTYPE_SWITCH(dtype, "sg_maxpool_bwd", {
    const MaxPoolBwd<T> op = {{g, (const T*)x, (const T*)y, (const T*)dy, (T*)dx}};
    return launch_pixels(op, N, H, W, C, vec, 0, (hipStream_t)stream, "maxpool_bwd");
  });
  return 0;
}

int sg_maxpool_fwd_idx(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int k, int stride, int pad_t,
                       int pad_l, int Ho, int Wo, const void* x, void* y, void* idx) {
  const PoolGeom g = {H, W, C, Ho, Wo, k, stride, pad_t, pad_l};
  if (int rc = maxpool_check("sg_maxpool_fwd_idx", ctx && x && y && idx, N, g, 15)) return rc;
  const bool vec = (C % 4 == 0) && sg_aligned16(x) && sg_aligned16(y) && sg_aligned16(idx);
  SG_DTYPE_SWITCH(dtype, "sg_maxpool_fwd_idx", {
    const MaxPoolFwdIdx<T> op = {{g, (const T*)x, nullptr, nullptr, (T*)y}, (unsigned char*)idx};
    return launch_pixels(op, N, Ho, Wo, C, vec, 0, (hipStream_t)stream, "maxpool_fwd_idx");
  });
  return 0;
}

int sg_maxpool_bwd_idx(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int k, int stride, int pad_t,
                       int pad_l, int Ho, int Wo, const void* dy, const void* idx, void* dx) {
  const PoolGeom g = {H, W, C, Ho, Wo, k, stride, pad_t, pad_l};
  if (int rc = maxpool_check("sg_maxpool_bwd_idx", ctx && dy && idx && dx, N, g, 15)) return rc;
  const bool vec = (C % 4 == 0) && sg_aligned16(dy) && sg_aligned16(dx) && sg_aligned16(idx);
  SG_DTYPE_SWITCH(dtype, "sg_maxpool_bwd_idx", {
    const MaxPoolBwdIdx<T> op = {{g, nullptr, nullptr, (const T*)dy, (T*)dx}, (const unsigned char*)idx};
    return launch_pixels(op, N, H, W, C, vec, 0, (hipStream_t)stream, "maxpool_bwd_idx");
  });
  return 0;
}

size_t sg_avgpool_ws_bytes(const sg_ctx* ctx, int N, int H, int W, int C, int kh, int kw) {
  if (!ctx || kh <= 0 || kw <= 0) return 0;
  const int nseg = N * (H / kh) * (W / kw);
  const SegPlan a = seg_plan<1>(ctx->num_cus, nseg, (int64_t)kh * kw, C, true),
                b = seg_plan<1>(ctx->num_cus, nseg, (int64_t)kh * kw, C, false);
  return (a.part_bytes > b.part_bytes ? a.part_bytes : b.part_bytes) + 256;
}

int sg_avgpool_fwd(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int kh, int kw, const void* x,
                   void* y, void* ws, size_t ws_bytes) {
  if (int rc = avgpool_check("sg_avgpool_fwd", ctx && x && y, N, H, W, C, kh, kw)) return rc;
  SG_DTYPE_SWITCH(dtype, "sg_avgpool_fwd", {
    AvgPoolOp<T> op;
    op.x = (const T*)x; op.y = (T*)y; op.H = H; op.W = W; op.C = C; op.Ho = H / kh; op.Wo = W / kw; op.kh = kh; op.kw = kw;
    op.fd_howo = make_fastdiv((uint32_t)(op.Ho * op.Wo)); op.fd_wo = make_fastdiv((uint32_t)op.Wo); op.fd_kw = make_fastdiv((uint32_t)kw);
    const int nseg = N * op.Ho * op.Wo;
    const bool vec = (C % 4 == 0) && sg_aligned16(x);
    const SegPlan pl = seg_plan<1>(ctx->num_cus, nseg, (int64_t)kh * kw, C, vec);
    if (!ws || ws_bytes < pl.part_bytes) {
      sg_set_error("sg_avgpool_fwd: workspace %zu < %zu", ws_bytes, pl.part_bytes);
      return SG_EWORKSPACE;
    }
    return seg_reduce_launch(op, pl, nseg, (int64_t)kh * kw, C, (float*)ws, (hipStream_t)stream, "avgpool_fwd");
  });
  return 0;
}

int sg_avgpool_bwd(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int kh, int kw, const void* dy,
                   void* dx, int accumulate) {
  if (int rc = avgpool_check("sg_avgpool_bwd", ctx && dy && dx, N, H, W, C, kh, kw)) return rc;
  const bool vec = (C % 4 == 0) && sg_aligned16(dy) && sg_aligned16(dx);
  SG_DTYPE_SWITCH(dtype, "sg_avgpool_bwd", {
    const AvgPoolBwd<T> op = {(const T*)dy, (T*)dx, H, W, C, kh, kw, accumulate};
    return launch_pixels(op, N, H, W, C, vec, 0, (hipStream_t)stream, "avgpool_bwd");
  });
  return 0;
}

int sg_upsample_nearest_fwd(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int sh, int sw,
                            const void* x, void* y, int y_ld) {
  if (int rc = upsample_check("sg_upsample_nearest_fwd", ctx && x && y, N, H, W, C, sh, sw, INT_MAX, "y_ld", y_ld)) return rc;
  const bool vec = (C % 4 == 0) && (y_ld % 4 == 0) && sg_aligned16(x) && sg_aligned16(y);
  SG_DTYPE_SWITCH(dtype, "sg_upsample_nearest_fwd", {
    const UpsampleFwd<T> op = {(const T*)x, (T*)y, H, W, C, sh, sw, y_ld};
    return launch_pixels(op, N, H * sh, W * sw, C, vec, 0, (hipStream_t)stream, "upsample_fwd");
  });
  return 0;
}

int sg_upsample_nearest_bwd(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int sh, int sw,
                            const void* dy, int dy_ld, void* dx, int accumulate) {
  if (int rc = upsample_check("sg_upsample_nearest_bwd", ctx && dy && dx, N, H, W, C, sh, sw, INT_MAX, "dy_ld", dy_ld)) return rc;
  const bool vec = (C % 4 == 0) && (dy_ld % 4 == 0) && sg_aligned16(dy) && sg_aligned16(dx);
  SG_DTYPE_SWITCH(dtype, "sg_upsample_nearest_bwd", {
    const UpsampleBwd<T> op = {(const T*)dy, (T*)dx, H, W, C, sh, sw, dy_ld, accumulate, make_fastdiv((uint32_t)sw)};
    if (window_ok(vec, N, H, W, sh, sw)) return launch_window(op, N, H, W, C, 0, (hipStream_t)stream, "upsample_bwd_window");
    return launch_pixels(op, N, H, W, C, vec, 0, (hipStream_t)stream, "upsample_bwd");
  });
  return 0;
}

int sg_upsample_bilinear_fwd(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int sh, int sw,
                             const void* x, void* y, int y_ld) {
  if (int rc = upsample_check("sg_upsample_bilinear_fwd", ctx && x && y, N, H, W, C, sh, sw, SG_BILINEAR_MAX_FACTOR, "y_ld", y_ld))
    return rc;
  // the vector form under sg_upsample_nearest_fwd's conditions
  const bool vec = (C % 4 == 0) && (y_ld % 4 == 0) && sg_aligned16(x) && sg_aligned16(y);
  const size_t lds = (size_t)(sh + sw) * sizeof(float);
  SG_DTYPE_SWITCH(dtype, "sg_upsample_bilinear_fwd", {
    const BilinearFwd<T> op = {(const T*)x, (T*)y, H, W, C, sh, sw, y_ld, make_fastdiv((uint32_t)sh), make_fastdiv((uint32_t)sw)};
    return launch_pixels(op, N, H * sh, W * sw, C, vec, lds, (hipStream_t)stream, "upsample_bilinear_fwd");
  });
  return 0;
}

int sg_upsample_bilinear_bwd(sg_ctx* ctx, void* stream, int dtype, int N, int H, int W, int C, int sh, int sw,
                             const void* dy, int dy_ld, void* dx, int accumulate) {
  if (int rc = upsample_check("sg_upsample_bilinear_bwd", ctx && dy && dx, N, H, W, C, sh, sw, SG_BILINEAR_MAX_FACTOR, "dy_ld", dy_ld))
    return rc;
  const bool vec = (C % 4 == 0) && (dy_ld % 4 == 0) && sg_aligned16(dy) && sg_aligned16(dx);
  const size_t lds = (size_t)2 * (sh + sw) * sizeof(float);
  SG_DTYPE_SWITCH(dtype, "sg_upsample_bilinear_bwd", {
    const BilinearBwd<T> op = {(const T*)dy, (T*)dx, H, W, C, sh, sw, dy_ld, accumulate};
    if (window_ok(vec, N, H, W, sh, sw)) return launch_window(op, N, H, W, C, lds, (hipStream_t)stream, "upsample_bilinear_bwd_window");
    return launch_pixels(op, N, H, W, C, vec, lds, (hipStream_t)stream, "upsample_bilinear_bwd");
  });
  return 0;
}

int sg_resize_fwd(sg_ctx* ctx, void* stream, int dtype, int method, int N, int H, int W, int C, int OH, int OW, const void* x,
                  void* y, int y_ld) {
  if (int rc = resize_check("sg_resize_fwd", ctx && x && y, method, N, H, W, C, OH, OW, "y_ld", y_ld)) return rc;
  const bool vec = (C % 4 == 0) && (y_ld % 4 == 0) && sg_aligned16(x) && sg_aligned16(y);
  const ResizeAxis ah = resize_axis(H, OH), aw = resize_axis(W, OW);
  SG_DTYPE_SWITCH(dtype, "sg_resize_fwd", {
    if (method == SG_RESIZE_NEAREST) {
      const ResizeFwd<T, SG_RESIZE_NEAREST> op = {(const T*)x, (T*)y, C, y_ld, ah, aw};
      return launch_pixels(op, N, OH, OW, C, vec, 0, (hipStream_t)stream, "resize_nearest_fwd");
    }
    const ResizeFwd<T, SG_RESIZE_BILINEAR> op = {(const T*)x, (T*)y, C, y_ld, ah, aw};
    return launch_pixels(op, N, OH, OW, C, vec, 0, (hipStream_t)stream, "resize_bilinear_fwd");
  });
  return 0;
}

int sg_resize_bwd(sg_ctx* ctx, void* stream, int dtype, int method, int N, int H, int W, int C, int OH, int OW, const void* dy,
                  int dy_ld, void* dx, int accumulate) {
  if (int rc = resize_check("sg_resize_bwd", ctx && dy && dx, method, N, H, W, C, OH, OW, "dy_ld", dy_ld)) return rc;
  const bool vec = (C % 4 == 0) && (dy_ld % 4 == 0) && sg_aligned16(dy) && sg_aligned16(dx);
  const ResizeAxis ah = resize_axis(H, OH), aw = resize_axis(W, OW);
  SG_DTYPE_SWITCH(dtype, "sg_resize_bwd", {
    if (method == SG_RESIZE_NEAREST) {
      const ResizeBwd<T, SG_RESIZE_NEAREST> op = {(const T*)dy, (T*)dx, C, dy_ld, accumulate, ah, aw};
      return launch_pixels(op, N, H, W, C, vec, 0, (hipStream_t)stream, "resize_nearest_bwd");
    }
    const ResizeBwd<T, SG_RESIZE_BILINEAR> op = {(const T*)dy, (T*)dx, C, dy_ld, accumulate, ah, aw};
    return launch_pixels(op, N, H, W, C, vec, 0, (hipStream_t)stream, "resize_bilinear_bwd");
  });
  return 0;
}

}  // extern "C"
