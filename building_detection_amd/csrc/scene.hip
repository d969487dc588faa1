// Soft scene inference (include/segengine.h, "inference tail"): the device tile cutter, the probability-domain stitch and
// its finalisation.  The item table travels by value in the kernel-argument segment (as AugTable does in train.hip): an
// item index is uniform in a wave, so reading an item is scalar work.
//
// The tile <-> window map is defined once (tile_to_win / win_to_tile) and used by both kernels: for tile coordinate (r, c)
// of a T x T tile, (a, b) = transpose ? (c, r) : (r, c), u = flip_ud ? T-1-a : a, v = flip_lr ? T-1-b : b, and the tile
// element corresponds to scene / canvas pixel (y0+u, x0+v).  A window is the T x T square at (y0, x0) under every symmetry.
#include "sg_common.h"
#include "resize_coords.h"

namespace {

struct SceneTable {
  sg_scene_item it[SG_SCENE_MAX_ITEMS];
};

__device__ __forceinline__ void tile_to_win(int sym, int T, int r, int c, int& u, int& v) {
  const int a = (sym & SG_SYM_TRANSPOSE) ? c : r, b = (sym & SG_SYM_TRANSPOSE) ? r : c;
  u = (sym & SG_SYM_FLIP_UD) ? T - 1 - a : a;
  v = (sym & SG_SYM_FLIP_LR) ? T - 1 - b : b;
}

// the inverse: a flip is its own inverse, the swap follows the un-flipping
__device__ __forceinline__ void win_to_tile(int sym, int T, int u, int v, int& r, int& c) {
  const int a = (sym & SG_SYM_FLIP_UD) ? T - 1 - u : u, b = (sym & SG_SYM_FLIP_LR) ? T - 1 - v : v;
  r = (sym & SG_SYM_TRANSPOSE) ? b : a;
  c = (sym & SG_SYM_TRANSPOSE) ? a : b;
}

// np.float32(np.float64(s) / 127.5 - 1): the division and the subtraction in double, one rounding to float
__device__ __forceinline__ float scene_value(unsigned char s) { return (float)((double)s / 127.5 - 1.0); }

// One tile per blockIdx.y; a thread computes SCENE_PX consecutive pixels of one tile row and writes their 12 floats as three
// 16-byte stores (VEC: T % 4 == 0 and a 16-byte aligned output, so every group of four pixels starts 48-byte aligned) or
// float by float.  The transposed symmetries read down a column of the uint8 scene, which stays in L2 / the Infinity Cache.
// All indices fit 32 bits (the host bounds both tensors below 2 GiB).
constexpr int SCENE_PX = 4;

template <bool VEC>
__global__ __launch_bounds__(256) void scene_tiles_kernel(const unsigned char* __restrict__ scene, float* __restrict__ tiles,
                                                          const SceneTable tab, int H, int W, int T, int qw) {
  const sg_scene_item it = tab.it[blockIdx.y];
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= T * qw) return;
  const int r = t / qw;
  const int c0 = (t - r * qw) * SCENE_PX;
  float val[SCENE_PX * 3];
#pragma unroll
  for (int k = 0; k < SCENE_PX; ++k) {
    const int c = c0 + k;
    int u, v;
    tile_to_win(it.sym, T, r, c, u, v);
    const int y = it.y0 + u, x = it.x0 + v;
    const bool in = c < T && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    const int s = in ? (y * W + x) * 3 : 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) val[k * 3 + ch] = in ? scene_value(scene[s + ch]) : 0.0f;
  }
  const int off = (((int)blockIdx.y * T + r) * T + c0) * 3;
  if (VEC) {
    f32x4* __restrict__ d = reinterpret_cast<f32x4*>(tiles + off);
#pragma unroll
    for (int j = 0; j < 3; ++j) d[j] = (f32x4){val[4 * j], val[4 * j + 1], val[4 * j + 2], val[4 * j + 3]};
  } else {
    const int nf = min(SCENE_PX, T - c0) * 3;
#pragma unroll
    for (int b = 0; b < SCENE_PX * 3; ++b)
      if (b < nf) tiles[off + b] = val[b];
  }
}

// grid = (floats of a T x T x C window, item j).  The thread of window position (u, v) and class k owns canvas element
// (y0_j+u, x0_j+v, k) if j is the lowest-index item of the table whose window covers that pixel; otherwise the owner sits in
// an earlier item's part of the grid and this thread leaves.  The owner then walks the items j ... N-1 that cover the pixel,
// in table order, with the running value in a register, and stores once: no atomics, a fixed order, and work proportional to
// the items (never to the canvas).  The coverage tests compare a thread's pixel with table entries read by a uniform index.
// Consecutive threads are consecutive canvas floats, and consecutive floats of p for the un-transposed symmetries; the
// thread of class 0 also carries wsum.  PAIR (C = 2, 8-byte aligned p and acc): one thread per pixel, both classes as one
// 8-byte access.
template <bool PAIR>
__global__ __launch_bounds__(256) void prob_accumulate_kernel(const float* __restrict__ p, const float* __restrict__ win,
                                                              float* __restrict__ acc, float* __restrict__ wsum,
                                                              const SceneTable tab, int N, int C, int T, FastDiv dC, FastDiv dT,
                                                              float scale, int CH, int CW) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const int j = (int)blockIdx.y;
  const sg_scene_item me = tab.it[j];
  // all symmetries of one tile share a window: the first of them owns all of it (a uniform exit for the others)
  for (int i = 0; i < j; ++i)
    if (tab.it[i].y0 == me.y0 && tab.it[i].x0 == me.x0) return;
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (uint32_t)T * (uint32_t)T * (uint32_t)(PAIR ? 1 : C)) return;
  uint32_t q = e, k = 0, u, v;
  if (!PAIR) fd_divmod(e, dC, q, k);
  fd_divmod(q, dT, u, v);
  const int y = me.y0 + (int)u, x = me.x0 + (int)v;   // |y0| < 2^30 and CH < 2^30: every difference below fits an int
  if ((unsigned)y >= (unsigned)CH || (unsigned)x >= (unsigned)CW) return;
  for (int i = 0; i < j; ++i) {
    const sg_scene_item o = tab.it[i];
    if ((unsigned)(y - o.y0) < (unsigned)T && (unsigned)(x - o.x0) < (unsigned)T) return;
  }
  const int64_t pix = (int64_t)y * CW + x;
  float* __restrict__ dst = acc + pix * C + k;
  float a0, a1 = 0.f, ws = 0.f;
  if (PAIR) {
    const f32x2 t = *reinterpret_cast<const f32x2*>(dst);
    a0 = t[0];
    a1 = t[1];
  } else {
    a0 = *dst;
  }
  if (k == 0) ws = wsum[pix];
  for (int i = j; i < N; ++i) {
    const sg_scene_item o = tab.it[i];
    const int uu = y - o.y0, vv = x - o.x0;
    if ((unsigned)uu >= (unsigned)T || (unsigned)vv >= (unsigned)T) continue;
    const float w = __fmul_rn(__fmul_rn(scale, win[uu]), win[vv]);   // never contracted into the sums below
    int r, c;
    win_to_tile(o.sym, T, uu, vv, r, c);
    const float* __restrict__ src = p + (((int64_t)i * T + r) * T + c) * C + k;
    if (PAIR) {
      const f32x2 t = *reinterpret_cast<const f32x2*>(src);
      a0 = fmaf(w, t[0], a0);
      a1 = fmaf(w, t[1], a1);
    } else {
      a0 = fmaf(w, *src, a0);
    }
    ws = __fadd_rn(ws, w);
  }
  if (PAIR)
    *reinterpret_cast<f32x2*>(dst) = (f32x2){a0, a1};
  else
    *dst = a0;
  if (k == 0) wsum[pix] = ws;
}

// One thread per canvas pixel: the first maximum of acc[pixel, :] (strict >: ties go to the lowest index), then the
// quotients.  probs may be acc itself: a thread reads an element before it writes it and touches no other pixel.
__global__ __launch_bounds__(256) void prob_finalize_kernel(const float* acc, const float* __restrict__ wsum, float* probs,
                                                            unsigned char* __restrict__ map, int64_t npix, int C, int out_scale) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
    const float ws = wsum[i];
    const float* a = acc + i * C;
    float best = a[0];
    int q = 0;
    for (int k = 1; k < C; ++k) {
      const float t = a[k];
      if (t > best) {
        best = t;
        q = k;
      }
    }
    const bool reached = ws != 0.f;
    map[i] = reached ? (unsigned char)(out_scale * q) : (unsigned char)0;
    if (probs) {
      float* d = probs + i * C;
      for (int k = 0; k < C; ++k) d[k] = reached ? a[k] / ws : 0.f;
    }
  }
}

// One thread per base canvas element (y, x, k): blockIdx.y is the canvas row (CH <= 16384), the x grid covers the row's CW * C
// floats.  The bilinear taps of resize_coords.h from the scaled canvases (HS, WS) to the base ones (CH, CW), each tap
// normalised by its own wsum_s before the blend (a pixel the scaled pass never reached counts as probability 0), the blend in
// sg_resize_fwd's order, one fma into acc.  The thread of class 0 carries wsum.  Canvas offsets are 64-bit.
__global__ __launch_bounds__(256) void prob_resize_accumulate_kernel(const float* __restrict__ acc_s, const float* __restrict__ wsum_s,
                                                                     float* __restrict__ acc, float* __restrict__ wsum, int C, int HS,
                                                                     int WS, int CH, int CW, float weight, FastDiv dC, FastDiv d2h,
                                                                     FastDiv d2w) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (uint32_t)CW * (uint32_t)C) return;   // < 16384 * 32
  const int y = (int)blockIdx.y;
  uint32_t x, k;
  fd_divmod(j, dC, x, k);
  const RsTap th = rs_taps_from_fl(y, HS, CH, (int)fd_div((uint32_t)((2 * y + 1) * HS + CH), d2h) - 1);
  const RsTap tw = rs_taps_from_fl((int)x, WS, CW, (int)fd_div((uint32_t)((2 * (int)x + 1) * WS + CW), d2w) - 1);
  const float fy = rs_frac(th), fx = rs_frac(tw);
  float q[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int64_t sp = (int64_t)(a ? th.hi : th.lo) * WS + (b ? tw.hi : tw.lo);
      const float ws = wsum_s[sp];
      q[a][b] = ws > 0.f ? __fdiv_rn(acc_s[sp * C + k], ws) : 0.f;
    }
  const float top = fmaf(q[0][1] - q[0][0], fx, q[0][0]), bot = fmaf(q[1][1] - q[1][0], fx, q[1][0]);
  const float v = fmaf(bot - top, fy, top);
  const int64_t pix = (int64_t)y * CW + x;
  acc[pix * C + k] = fmaf(weight, v, acc[pix * C + k]);
  if (k == 0) wsum[pix] = __fadd_rn(wsum[pix], weight);
}

// the checks both table-taking entry points share; fills `tab`
inline int scene_table(const char* who, int N, const sg_scene_item* items, SceneTable& tab) {
  SG_CHECK_ARG(N >= 1 && N <= SG_SCENE_MAX_ITEMS, "%s: N = %d outside [1, %d]", who, N, SG_SCENE_MAX_ITEMS);
  SG_CHECK_ARG(items, "%s: null item table", who);
  const int lim = 1 << 30;
  for (int i = 0; i < N; ++i) {
    const sg_scene_item& a = items[i];
    SG_CHECK_ARG(a.sym >= 0 && a.sym < 8, "%s: item %d: symmetry %d outside [0, 8)", who, i, a.sym);
    SG_CHECK_ARG(a.reserved == 0, "%s: item %d: reserved = %d, not 0", who, i, a.reserved);
    SG_CHECK_ARG(a.y0 > -lim && a.y0 < lim && a.x0 > -lim && a.x0 < lim, "%s: item %d: origin (%d, %d) beyond 2^30", who, i, a.y0,
                 a.x0);
    tab.it[i] = a;
  }
  for (int i = N; i < SG_SCENE_MAX_ITEMS; ++i) tab.it[i] = sg_scene_item{0, 0, 0, 0};
  return 0;
}

}  // namespace

extern "C" {

int sg_scene_tiles_u8(sg_ctx* ctx, void* stream, int H, int W, const void* scene_u8, int N, const sg_scene_item* items, int T,
                      void* tiles_f32) {
  SG_CHECK_ARG(ctx && scene_u8 && tiles_f32, "sg_scene_tiles_u8: null argument");
  SG_CHECK_ARG(H > 0 && W > 0 && T > 0, "sg_scene_tiles_u8: scene %d x %d, tile %d", H, W, T);
  SceneTable tab;
  if (const int rc = scene_table("sg_scene_tiles_u8", N, items, tab)) return rc;
  SG_CHECK_ARG((int64_t)H * W * 3 < (1ll << 31) && (int64_t)N * T * T * 3 * 4 < (1ll << 31),
               "sg_scene_tiles_u8: a scene of %d x %d x 3 bytes / %d tiles of %d x %d x 3 floats exceed 2 GiB", H, W, N, T, T);
  const int qw = (int)sg_cdiv(T, SCENE_PX);
  const dim3 grid((unsigned)sg_cdiv((int64_t)T * qw, 256), (unsigned)N);
  if (T % SCENE_PX == 0 && ((uintptr_t)tiles_f32 & 15) == 0)
    hipLaunchKernelGGL(scene_tiles_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)scene_u8,
                       (float*)tiles_f32, tab, H, W, T, qw);
  else
    hipLaunchKernelGGL(scene_tiles_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)scene_u8,
                       (float*)tiles_f32, tab, H, W, T, qw);
  SG_LAUNCH_CHECK("scene_tiles_kernel");
  return 0;
}

int sg_prob_accumulate(sg_ctx* ctx, void* stream, int C, int T, const void* p_f32, int N, const sg_scene_item* items,
                       const void* win_f32, float scale, void* acc_f32, void* wsum_f32, int CH, int CW) {
  SG_CHECK_ARG(ctx && p_f32 && win_f32 && acc_f32 && wsum_f32, "sg_prob_accumulate: null argument");
  SG_CHECK_ARG(C >= 2 && C <= SG_MAX_CLASSES, "sg_prob_accumulate: C = %d outside [2, %d]", C, SG_MAX_CLASSES);
  SG_CHECK_ARG(T > 0 && (int64_t)T * T * C < (1ll << 31), "sg_prob_accumulate: a tile of %d x %d x %d", T, T, C);
  SG_CHECK_ARG(CH > 0 && CW > 0 && CH < (1 << 30) && CW < (1 << 30), "sg_prob_accumulate: a canvas of %d x %d", CH, CW);
  SceneTable tab;
  if (const int rc = scene_table("sg_prob_accumulate", N, items, tab)) return rc;
  const bool pair = C == 2 && (((uintptr_t)p_f32 | (uintptr_t)acc_f32) & 7) == 0;
  const dim3 grid((unsigned)sg_cdiv((int64_t)T * T * (pair ? 1 : C), 256), (unsigned)N);
  const FastDiv dC = make_fastdiv((uint32_t)C), dT = make_fastdiv((uint32_t)T);
  if (pair)
    hipLaunchKernelGGL(prob_accumulate_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)p_f32,
                       (const float*)win_f32, (float*)acc_f32, (float*)wsum_f32, tab, N, C, T, dC, dT, scale, CH, CW);
  else
    hipLaunchKernelGGL(prob_accumulate_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)p_f32,
                       (const float*)win_f32, (float*)acc_f32, (float*)wsum_f32, tab, N, C, T, dC, dT, scale, CH, CW);
  SG_LAUNCH_CHECK("prob_accumulate_kernel");
  return 0;
}

int sg_prob_finalize(sg_ctx* ctx, void* stream, int C, const void* acc_f32, const void* wsum_f32, int CH, int CW,
                     void* probs_out_f32, int out_scale, void* map_u8) {
  SG_CHECK_ARG(ctx && acc_f32 && wsum_f32 && map_u8, "sg_prob_finalize: null argument");
  SG_CHECK_ARG(C >= 2 && C <= SG_MAX_CLASSES, "sg_prob_finalize: C = %d outside [2, %d]", C, SG_MAX_CLASSES);
  SG_CHECK_ARG(CH > 0 && CW > 0, "sg_prob_finalize: a canvas of %d x %d", CH, CW);
  SG_CHECK_ARG(out_scale >= 1 && out_scale <= 255 / (C - 1), "sg_prob_finalize: out_scale %d times class %d does not fit a byte",
               out_scale, C - 1);
  const int64_t npix = (int64_t)CH * CW;
  int64_t blocks = sg_cdiv(npix, 256);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(prob_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)acc_f32,
                     (const float*)wsum_f32, (float*)probs_out_f32, (unsigned char*)map_u8, npix, C, out_scale);
  SG_LAUNCH_CHECK("prob_finalize_kernel");
  return 0;
}

int sg_prob_resize_accumulate(sg_ctx* ctx, void* stream, int C, const void* acc_s_f32, const void* wsum_s_f32, int HS, int WS,
                              float weight, void* acc_f32, void* wsum_f32, int CH, int CW) {
  SG_CHECK_ARG(ctx && acc_s_f32 && wsum_s_f32 && acc_f32 && wsum_f32, "sg_prob_resize_accumulate: null argument");
  SG_CHECK_ARG(C >= 2 && C <= SG_MAX_CLASSES, "sg_prob_resize_accumulate: C = %d outside [2, %d]", C, SG_MAX_CLASSES);
  SG_CHECK_ARG(HS >= 1 && HS <= RS_MAX_EXTENT && WS >= 1 && WS <= RS_MAX_EXTENT && CH >= 1 && CH <= RS_MAX_EXTENT && CW >= 1 &&
                   CW <= RS_MAX_EXTENT,
               "sg_prob_resize_accumulate: %d x %d -> %d x %d: an extent outside [1, %d]", HS, WS, CH, CW, RS_MAX_EXTENT);
  SG_CHECK_ARG(weight > 0.f && weight <= 3.402823466e38f, "sg_prob_resize_accumulate: weight %g is not positive and finite",
               (double)weight);
  const dim3 grid((unsigned)sg_cdiv((int64_t)CW * C, 256), (unsigned)CH);
  hipLaunchKernelGGL(prob_resize_accumulate_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float*)acc_s_f32,
                     (const float*)wsum_s_f32, (float*)acc_f32, (float*)wsum_f32, C, HS, WS, CH, CW, weight,
                     make_fastdiv((uint32_t)C), make_fastdiv((uint32_t)(2 * CH)), make_fastdiv((uint32_t)(2 * CW)));
  SG_LAUNCH_CHECK("prob_resize_accumulate_kernel");
  return 0;
}

}  // extern "C"
