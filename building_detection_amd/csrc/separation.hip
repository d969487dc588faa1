// Distances to the two nearest distinct objects of a label map (sg_object_distances) and the U-Net border weight built on them
// (sg_separation_weights; Ronneberger et al. 2015: w0 * exp(-(d1 + d2)^2 / (2 sigma^2)) on background pixels).  With d2sq == NULL
// the first call is a plain exact Euclidean distance transform.
//
// Exact, in integers.  Take a fixed row y': the pixel of an object in that row that is nearest to (x, y) is the object's pixel
// nearest to column x.  So per row and column it is enough to know the two nearest DISTINCT objects along the row: if an
// object's row-nearest pixel were third in its row, at least one of the two objects in front of it differs from the object that
// realises the image-wide d1sq and is closer, so the third can realise neither d1sq nor d2sq.
//
//   row pass     one wave per row.  A candidate state (nearest labelled column, its object, nearest column of another object,
//                that object) is an associative "nearer segment wins" merge, so a row is scanned in tiles of SEP_WAVE pixels
//                with a shuffle scan inside the tile and a wave-uniform carry between tiles: once left to right, once right to
//                left (the same code on the mirrored column).  The first scan parks its result in the workspace, the second
//                merges both sides and leaves the final two candidates there: two signed 16-bit column offsets in one dword
//                per pixel (|dx| <= 16383 by the ABI's limit on W; SEP_NONE = no candidate).  The object of a candidate is not
//                stored: it is labels[row][x + offset].
//   column pass  one thread per pixel, a wave = SEP_WAVE consecutive x of one row, so every step reads one coalesced dword per
//                lane.  It walks the rows outward from y (dy = 0, 1, ...), keeps the best distance, its object and the best
//                distance of any other object, and stops when dy^2 is no smaller than the second best (the best, without
//                d2sq).  An object is looked up only for a candidate that would improve what is held.
//
// Integer results: the same bits in every run, no atomics.  No kernel waits for another workgroup and none uses LDS.
#include "sg_common.h"

namespace {

constexpr int SEP_WAVE = 64;   // pixels per scan tile of the row pass = columns per workgroup of the column pass (one wave)
constexpr int SEP_ROWS = 4;    // rows per workgroup in both passes, one wave each
constexpr int SEP_NT = SEP_WAVE * SEP_ROWS;
constexpr int SEP_NONE = -32768;         // "no candidate" as a 16-bit offset
constexpr int SEP_INF = 0x7fffffff;
constexpr int SEP_MAX_DIM = 16384;       // |dx| <= 16383 fits 15 bits; 2 * 16383^2 < 2^31

// Scan coordinate u grows in the scan's direction; a state looks back at u' <= u.  p = -1: none.
struct RowState {
  int p1, o1, p2, o2;
};

// `b` covers the columns nearer than those of `a`
template <bool SECOND>
__device__ __forceinline__ RowState row_merge(const RowState& a, const RowState& b) {
  if (b.p1 < 0) return a;
  RowState r = b;
  if (SECOND && b.p2 < 0) {
    if (a.p1 >= 0 && a.o1 != b.o1) { r.p2 = a.p1; r.o2 = a.o1; }
    else if (a.p2 >= 0 && a.o2 != b.o1) { r.p2 = a.p2; r.o2 = a.o2; }
  }
  return r;
}

template <bool SECOND>
__device__ __forceinline__ RowState row_shfl_up(const RowState& s, int off) {
  RowState o;
  o.p1 = __shfl_up(s.p1, off);
  if (SECOND) { o.o1 = __shfl_up(s.o1, off); o.p2 = __shfl_up(s.p2, off); o.o2 = __shfl_up(s.o2, off); }
  else { o.o1 = 0; o.p2 = -1; o.o2 = 0; }
  return o;
}

template <bool SECOND>
__device__ __forceinline__ RowState row_bcast_last(const RowState& s) {
  RowState o;
  o.p1 = __shfl(s.p1, SEP_WAVE - 1);
  if (SECOND) { o.o1 = __shfl(s.o1, SEP_WAVE - 1); o.p2 = __shfl(s.p2, SEP_WAVE - 1); o.o2 = __shfl(s.o2, SEP_WAVE - 1); }
  else { o.o1 = 0; o.p2 = -1; o.o2 = 0; }
  return o;
}

// the state of scan coordinate u = tile * SEP_WAVE + lane (label `lab`, -1 outside the row), the carry of the tiles before it
// merged in; the carry then becomes the last lane's state
template <bool SECOND>
__device__ __forceinline__ RowState row_scan_tile(int u, int lab, int lane, RowState& carry) {
  RowState s = {lab >= 0 ? u : -1, lab, -1, 0};
#pragma unroll
  for (int off = 1; off < SEP_WAVE; off <<= 1) {
    const RowState o = row_shfl_up<SECOND>(s, off);
    if (lane >= off) s = row_merge<SECOND>(o, s);
  }
  s = row_merge<SECOND>(carry, s);
  carry = row_bcast_last<SECOND>(s);
  return s;
}

struct Cand {
  int off, obj;  // off == SEP_NONE: none
};

__device__ __forceinline__ int cand_dist(const Cand& c) { return c.off < 0 ? -c.off : c.off; }  // SEP_NONE -> 32768: beyond all

__device__ __forceinline__ Cand cand_nearer(const Cand& a, const Cand& b) { return cand_dist(b) < cand_dist(a) ? b : a; }

// the nearest candidate of one side whose object is not `obj`: the first unless it is `obj` itself, then the second
__device__ __forceinline__ Cand cand_other(const Cand& c1, const Cand& c2, int obj) {
  return (c1.off != SEP_NONE && c1.obj == obj) ? c2 : c1;
}

__device__ __forceinline__ unsigned cand_pack(int off1, int off2) { return ((unsigned)off1 & 0xffffu) | ((unsigned)off2 << 16); }
__device__ __forceinline__ int cand_lo(unsigned c) { return (int)(short)(c & 0xffffu); }
__device__ __forceinline__ int cand_hi(unsigned c) { return (int)(short)(c >> 16); }

template <bool SECOND>
__global__ __launch_bounds__(SEP_NT) void sep_row_kernel(const int* __restrict__ labels, unsigned* cand, int64_t rows, int W) {
  const int lane = threadIdx.x & (SEP_WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * SEP_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;  // whole waves leave; nothing below synchronises the workgroup
  const int* __restrict__ L = labels + row * W;
  unsigned* c = cand + row * W;
  const int tiles = (W + SEP_WAVE - 1) / SEP_WAVE;
  // left to right: u = x; offsets <= 0
  RowState carry = {-1, 0, -1, 0};
  for (int t = 0; t < tiles; ++t) {
    const int x = t * SEP_WAVE + lane;
    const RowState s = row_scan_tile<SECOND>(x, x < W ? L[x] : -1, lane, carry);
    if (x < W) c[x] = cand_pack(s.p1 >= 0 ? s.p1 - x : SEP_NONE, (SECOND && s.p2 >= 0) ? s.p2 - x : SEP_NONE);
  }
  __threadfence();  // the second scan reads the parked states through other lanes of this wave
  // right to left: u = W - 1 - x; offsets >= 0
  carry = {-1, 0, -1, 0};
  for (int t = 0; t < tiles; ++t) {
    const int u = t * SEP_WAVE + lane;
    const int x = W - 1 - u;
    const RowState s = row_scan_tile<SECOND>(u, x >= 0 ? L[x] : -1, lane, carry);
    if (x < 0) continue;
    const unsigned left = __hip_atomic_load(&c[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // from L2, where the fence put it
    Cand l1 = {cand_lo(left), 0}, l2 = {cand_hi(left), 0};
    Cand r1 = {s.p1 >= 0 ? u - s.p1 : SEP_NONE, s.o1}, r2 = {s.p2 >= 0 ? u - s.p2 : SEP_NONE, s.o2};
    if (!SECOND) {
      c[x] = cand_pack(cand_nearer(l1, r1).off, SEP_NONE);
      continue;
    }
    if (l1.off != SEP_NONE) l1.obj = L[x + l1.off];
    if (l2.off != SEP_NONE) l2.obj = L[x + l2.off];
    Cand first, second;
    if (cand_dist(l1) <= cand_dist(r1)) {  // both none: first = none, and so is everything else
      first = l1;
      second = cand_nearer(l2, cand_other(r1, r2, l1.obj));
    } else {
      first = r1;
      second = cand_nearer(r2, cand_other(l1, l2, r1.obj));
    }
    c[x] = cand_pack(first.off, second.off);
  }
}

template <bool SECOND>
__global__ __launch_bounds__(SEP_NT) void sep_col_kernel(const int* __restrict__ labels, const unsigned* __restrict__ cand, int H,
                                                         int W, int tiles_x, int tiles_y, int* __restrict__ d1sq,
                                                         int* __restrict__ d2sq) {
  const int lane = threadIdx.x & (SEP_WAVE - 1);
  const unsigned b = blockIdx.x;
  const unsigned per_image = (unsigned)tiles_x * (unsigned)tiles_y;
  const unsigned n = b / per_image, rem = b - n * per_image;
  const int ty = (int)(rem / (unsigned)tiles_x), tx = (int)(rem - (unsigned)ty * (unsigned)tiles_x);
  const int x = tx * SEP_WAVE + lane, y = ty * SEP_ROWS + (int)(threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const int64_t img = (int64_t)n * H * W;  // rows of another image are never visited
  const unsigned* __restrict__ C = cand + img + x;
  const int* __restrict__ L = labels + img + x;
  int best1 = SEP_INF, best2 = SEP_INF, obj1 = -1;
  auto take = [&](int d, int o) {  // d < best2
    if (d < best1) {
      if (o != obj1) best2 = best1;
      best1 = d;
      obj1 = o;
    } else if (o != obj1) {
      best2 = d;
    }
  };
  auto visit = [&](int r, int dy2) {
    const int64_t at = (int64_t)r * W;
    const unsigned c = C[at];
    const int off1 = cand_lo(c);
    if (off1 == SEP_NONE) return;
    const int da = off1 * off1 + dy2;
    if (!SECOND) {
      best1 = da < best1 ? da : best1;
      return;
    }
    if (da < best2) take(da, L[at + off1]);
    const int off2 = cand_hi(c);
    if (off2 == SEP_NONE) return;
    const int db = off2 * off2 + dy2;
    if (db < best2) take(db, L[at + off2]);
  };
  for (int dy = 0; dy < H; ++dy) {
    const int dy2 = dy * dy;
    if (dy2 >= (SECOND ? best2 : best1)) break;
    const bool up = y - dy >= 0, down = dy > 0 && y + dy < H;
    if (!up && !down) break;
    if (up) visit(y - dy, dy2);
    if (down) visit(y + dy, dy2);
  }
  const int64_t i = img + (int64_t)y * W + x;
  d1sq[i] = best1;
  if (SECOND) d2sq[i] = best2;
}

__global__ __launch_bounds__(SEP_NT) void sep_weight_kernel(const int* __restrict__ d1sq, const int* __restrict__ d2sq, int64_t n,
                                                            float w0, float sigma, float* __restrict__ y4) {
  const int64_t i = (int64_t)blockIdx.x * SEP_NT + threadIdx.x;
  if (i >= n) return;
  const int a = d1sq[i], b = d2sq[i];
  if (a <= 0 || b == SEP_INF) return;
  const float s = sqrtf((float)a) + sqrtf((float)b);
  const float t = w0 * expf(-(s * s) / (2.0f * sigma * sigma));
  if (t != 0.0f) y4[i * 4 + 2] += t;  // adding +0 changes no bit of a weight: leave the pixel alone
}

inline size_t sep_align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline bool sep_shape_ok(int N, int H, int W) {
  return N > 0 && H >= 1 && W >= 1 && H <= SEP_MAX_DIM && W <= SEP_MAX_DIM && (int64_t)N * H * W < (1ll << 31);
}

}  // namespace

extern "C" {

size_t sg_object_distances_ws_bytes(int N, int H, int W) {
  if (!sep_shape_ok(N, H, W)) return 0;
  return sep_align256((size_t)N * H * W * sizeof(unsigned));  // one dword per pixel: two 16-bit column offsets
}

int sg_object_distances(sg_ctx* ctx, void* stream, int N, int H, int W, const void* labels_i32, void* ws, size_t ws_bytes,
                        void* d1sq_i32, void* d2sq_i32) {
  SG_CHECK_ARG(ctx && labels_i32 && ws && d1sq_i32, "sg_object_distances: bad argument");
  SG_CHECK_ARG(sep_shape_ok(N, H, W), "sg_object_distances: N %d, H %d, W %d (1 <= H, W <= %d, N*H*W < 2^31)", N, H, W, SEP_MAX_DIM);
  if (ws_bytes < sg_object_distances_ws_bytes(N, H, W)) {
    sg_set_error("sg_object_distances: workspace %zu < %zu", ws_bytes, sg_object_distances_ws_bytes(N, H, W));
    return SG_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)N * H;
  const unsigned row_blocks = (unsigned)((rows + SEP_ROWS - 1) / SEP_ROWS);
  const int tiles_x = (W + SEP_WAVE - 1) / SEP_WAVE, tiles_y = (H + SEP_ROWS - 1) / SEP_ROWS;
  const unsigned col_blocks = (unsigned)((int64_t)N * tiles_x * tiles_y);  // <= N*H*W < 2^31
  const int* L = (const int*)labels_i32;
  unsigned* c = (unsigned*)ws;
  if (d2sq_i32) {
    hipLaunchKernelGGL(sep_row_kernel<true>, dim3(row_blocks), dim3(SEP_NT), 0, st, L, c, rows, W);
    hipLaunchKernelGGL(sep_col_kernel<true>, dim3(col_blocks), dim3(SEP_NT), 0, st, L, (const unsigned*)c, H, W, tiles_x, tiles_y,
                       (int*)d1sq_i32, (int*)d2sq_i32);
  } else {
    hipLaunchKernelGGL(sep_row_kernel<false>, dim3(row_blocks), dim3(SEP_NT), 0, st, L, c, rows, W);
    hipLaunchKernelGGL(sep_col_kernel<false>, dim3(col_blocks), dim3(SEP_NT), 0, st, L, (const unsigned*)c, H, W, tiles_x, tiles_y,
                       (int*)d1sq_i32, (int*)nullptr);
  }
  SG_LAUNCH_CHECK("sg_object_distances");
  return 0;
}

int sg_separation_weights(sg_ctx* ctx, void* stream, int N, int H, int W, const void* d1sq_i32, const void* d2sq_i32, float w0,
                          float sigma, void* y_true4) {
  SG_CHECK_ARG(ctx && d1sq_i32 && d2sq_i32 && y_true4, "sg_separation_weights: bad argument");
  SG_CHECK_ARG(sep_shape_ok(N, H, W), "sg_separation_weights: N %d, H %d, W %d (1 <= H, W <= %d, N*H*W < 2^31)", N, H, W,
               SEP_MAX_DIM);
  SG_CHECK_ARG(w0 >= 0.0f && w0 <= 3.402823466e38f && sigma > 0.0f && sigma <= 3.402823466e38f,
               "sg_separation_weights: w0 %g, sigma %g (w0 >= 0, sigma > 0, both finite)", (double)w0, (double)sigma);
  const int64_t n = (int64_t)N * H * W;
  hipLaunchKernelGGL(sep_weight_kernel, dim3((unsigned)((n + SEP_NT - 1) / SEP_NT)), dim3(SEP_NT), 0, (hipStream_t)stream,
                     (const int*)d1sq_i32, (const int*)d2sq_i32, n, w0, sigma, (float*)y_true4);
  SG_LAUNCH_CHECK("sg_separation_weights");
  return 0;
}

}  // extern "C"
