// Lovasz-Softmax loss on the C-class head, alone or added to one of the three pointwise losses of multiclass.hip (DESIGN 4.12;
// the definition is in include/segengine.h).  A segment is one (group, class): s = g * C + c, rows_per_image elements long.
//   lv_key_kernel     one pass over p and y_true: per (row, class) the 30-bit key 0x3F800000 - bits(m) and the payload
//                     {global pixel index, foreground flag in bit 31} -> the segment's slot of the row; the pointwise row sums
//                     -> one partial per workgroup
//   sort_pairs_run    sort.hip's passes, ping-pong between the two buffer pairs of the workspace (four passes for 30 bits)
//   lv_count_kernel   per tile of SG_SORT_TILE sorted elements the number of foreground flags (a ballot count, no atomics)
//   lv_scan_kernel    per segment the exclusive scan of the tile counts in place, and G
//   lv_grad_kernel    per tile: F_k from the tile's base, ballots and the fixed order wave -> round -> lane; g_k in double from
//                     the integer counts, rounded once; +-g_k / (images n_c) scattered to g_out[pixel, c]; m of the unclamped
//                     p gathered from the same place; the tile's sum of m g_k in double, folded in a fixed order
//   lv_seg_kernel     per segment the sum of its tiles' partials, in double in a fixed order
//   lv_final_kernel   one workgroup: the pointwise partials and the groups' sums -> {L, L_point, L_lovasz}
//   lv_bwd_kernel     dp = grad_scale * (point_weight * pointwise gradient + lovasz_weight * g)
// A double is kept in the workspace as two words, so 4-byte alignment is enough for every pointer.  No float atomics, no
// allocation, no synchronisation: the same bits from run to run, and every launch is a kernel node.
#include "loss_head.h"
#include "sort_impl.h"

namespace {

constexpr int MAX_IMAGES = 65535;
constexpr uint32_t ONE_BITS = 0x3f800000u;
constexpr uint32_t FG_BIT = 0x80000000u;

__device__ __forceinline__ void put_double(uint32_t* __restrict__ w, double v) {
  w[0] = (uint32_t)__double2loint(v);
  w[1] = (uint32_t)__double2hiint(v);
}

__device__ __forceinline__ double get_double(const uint32_t* __restrict__ w) { return __hiloint2double((int)w[1], (int)w[0]); }

template <int CM, bool EX>
__global__ __launch_bounds__(256) void lv_key_kernel(int kind, int64_t rows, int64_t n, int C, int y_cols, const ClassVec al,
                                                     const float* __restrict__ p, const float* __restrict__ yt,
                                                     uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                     float* __restrict__ part) {
  if (EX) C = CM;
  __shared__ float sm[4];
  float acc = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    float pv[CM], y[CM];
    SG_CLASS_FOR(c) {
      pv[c] = p[i * C + c];
      y[c] = yt[i * y_cols + c];
    }
    const int t = row_first_max<CM, EX>(y, C);
    const int64_t g = i / n, r = i - g * n;
    SG_CLASS_FOR(c) {
      const uint32_t q = clamp_bits(pv[c]);
      const bool f = c == t;
      const uint32_t mb = f ? __float_as_uint(1.0f - __uint_as_float(q)) : q;   // in [0, 1]: at most ONE_BITS
      const int64_t o = (g * C + c) * n + r;
      keys[o] = ONE_BITS - mb;
      vals[o] = (uint32_t)i | (f ? FG_BIT : 0u);
    }
    if (kind >= 0) {
      float s = 0.f;
      SG_CLASS_FOR(c) {
        const float w = kind == SG_LOSS_EDGE_FOCAL ? yt[i * y_cols + C + c] : 1.f;
        s += loss_row_term(kind, loss_coeff(kind, al.v[c], y[c], w), pv[c]);
      }
      acc += s;
    }
  }
  const float tot = block_sum_256(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// grid = segments * ntiles
__global__ __launch_bounds__(256) void lv_count_kernel(int64_t n, int64_t ntiles, const uint32_t* __restrict__ vals,
                                                       uint32_t* __restrict__ tilecnt) {
  __shared__ uint32_t wc[SORT_WAVES];
  const int64_t seg = blockIdx.x / ntiles, tile = blockIdx.x - seg * ntiles;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t* __restrict__ src = vals + seg * n;
  uint32_t cnt = 0u;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t e = sort_elem(tile, wave, r, lane);
    cnt += (uint32_t)__popcll(__ballot(e < n && (src[e] & FG_BIT)));
  }
  if (lane == 0) wc[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tilecnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// grid = segments; the row of ntiles counts -> its exclusive scan, the total to G[seg] (the scheme of sort_scan_kernel)
__global__ __launch_bounds__(256) void lv_scan_kernel(int64_t ntiles, uint32_t* __restrict__ tilecnt, uint32_t* __restrict__ G) {
  __shared__ uint32_t ws[SORT_WAVES];
  uint32_t* __restrict__ row = tilecnt + (int64_t)blockIdx.x * ntiles;
  const int64_t per = (ntiles + 255) / 256;
  const int64_t t0 = (int64_t)threadIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  uint32_t s = 0u;
  for (int64_t t = t0; t < t1; ++t) s += row[t];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t inc = s;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = __shfl_up(inc, off, 64);
    if (lane >= off) inc += v;
  }
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  uint32_t base = 0u;
  for (int w = 0; w < wave; ++w) base += ws[w];
  uint32_t run = base + inc - s;
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t v = row[t];
    row[t] = run;
    run += v;
  }
  if (threadIdx.x == 255) G[blockIdx.x] = base + inc;
}

// classes of group g that take part: all of them, or those with G > 0
__device__ __forceinline__ int group_classes(const uint32_t* __restrict__ G, int64_t g, int C, int classes_all) {
  if (classes_all) return C;
  int nc = 0;
  for (int c = 0; c < C; ++c) nc += G[g * C + c] > 0u ? 1 : 0;
  return nc;
}

// grid = segments * ntiles
__global__ __launch_bounds__(256) void lv_grad_kernel(int64_t n, int64_t ntiles, int C, int images, int classes_all, int64_t total,
                                                      const float* __restrict__ p, const uint32_t* __restrict__ vals,
                                                      const uint32_t* __restrict__ tilecnt, const uint32_t* __restrict__ G,
                                                      float* __restrict__ g_out, uint32_t* __restrict__ part) {
  __shared__ uint32_t wc[SORT_WAVES];
  __shared__ double sm[SORT_WAVES];
  const int64_t seg = blockIdx.x / ntiles, tile = blockIdx.x - seg * ntiles;
  const int64_t grp = seg / C;
  const int c = (int)(seg - grp * C);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t Gs = G[seg];
  const int nc = group_classes(G, grp, C, classes_all);
  const bool skipped = !classes_all && Gs == 0u;
  const float inv = (float)(1.0 / ((double)images * (double)nc));
  const uint32_t* __restrict__ src = vals + seg * n;
  uint32_t v[SORT_ROUNDS];
  uint64_t fb[SORT_ROUNDS];
  uint32_t cnt = 0u;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t e = sort_elem(tile, wave, r, lane);
    v[r] = e < n ? src[e] : 0u;
    fb[r] = __ballot((v[r] & FG_BIT) != 0u);
    cnt += (uint32_t)__popcll(fb[r]);
  }
  if (lane == 0) wc[wave] = cnt;
  __syncthreads();
  uint32_t F = tilecnt[blockIdx.x];   // foreground pixels in front of this wave's share
  for (int w = 0; w < wave; ++w) F += wc[w];
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t e = sort_elem(tile, wave, r, lane);
    const uint32_t Fk = F + (uint32_t)__popcll(fb[r] & ((2ull << lane) - 1ull));   // inclusive
    F += (uint32_t)__popcll(fb[r]);
    if (e >= n) continue;
    const bool f = (v[r] & FG_BIT) != 0u;
    const int64_t o = (int64_t)(v[r] & ~FG_BIT) * C + c;
    if (o >= total) continue;   // cannot be: the payload is a row of p.  Never a store outside the tensor
    if (skipped) {
      g_out[o] = 0.f;
      continue;
    }
    const double k = (double)(e + 1), I = (double)(Gs - Fk), U = (double)Gs + k - (double)Fk;
    double gk;
    if (Gs == 0u) gk = e == 0 ? 1.0 : 0.0;
    else gk = f ? 1.0 / U : I / (U * (U - 1.0));
    const float g32 = (float)gk;
    g_out[o] = g32 == 0.f ? 0.f : (f ? -(g32 * inv) : g32 * inv);
    const float pv = p[o];
    const float m = f ? 1.0f - pv : pv;
    acc += (double)m * gk;
  }
  const double t = block_sum_double(acc, sm);
  if (threadIdx.x == 0) put_double(part + 2 * (int64_t)blockIdx.x, skipped ? 0.0 : t);
}

// grid = segments
__global__ __launch_bounds__(256) void lv_seg_kernel(int64_t ntiles, const uint32_t* __restrict__ part, uint32_t* __restrict__ segsum) {
  __shared__ double sm[SORT_WAVES];
  const uint32_t* __restrict__ row = part + 2 * (int64_t)blockIdx.x * ntiles;
  double s = 0.0;
  for (int64_t t = threadIdx.x; t < ntiles; t += 256) s += get_double(row + 2 * t);
  const double tot = block_sum_double(s, sm);
  if (threadIdx.x == 0) put_double(segsum + 2 * (int64_t)blockIdx.x, tot);
}

// one workgroup: thread t adds the pointwise partials t, t + 256, ... and the groups t, t + 256, ... in double
__global__ __launch_bounds__(256) void lv_final_kernel(const float* __restrict__ ppart, int nparts, int64_t rows, int C, int images,
                                                       int classes_all, int kind, float point_weight, float lovasz_weight,
                                                       const uint32_t* __restrict__ G, const uint32_t* __restrict__ segsum,
                                                       float* __restrict__ out) {
  __shared__ double sm[SORT_WAVES];
  double sp = 0.0, sl = 0.0;
  if (kind >= 0)
    for (int i = threadIdx.x; i < nparts; i += 256) sp += (double)ppart[i];
  for (int64_t g = threadIdx.x; g < images; g += 256) {
    const int nc = group_classes(G, g, C, classes_all);
    double s = 0.0;
    for (int c = 0; c < C; ++c)
      if (classes_all || G[g * C + c] > 0u) s += get_double(segsum + 2 * (g * C + c));
    sl += s / (double)nc;
  }
  const double tp = block_sum_double(sp, sm);
  __syncthreads();
  const double tl = block_sum_double(sl, sm);
  if (threadIdx.x == 0) {
    put_loss_terms(out, kind, point_weight, kind >= 0 ? -tp / (double)rows : 0.0, lovasz_weight, tl / (double)images);
  }
}

// The pointwise part is lossn_bwd_kernel's k * a * g with k = -(scale * point_weight) / rows: with point_weight = 1 and
// lovasz_weight = 0 the bits of sg_lossn_bwd (the Lovasz term is then not added at all, so a -0 stays a -0).
template <int CM, bool EX>
__global__ __launch_bounds__(256) void lv_bwd_kernel(int kind, int64_t rows, int C, int y_cols, const ClassVec al,
                                                     const float* __restrict__ p, const float* __restrict__ yt,
                                                     const float* __restrict__ gl, float* __restrict__ dp, float scale,
                                                     float point_weight, float lovasz_weight) {
  if (EX) C = CM;
  const float k = -(scale * point_weight) / (float)rows;
  const float sl = scale * lovasz_weight;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    if (kind < 0) {
      SG_CLASS_FOR(c) dp[i * C + c] = sl * gl[i * C + c];
      continue;
    }
    float pv[CM], y[CM], w[CM];
    SG_CLASS_FOR(c) {
      pv[c] = p[i * C + c];
      y[c] = yt[i * y_cols + c];
      w[c] = kind == SG_LOSS_EDGE_FOCAL ? yt[i * y_cols + C + c] : 1.f;
    }
    SG_CLASS_FOR(c) {
      const float a = loss_coeff(kind, al.v[c], y[c], w[c]);
      const float g = loss_row_grad(kind, pv[c]);
      const float pg = k * a * g;
      dp[i * C + c] = lovasz_weight == 0.f ? pg : pg + sl * gl[i * C + c];
    }
  }
}

// 0, or SG_EINVAL with the error text set
inline int desc_ok(const char* who, const sg_lovasz_desc* d) {
  SG_CHECK_ARG(d, "%s: no descriptor", who);
  if (const int rc = loss_head_ok(who, d->C, d->y_cols, d->point_kind, true, "pointwise loss", d->point_alpha, "point_alpha")) return rc;
  SG_CHECK_ARG(d->images >= 1 && d->images <= MAX_IMAGES, "%s: %d images outside [1, %d]", who, d->images, MAX_IMAGES);
  SG_CHECK_ARG(d->classes_all == 0 || d->classes_all == 1, "%s: classes_all = %d is not 0 or 1", who, d->classes_all);
  SG_CHECK_ARG(d->reserved == 0, "%s: reserved = %d", who, d->reserved);
  SG_CHECK_ARG(d->rows_per_image >= 1 && d->rows_per_image <= INT32_MAX / ((int64_t)d->images * d->C),
               "%s: rows_per_image = %lld: images * rows_per_image * C must lie in [1, 2^31 - 1]", who, (long long)d->rows_per_image);
  if (const int rc = loss_weights_ok(who, d->point_kind, d->point_weight, d->lovasz_weight, "lovasz_weight")) return rc;
  return sort_pairs_shape_ok(who, (int64_t)d->images * d->C, d->rows_per_image, 30);
}

// the workspace in words, in this order
struct Layout {
  size_t N, S, tiles, parts;
  size_t keys_a() const { return 0; }
  size_t vals_a() const { return N; }
  size_t keys_b() const { return 2 * N; }
  size_t vals_b() const { return 3 * N; }
  size_t table() const { return 4 * N; }
  size_t tilecnt() const { return table() + S * SORT_RADIX * (tiles + 1); }
  size_t part() const { return tilecnt() + S * tiles; }
  size_t G() const { return part() + 2 * S * tiles; }
  size_t segsum() const { return G() + S; }
  size_t ppart() const { return segsum() + 2 * S; }
  size_t words() const { return ppart() + parts; }
};

inline Layout layout(const sg_lovasz_desc* d) {
  Layout l;
  l.S = (size_t)d->images * (size_t)d->C;
  l.N = l.S * (size_t)d->rows_per_image;
  l.tiles = (size_t)sort_tiles(d->rows_per_image);
  l.parts = (size_t)sg_loss_parts(d->rows_per_image * d->images);
  return l;
}

}  // namespace

extern "C" {

size_t sg_loss_lovasz_ws_bytes(const sg_ctx*, const sg_lovasz_desc* desc) {
  if (desc_ok("sg_loss_lovasz_ws_bytes", desc)) return 0;
  return layout(desc).words() * sizeof(uint32_t);
}

int sg_loss_lovasz_fwd(sg_ctx* ctx, void* stream, const sg_lovasz_desc* desc, const void* p, const void* y_true, void* loss_out,
                       void* g_out, void* ws, size_t ws_bytes) {
  SG_CHECK_ARG(ctx && p && y_true && loss_out && g_out, "sg_loss_lovasz_fwd: bad argument");
  if (const int rc = desc_ok("sg_loss_lovasz_fwd", desc)) return rc;
  const Layout l = layout(desc);
  const size_t need = l.words() * sizeof(uint32_t);
  if (!ws || ws_bytes < need) {
    sg_set_error("sg_loss_lovasz_fwd: workspace %zu < %zu", ws_bytes, need);
    return SG_EWORKSPACE;
  }
  const int C = desc->C, kind = desc->point_kind, images = desc->images, y_cols = desc->y_cols, all = desc->classes_all;
  const int64_t n = desc->rows_per_image, rows = n * images, ntiles = (int64_t)l.tiles, S = (int64_t)l.S;
  const int parts = (int)l.parts;
  const ClassVec al = class_vec(desc->point_kind, desc->C, desc->point_alpha);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* w = (uint32_t*)ws;
  uint32_t *ka = w + l.keys_a(), *va = w + l.vals_a(), *kb = w + l.keys_b(), *vb = w + l.vals_b();
  uint32_t *table = w + l.table(), *tilecnt = w + l.tilecnt(), *part = w + l.part(), *G = w + l.G(), *segsum = w + l.segsum();
  float* ppart = (float*)(w + l.ppart());
#define L(CM, EX)                                                                                                           \
  hipLaunchKernelGGL((lv_key_kernel<CM, EX>), dim3(parts), dim3(256), 0, st, kind, rows, n, C, y_cols, al, (const float*)p, \
                     (const float*)y_true, ka, va, ppart)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("lv_key_kernel");
  // pass 0 reads pair a and writes pair b, pass 1 writes pair a, ...
  if (const int rc = sort_pairs_run(st, S, n, 30, ka, va, kb, vb, ka, va, table)) return rc;
  const uint32_t* vs = sort_final_buffer(sort_passes(30)) == 0 ? vb : va;
  const unsigned blocks = (unsigned)(S * ntiles);
  hipLaunchKernelGGL(lv_count_kernel, dim3(blocks), dim3(256), 0, st, n, ntiles, vs, tilecnt);
  SG_LAUNCH_CHECK("lv_count_kernel");
  hipLaunchKernelGGL(lv_scan_kernel, dim3((unsigned)S), dim3(256), 0, st, ntiles, tilecnt, G);
  SG_LAUNCH_CHECK("lv_scan_kernel");
  hipLaunchKernelGGL(lv_grad_kernel, dim3(blocks), dim3(256), 0, st, n, ntiles, C, images, all, rows * C, (const float*)p, vs,
                     (const uint32_t*)tilecnt, (const uint32_t*)G, (float*)g_out, part);
  SG_LAUNCH_CHECK("lv_grad_kernel");
  hipLaunchKernelGGL(lv_seg_kernel, dim3((unsigned)S), dim3(256), 0, st, ntiles, (const uint32_t*)part, segsum);
  SG_LAUNCH_CHECK("lv_seg_kernel");
  hipLaunchKernelGGL(lv_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ppart, parts, rows, C, images, all, kind,
                     desc->point_weight, desc->lovasz_weight, (const uint32_t*)G, (const uint32_t*)segsum, (float*)loss_out);
  SG_LAUNCH_CHECK("lv_final_kernel");
  return 0;
}

int sg_loss_lovasz_bwd(sg_ctx* ctx, void* stream, const sg_lovasz_desc* desc, const void* p, const void* y_true, const void* g,
                       void* dp, float grad_scale) {
  SG_CHECK_ARG(ctx && p && y_true && g && dp, "sg_loss_lovasz_bwd: bad argument");
  if (const int rc = desc_ok("sg_loss_lovasz_bwd", desc)) return rc;
  const int64_t rows = desc->rows_per_image * desc->images;
  const ClassVec al = class_vec(desc->point_kind, desc->C, desc->point_alpha);
#define L(CM, EX)                                                                                                             \
  hipLaunchKernelGGL((lv_bwd_kernel<CM, EX>), dim3(loss_bwd_blocks(rows)), dim3(256), 0, (hipStream_t)stream, desc->point_kind, rows, \
                     desc->C, desc->y_cols, al, (const float*)p, (const float*)y_true, (const float*)g, (float*)dp, grad_scale,  \
                     desc->point_weight, desc->lovasz_weight)
  SG_CLASS_DISPATCH(desc->C, L);
#undef L
  SG_LAUNCH_CHECK("lv_bwd_kernel");
  return 0;
}

}  // extern "C"
