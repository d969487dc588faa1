// Hard-pixel mining (OHEM) for the three pointwise losses of multiclass.hip.  Row i has the truth class
// t_i = argmax y_true[i, :C] (ties to the lowest index) and the key q_i = p[i, t_i] clamped to [0, 1] (a NaN counts as 0).
// With q_(k) the k-th smallest key, T = max(thresh, q_(k)); a row is kept iff q_i <= T (every tie at T is kept), and
//   L = sum_kept l_i / n_kept,   dL/dp[i, :] = grad_scale * dl_i/dp / n_kept on kept rows, +0 on the others.
// A non-negative float orders as its bit pattern does, so q_(k) comes from an exact radix select on the 32 key bits, in three
// digits of 11, 11 and 10 bits from the top:
//   mine_zero_kernel    clears the state words and the digit tables (a kernel, not a memset node: DESIGN 4.10)
//   mine_key_kernel     one pass over p and y_true: key bits -> ws (4 B per row), histogram of the top digit, #{key <= thresh}
//                       (one count per workgroup, added up by the pick kernel)
//   mine_pick_kernel    one workgroup: the digit's bin that holds rank k, the rank left inside it, the count below it.  After
//                       the first digit, #{key <= thresh} >= k means q_(k) <= thresh: T = thresh, the record is written and
//                       the later select kernels return at once
//   mine_narrow_kernel  one pass over the stored keys: histogram of the next digit among the keys that carry the prefix
//   mine_sum_kernel     one pass over p and y_true: workgroup partials of the row sums over key <= T, summed in a fixed order
//                       in double by mine_final_kernel.  n_kept needs no pass: the count below the last bin plus its population
//   mine_bwd_kernel     reads the record {T bits, 0, n_kept} and recomputes the key (the workspace is not kept between the calls)
// Histogram counters are integers: a workgroup counts in LDS and adds each non-zero bin to the table once, exact whatever the
// order.  No float atomics, no allocation, no synchronisation: the same bits from run to run, and every call can be captured.
// fp32, dense rows, dword accesses to p and y_true (4-byte alignment is enough); the stored keys are read 16 bytes at a time
// when the workspace is 16-byte aligned.
#include <string.h>
#include "loss_head.h"

namespace {

constexpr int BINS = 2048;      // bins of a digit's table (the last digit uses 1024 of them)
constexpr int LEVELS = 3;
// the state words in front of the tables
enum { ST_PREFIX = 0, ST_RANK, ST_BELOW, ST_DONE, ST_WORDS = 8 };
constexpr int TAB_WORDS = ST_WORDS + LEVELS * BINS;

// the key bits of one row: p at the first maximum of y_true[:C], clamped to [0, 1] on the bits
template <int CM, bool EX>
__device__ __forceinline__ uint32_t row_key(const float* __restrict__ p_row, const float* __restrict__ y_row, int C) {
  float y[CM];
  SG_CLASS_FOR(c) y[c] = y_row[c];
  return clamp_bits(p_row[row_first_max<CM, EX>(y, C)]);
}

// the workgroup's LDS table -> the global one: one integer add per non-zero bin
__device__ __forceinline__ void flush_bins(const uint32_t* h, uint32_t* __restrict__ dst) {
  for (int b = threadIdx.x; b < BINS; b += 256) {
    const uint32_t v = h[b];
    if (v) atomicAdd(dst + b, v);
  }
}

// the state words and the three tables start at 0 (a kernel node like every other launch of a captured step)
__global__ __launch_bounds__(256) void mine_zero_kernel(uint32_t* __restrict__ tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < TAB_WORDS) tab[i] = 0u;
}

template <int CM, bool EX>
__global__ __launch_bounds__(256) void mine_key_kernel(int64_t rows, int C, int y_cols, uint32_t thresh_bits,
                                                       const float* __restrict__ p, const float* __restrict__ yt,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ tab,
                                                       uint32_t* __restrict__ lep) {
  if (EX) C = CM;
  __shared__ uint32_t h[BINS];
  __shared__ uint32_t wle[4];
  for (int b = threadIdx.x; b < BINS; b += 256) h[b] = 0u;
  __syncthreads();
  uint32_t le = 0u;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    const uint32_t k = row_key<CM, EX>(p + i * C, yt + i * y_cols, C);
    keys[i] = k;
    atomicAdd(&h[k >> 21], 1u);
    le += k <= thresh_bits ? 1u : 0u;
  }
  le = block_sum_256(le, wle);
  if (threadIdx.x == 0) lep[blockIdx.x] = le;  // one word per workgroup: 8192 waves adding to one address took 60 us of a
  flush_bins(h, tab + ST_WORDS);               // 107 us pass
}

// one workgroup of 256 threads, eight bins each
__global__ __launch_bounds__(256) void mine_pick_kernel(uint32_t* __restrict__ tab, int level, uint32_t k, uint32_t thresh_bits,
                                                        const uint32_t* __restrict__ lep, int parts, uint32_t* __restrict__ sel) {
  __shared__ uint32_t ls[256], ex[256], wle[4];
  const int t = threadIdx.x;
  const uint32_t done = tab[ST_DONE], prefix = level ? tab[ST_PREFIX] : 0u, below0 = level ? tab[ST_BELOW] : 0u;
  const uint32_t rank = level ? tab[ST_RANK] : k;
  if (level == 0) {  // #{key <= thresh}: the key pass left one count per workgroup
    uint32_t a = 0u;
    for (int i = t; i < parts; i += 256) a += lep[i];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if ((t & 63) == 0) wle[t >> 6] = a;
  }
  const uint32_t* h = tab + ST_WORDS + level * BINS;
  uint32_t v[8], s = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = h[8 * t + j];
    s += v[j];
  }
  ls[t] = s;
  __syncthreads();  // every thread has read the state before one of them writes it
  if (done) return;
  const uint32_t le = level == 0 ? wle[0] + wle[1] + wle[2] + wle[3] : 0u;
  if (level == 0 && le >= k) {  // q_(k) <= thresh: T = thresh and the kept rows are those counted by the key pass
    if (t == 0) {
      sel[0] = thresh_bits, sel[1] = 0u, sel[2] = le, sel[3] = 0u;
      tab[ST_DONE] = 1u;
    }
    return;
  }
  if (t == 0) {
    uint32_t run = 0u;
    for (int j = 0; j < 256; ++j) {
      ex[j] = run;
      run += ls[j];
    }
  }
  __syncthreads();
  uint32_t below = ex[t];
  if (below < rank && rank <= below + s) {  // exactly one thread: rank >= 1 and the table holds at least rank keys
    int j = 0;
    while (j < 7 && rank > below + v[j]) below += v[j++];
    const int bits = level == 2 ? 10 : 11;
    const uint32_t pre = (prefix << bits) | (uint32_t)(8 * t + j);
    tab[ST_PREFIX] = pre;
    tab[ST_RANK] = rank - below;
    tab[ST_BELOW] = below0 + below;
    if (level == 2) {  // pre = the bits of q_(k), above thresh here; kept = the keys below it and all that equal it
      const unsigned long long n = (unsigned long long)below0 + below + v[j];
      sel[0] = pre > thresh_bits ? pre : thresh_bits;
      sel[1] = 0u;
      sel[2] = (uint32_t)n;
      sel[3] = (uint32_t)(n >> 32);
    }
  }
}

// level 1: keys whose top 11 bits are the prefix, digit = bits 20..10; level 2: top 22 bits, digit = bits 9..0
template <bool VEC>
__global__ __launch_bounds__(256) void mine_narrow_kernel(int64_t rows, const uint32_t* __restrict__ keys,
                                                          uint32_t* __restrict__ tab, int level) {
  if (tab[ST_DONE]) return;  // nobody writes it in this launch
  __shared__ uint32_t h[BINS];
  for (int b = threadIdx.x; b < BINS; b += 256) h[b] = 0u;
  __syncthreads();
  const uint32_t prefix = tab[ST_PREFIX];
  const int shift = level == 1 ? 21 : 10, dshift = level == 1 ? 10 : 0;
  const uint32_t mask = level == 1 ? 0x7ffu : 0x3ffu;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    const int64_t n4 = rows >> 2;
    const u32x4_c* __restrict__ k4 = reinterpret_cast<const u32x4_c*>(keys);
    for (int64_t j = gt; j < n4; j += stride) {
      const u32x4_c q = k4[j];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((q[e] >> shift) == prefix) atomicAdd(&h[(q[e] >> dshift) & mask], 1u);
    }
    const int64_t i = (n4 << 2) + gt;  // the last rows % 4 keys
    if (i < rows && (keys[i] >> shift) == prefix) atomicAdd(&h[(keys[i] >> dshift) & mask], 1u);
  } else {
    for (int64_t i = gt; i < rows; i += stride) {
      const uint32_t q = keys[i];
      if ((q >> shift) == prefix) atomicAdd(&h[(q >> dshift) & mask], 1u);
    }
  }
  __syncthreads();
  flush_bins(h, tab + ST_WORDS + level * BINS);
}

template <int CM, bool EX>
__global__ __launch_bounds__(256) void mine_sum_kernel(int kind, int64_t rows, int C, int y_cols, const ClassVec al,
                                                       const float* __restrict__ p, const float* __restrict__ yt,
                                                       const uint32_t* __restrict__ sel, float* __restrict__ part) {
  if (EX) C = CM;
  __shared__ float sm[4];
  const uint32_t T = sel[0];
  float acc = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    if (row_key<CM, EX>(p + i * C, yt + i * y_cols, C) > T) continue;
    float r = 0.f;
    SG_CLASS_FOR(c) {
      const float pv = p[i * C + c], y = yt[i * y_cols + c];
      const float w = kind == SG_LOSS_EDGE_FOCAL ? yt[i * y_cols + C + c] : 1.f;
      r += loss_row_term(kind, loss_coeff(kind, al.v[c], y, w), pv);
    }
    acc += r;
  }
  const float t = block_sum_256(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// one workgroup of 256 threads: thread t adds parts t, t + 256, ... in double, a wave folds its 64 sums by xor-shuffles, thread 0
// adds the four wave sums in wave order.  The order is fixed by the launch shape alone.  (One thread walking 2048 parts, each
// add behind a load, took 105 us.)
__global__ __launch_bounds__(256) void mine_final_kernel(const float* __restrict__ part, int nparts,
                                                         const uint32_t* __restrict__ sel, float* __restrict__ out) {
  __shared__ double ws[4];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < nparts; i += 256) s += (double)part[i];
  const double tot = block_sum_double(s, ws);
  if (t == 0) {
    const unsigned long long n = (unsigned long long)sel[2] | ((unsigned long long)sel[3] << 32);
    out[0] = (float)(-tot / (double)n);
  }
}

template <int CM, bool EX>
__global__ __launch_bounds__(256) void mine_bwd_kernel(int kind, int64_t rows, int C, int y_cols, const ClassVec al,
                                                       const float* __restrict__ p, const float* __restrict__ yt,
                                                       const uint32_t* __restrict__ sel, float* __restrict__ dp, float scale) {
  if (EX) C = CM;
  const uint32_t T = sel[0];
  const unsigned long long n = (unsigned long long)sel[2] | ((unsigned long long)sel[3] << 32);
  const float k = -scale / (float)n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    if (row_key<CM, EX>(p + i * C, yt + i * y_cols, C) > T) {
      SG_CLASS_FOR(c) dp[i * C + c] = 0.f;
      continue;
    }
    SG_CLASS_FOR(c) {
      const float pv = p[i * C + c], y = yt[i * y_cols + c];
      const float w = kind == SG_LOSS_EDGE_FOCAL ? yt[i * y_cols + C + c] : 1.f;
      dp[i * C + c] = k * loss_coeff(kind, al.v[c], y, w) * loss_row_grad(kind, pv);
    }
  }
}

// 0, or SG_EINVAL with the error text set
inline int desc_ok(const char* who, const sg_mine_desc* d) {
  SG_CHECK_ARG(d, "%s: no descriptor", who);
  if (const int rc = loss_head_ok(who, d->C, d->y_cols, d->kind, false, "loss", d->alpha, "alpha")) return rc;
  SG_CHECK_ARG(d->reserved == 0, "%s: reserved = %d", who, d->reserved);
  SG_CHECK_ARG(d->rows >= 1 && d->rows <= 0xffffffffll, "%s: rows = %lld outside [1, 2^32 - 1]", who, (long long)d->rows);
  SG_CHECK_ARG(d->min_kept >= 1 && d->min_kept <= d->rows, "%s: min_kept = %lld outside [1, rows = %lld]", who,
               (long long)d->min_kept, (long long)d->rows);
  SG_CHECK_ARG(d->thresh >= 0.f && d->thresh <= 1.f, "%s: thresh = %g outside [0, 1]", who, d->thresh);  // a NaN fails both
  return 0;
}

// keys[rows] | state and tables | #{key <= thresh} per workgroup [parts] | loss partials [parts]
inline size_t ws_words(const sg_mine_desc* d) { return (size_t)d->rows + TAB_WORDS + 2 * (size_t)sg_loss_parts(d->rows); }

inline uint32_t float_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  return u;
}

}  // namespace

extern "C" {

size_t sg_loss_mined_ws_bytes(const sg_ctx*, const sg_mine_desc* desc) {
  if (desc_ok("sg_loss_mined_ws_bytes", desc)) return 0;
  return ws_words(desc) * sizeof(uint32_t);
}

int sg_loss_mined_fwd(sg_ctx* ctx, void* stream, const sg_mine_desc* desc, const void* p, const void* y_true, void* loss_out,
                      void* sel_out, void* ws, size_t ws_bytes) {
  SG_CHECK_ARG(ctx && p && y_true && loss_out && sel_out, "sg_loss_mined_fwd: bad argument");
  if (const int rc = desc_ok("sg_loss_mined_fwd", desc)) return rc;
  const size_t need = ws_words(desc) * sizeof(uint32_t);
  if (!ws || ws_bytes < need) {
    sg_set_error("sg_loss_mined_fwd: workspace %zu < %zu", ws_bytes, need);
    return SG_EWORKSPACE;
  }
  const int C = desc->C, kind = desc->kind, y_cols = desc->y_cols;
  const int64_t rows = desc->rows;
  const int parts = sg_loss_parts(rows);
  const uint32_t k = (uint32_t)desc->min_kept;
  const uint32_t thresh_bits = desc->thresh > 0.f ? float_bits(desc->thresh) : 0u;  // -0 is 0
  const ClassVec al = class_vec(desc->kind, desc->C, desc->alpha);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* keys = (uint32_t*)ws;
  uint32_t* tab = keys + rows;
  uint32_t* lep = tab + TAB_WORDS;
  float* part = (float*)(lep + parts);
  uint32_t* sel = (uint32_t*)sel_out;
  const bool vec = ((uintptr_t)ws & 15) == 0;
  hipLaunchKernelGGL(mine_zero_kernel, dim3((TAB_WORDS + 255) / 256), dim3(256), 0, st, tab);
  SG_LAUNCH_CHECK("mine_zero_kernel");
#define L(CM, EX)                                                                                                      \
  hipLaunchKernelGGL((mine_key_kernel<CM, EX>), dim3(parts), dim3(256), 0, st, rows, C, y_cols, thresh_bits, (const float*)p, \
                     (const float*)y_true, keys, tab, lep)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("mine_key_kernel");
  for (int level = 0; level < LEVELS; ++level) {
    if (level > 0) {
      if (vec)
        hipLaunchKernelGGL(mine_narrow_kernel<true>, dim3(parts), dim3(256), 0, st, rows, (const uint32_t*)keys, tab, level);
      else
        hipLaunchKernelGGL(mine_narrow_kernel<false>, dim3(parts), dim3(256), 0, st, rows, (const uint32_t*)keys, tab, level);
      SG_LAUNCH_CHECK("mine_narrow_kernel");
    }
    hipLaunchKernelGGL(mine_pick_kernel, dim3(1), dim3(256), 0, st, tab, level, k, thresh_bits, (const uint32_t*)lep, parts,
                       sel);
    SG_LAUNCH_CHECK("mine_pick_kernel");
  }
#define L(CM, EX)                                                                                                            \
  hipLaunchKernelGGL((mine_sum_kernel<CM, EX>), dim3(parts), dim3(256), 0, st, kind, rows, C, y_cols, al, (const float*)p, \
                     (const float*)y_true, (const uint32_t*)sel, part)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("mine_sum_kernel");
  hipLaunchKernelGGL(mine_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, parts, (const uint32_t*)sel,
                     (float*)loss_out);
  SG_LAUNCH_CHECK("mine_final_kernel");
  return 0;
}

int sg_loss_mined_bwd(sg_ctx* ctx, void* stream, const sg_mine_desc* desc, const void* p, const void* y_true, const void* sel,
                      void* dp, float grad_scale) {
  SG_CHECK_ARG(ctx && p && y_true && sel && dp, "sg_loss_mined_bwd: bad argument");
  if (const int rc = desc_ok("sg_loss_mined_bwd", desc)) return rc;
  const ClassVec al = class_vec(desc->kind, desc->C, desc->alpha);
#define L(CM, EX)                                                                                                              \
  hipLaunchKernelGGL((mine_bwd_kernel<CM, EX>), dim3(loss_bwd_blocks(desc->rows)), dim3(256), 0, (hipStream_t)stream, desc->kind, desc->rows, \
                     desc->C, desc->y_cols, al, (const float*)p, (const float*)y_true, (const uint32_t*)sel, (float*)dp, grad_scale)
  SG_CLASS_DISPATCH(desc->C, L);
#undef L
  SG_LAUNCH_CHECK("mine_bwd_kernel");
  return 0;
}

}  // extern "C"
