// The C-class (2 <= C <= SG_MAX_CLASSES) softmax head: last-axis softmax, the three losses with per-class weights, the
// C x C confusion matrix and the class-map canvas of the inference tail.  fp32, rows x C, row-major, dense; a row is C
// floats and C is usually no multiple of 4, so every access is a dword access and no operand needs more than 4-byte
// alignment.  One thread owns one row and keeps it in registers: the row kernels are instantiated for C = 2 ... 8 and as
// two bounded forms (C <= 16, C <= 32) whose unrolled loops are predicated on the runtime C.
//
// At C = 2 every kernel here evaluates the expressions of the 2-class kernels (softmax2_*_kernel, loss_*_kernel,
// confusion_kernel, argmax_acc_kernel) in the same order; only the loss scalar's per-row sum is shaped differently.
#include "sg_reduce.h"
#include "loss_head.h"

namespace {

constexpr int64_t EW_CAP = 8192;   // ew_blocks: workgroups of this file's element-wise launches

template <int CM, bool EX>
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* z, float* p, int64_t rows, int C) {
  if (EX) C = CM;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    float v[CM];
    SG_CLASS_FOR(c) v[c] = z[i * C + c];
    float m = v[0];
    SG_CLASS_FOR(c) if (c > 0) m = fmaxf(m, v[c]);
    float s = 0.f;
    SG_CLASS_FOR(c) {
      v[c] = expf(v[c] - m);
      s = c == 0 ? v[c] : s + v[c];
    }
    const float inv = 1.0f / s;
    SG_CLASS_FOR(c) p[i * C + c] = v[c] * inv;
  }
}

template <int CM, bool EX>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* __restrict__ p, const float* __restrict__ dp,
                                                          float* __restrict__ dz, int64_t rows, int C) {
  if (EX) C = CM;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    float pv[CM], g[CM];
    SG_CLASS_FOR(c) {
      pv[c] = p[i * C + c];
      g[c] = dp[i * C + c];
    }
    float dot;
    if constexpr (EX && CM == 2) {
      dot = g[0] * pv[0] + g[1] * pv[1];  // softmax2_bwd_kernel's expression, so that it contracts alike
    } else {
      dot = 0.f;
      SG_CLASS_FOR(c) dot += g[c] * pv[c];
    }
    SG_CLASS_FOR(c) dz[i * C + c] = pv[c] * (g[c] - dot);
  }
}

template <int CM, bool EX>
__global__ __launch_bounds__(256) void lossn_fwd_kernel(int kind, int64_t rows, int C, int y_cols, const ClassVec al,
                                                        const float* __restrict__ p, const float* __restrict__ yt,
                                                        float* __restrict__ part) {
  if (EX) C = CM;
  __shared__ float sm[4];
  float acc = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    float pv[CM], y[CM], w[CM];
    SG_CLASS_FOR(c) {
      pv[c] = p[i * C + c];
      y[c] = yt[i * y_cols + c];
      w[c] = kind == SG_LOSS_EDGE_FOCAL ? yt[i * y_cols + C + c] : 1.f;
    }
    float r = 0.f;
    SG_CLASS_FOR(c) {
      const float a = loss_coeff(kind, al.v[c], y[c], w[c]);
      r += loss_row_term(kind, a, pv[c]);
    }
    acc += r;
  }
  const float t = block_sum_256(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ void lossn_final_kernel(const float* __restrict__ part, int nparts, int64_t rows, float* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += (double)part[i];
    out[0] = (float)(-s / (double)rows);
  }
}

// dL/dp_c = -(scale/rows) * a_c * d/dp [ f(p) log(p+eps) ];  f = (1-p)^2 -> -2(1-p) log(p+eps) + (1-p)^2/(p+eps)
template <int CM, bool EX>
__global__ __launch_bounds__(256) void lossn_bwd_kernel(int kind, int64_t rows, int C, int y_cols, const ClassVec al,
                                                        const float* __restrict__ p, const float* __restrict__ yt,
                                                        float* __restrict__ dp, float scale) {
  if (EX) C = CM;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float k = -scale / (float)rows;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    float pv[CM], y[CM], w[CM];
    SG_CLASS_FOR(c) {
      pv[c] = p[i * C + c];
      y[c] = yt[i * y_cols + c];
      w[c] = kind == SG_LOSS_EDGE_FOCAL ? yt[i * y_cols + C + c] : 1.f;
    }
    SG_CLASS_FOR(c) {
      const float a = loss_coeff(kind, al.v[c], y[c], w[c]);
      const float g = loss_row_grad(kind, pv[c]);
      dp[i * C + c] = k * a * g;
    }
  }
}

template <int CM, bool EX>
__device__ __forceinline__ int row_argmax(const float* __restrict__ r, int C) {
  float v[CM];
  SG_CLASS_FOR(c) v[c] = r[c];
  return row_first_max<CM, EX>(v, C);
}

// out[t * C + q] += #rows with argmax(y_true[:, :C]) == t and argmax(p) == q.  A workgroup counts into an LDS table of
// C * C uint32.  Real masks put most of a wave on one or two cells, so a wave does not send 64 atomics to one LDS address:
// it walks the distinct cells it holds (the first pending lane's cell, a ballot of the lanes that share it, one add of
// the popcount by that lane).  One 64-bit global integer atomic per non-zero cell and workgroup ends it: exact, whatever
// the order.  The LDS counters are 32 bits wide: one workgroup may count up to 2^32 rows (rows / 2048 of a launch), the limit
// confusion_kernel's per-thread counters have.
template <int CM, bool EX>
__global__ __launch_bounds__(256) void confusion_matrix_kernel(int64_t rows, int C, int y_cols, const float* __restrict__ p,
                                                               const float* __restrict__ yt,
                                                               unsigned long long* __restrict__ out) {
  if (EX) C = CM;
  __shared__ unsigned int tab[SG_MAX_CLASSES * SG_MAX_CLASSES];
  const int cells = C * C;
  for (int i = threadIdx.x; i < cells; i += 256) tab[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < rows; base += stride) {  // uniform in the workgroup
    const int64_t i = base + threadIdx.x;
    int cell = -1;
    if (i < rows) cell = row_argmax<CM, EX>(yt + i * y_cols, C) * C + row_argmax<CM, EX>(p + i * C, C);
    bool pending = cell >= 0;
    for (;;) {
      const unsigned long long todo = __ballot(pending);
      if (todo == 0ull) break;
      const int leader = __ffsll((long long)todo) - 1;
      const int lead_cell = __shfl(cell, leader, 64);
      const unsigned long long same = __ballot(pending && cell == lead_cell);
      if (lane == leader) atomicAdd(&tab[lead_cell], (unsigned int)__popcll(same));
      if (cell == lead_cell) pending = false;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += 256) {
    const unsigned int t = tab[i];
    if (t) atomicAdd(out + i, (unsigned long long)t);
  }
}

template <int CM, bool EX>
__global__ __launch_bounds__(256) void argmax_max_kernel(const float* __restrict__ p, int C, int TH, int TW,
                                                         unsigned char* __restrict__ canvas, int CH, int CW, int y0, int x0) {
  if (EX) C = CM;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)TH * TW) return;
  const int r = (int)(i / TW), c = (int)(i - (int64_t)r * TW);
  const int64_t yy = (int64_t)y0 + r, xx = (int64_t)x0 + c;
  if (yy < 0 || yy >= CH || xx < 0 || xx >= CW) return;
  const int q = row_argmax<CM, EX>(p + i * C, C);
  unsigned char* d = canvas + yy * CW + xx;
  const unsigned char old = *d;
  if ((unsigned char)q > old) *d = (unsigned char)q;
}

inline bool classes_ok(int C) { return C >= 2 && C <= SG_MAX_CLASSES; }

// kind, C, y_cols and alpha of the two loss calls (the weights' values are taken as they come); fills `al`
inline int lossn_args(const char* who, int kind, int C, int y_cols, const float* alpha, ClassVec& al) {
  if (const int rc = loss_head_ok(who, C, y_cols, kind, false, "loss", nullptr, "alpha")) return rc;
  SG_CHECK_ARG(kind == SG_LOSS_CE2 || alpha, "%s: focal losses need the C class weights", who);
  al = class_vec(kind, C, alpha);
  return 0;
}

}  // namespace

extern "C" {

int sg_softmax_fwd(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* z, void* p) {
  SG_CHECK_ARG(ctx && dtype == SG_F32 && z && p && rows >= 0, "sg_softmax_fwd: bad argument");
  SG_CHECK_ARG(classes_ok(C), "sg_softmax_fwd: C = %d outside [2, %d]", C, SG_MAX_CLASSES);
  if (rows == 0) return 0;
#define L(CM, EX)                                                                                                     \
  hipLaunchKernelGGL((softmax_fwd_kernel<CM, EX>), dim3(ew_blocks(rows, EW_CAP)), dim3(256), 0, (hipStream_t)stream, (const float*)z, \
                     (float*)p, rows, C)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("softmax_fwd_kernel");
  return 0;
}

int sg_softmax_bwd(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* p, const void* dp, void* dz) {
  SG_CHECK_ARG(ctx && dtype == SG_F32 && p && dp && dz && rows >= 0, "sg_softmax_bwd: bad argument");
  SG_CHECK_ARG(classes_ok(C), "sg_softmax_bwd: C = %d outside [2, %d]", C, SG_MAX_CLASSES);
  if (rows == 0) return 0;
#define L(CM, EX)                                                                                                     \
  hipLaunchKernelGGL((softmax_bwd_kernel<CM, EX>), dim3(ew_blocks(rows, EW_CAP)), dim3(256), 0, (hipStream_t)stream, (const float*)p, \
                     (const float*)dp, (float*)dz, rows, C)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("softmax_bwd_kernel");
  return 0;
}

size_t sg_lossn_ws_bytes(const sg_ctx*, int64_t rows) { return (size_t)sg_loss_parts(rows) * sizeof(float) + 256; }

int sg_lossn_fwd(sg_ctx* ctx, void* stream, int kind, int64_t rows, int C, int y_cols, const float* alpha, const void* p,
                 const void* y_true, void* loss_out, void* ws, size_t ws_bytes) {
  SG_CHECK_ARG(ctx && p && y_true && loss_out && rows > 0, "sg_lossn_fwd: bad argument");
  ClassVec al;
  if (const int rc = lossn_args("sg_lossn_fwd", kind, C, y_cols, alpha, al)) return rc;
  const int parts = sg_loss_parts(rows);
  if (!ws || ws_bytes < (size_t)parts * sizeof(float)) {
    sg_set_error("sg_lossn_fwd: workspace %zu < %zu", ws_bytes, (size_t)parts * sizeof(float));
    return SG_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
#define L(CM, EX)                                                                                                  \
  hipLaunchKernelGGL((lossn_fwd_kernel<CM, EX>), dim3(parts), dim3(256), 0, st, kind, rows, C, y_cols, al, (const float*)p, \
                     (const float*)y_true, (float*)ws)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("lossn_fwd_kernel");
  hipLaunchKernelGGL(lossn_final_kernel, dim3(1), dim3(64), 0, st, (const float*)ws, parts, rows, (float*)loss_out);
  SG_LAUNCH_CHECK("lossn_final_kernel");
  return 0;
}

int sg_lossn_bwd(sg_ctx* ctx, void* stream, int kind, int64_t rows, int C, int y_cols, const float* alpha, const void* p,
                 const void* y_true, void* dp, float grad_scale) {
  SG_CHECK_ARG(ctx && p && y_true && dp && rows > 0, "sg_lossn_bwd: bad argument");
  ClassVec al;
  if (const int rc = lossn_args("sg_lossn_bwd", kind, C, y_cols, alpha, al)) return rc;
#define L(CM, EX)                                                                                                      \
  hipLaunchKernelGGL((lossn_bwd_kernel<CM, EX>), dim3(loss_bwd_blocks(rows)), dim3(256), 0, (hipStream_t)stream, kind, rows, C, \
                     y_cols, al, (const float*)p, (const float*)y_true, (float*)dp, grad_scale)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("lossn_bwd_kernel");
  return 0;
}

int sg_confusion_matrix(sg_ctx* ctx, void* stream, int64_t rows, int C, int y_cols, const void* p, const void* y_true,
                        void* out_i64) {
  SG_CHECK_ARG(ctx && p && y_true && out_i64 && rows > 0, "sg_confusion_matrix: bad argument");
  SG_CHECK_ARG(classes_ok(C), "sg_confusion_matrix: C = %d outside [2, %d]", C, SG_MAX_CLASSES);
  SG_CHECK_ARG(y_cols == C || y_cols == 2 * C, "sg_confusion_matrix: y_true has %d columns, not C = %d or 2C", y_cols, C);
  int64_t blocks = sg_cdiv(rows, 256 * 4);
  if (blocks > 2048) blocks = 2048;
#define L(CM, EX)                                                                                                        \
  hipLaunchKernelGGL((confusion_matrix_kernel<CM, EX>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, C, \
                     y_cols, (const float*)p, (const float*)y_true, (unsigned long long*)out_i64)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("confusion_matrix_kernel");
  return 0;
}

int sg_argmax_max_u8(sg_ctx* ctx, void* stream, const void* p, int C, int TH, int TW, void* canvas_u8, int CH, int CW,
                     int y0, int x0) {
  SG_CHECK_ARG(ctx && p && canvas_u8 && TH > 0 && TW > 0 && CH > 0 && CW > 0, "sg_argmax_max_u8: bad argument");
  SG_CHECK_ARG(classes_ok(C), "sg_argmax_max_u8: C = %d outside [2, %d]", C, SG_MAX_CLASSES);
  const int64_t blocks = sg_cdiv((int64_t)TH * TW, 256);
  SG_CHECK_ARG(blocks < (1ll << 31), "sg_argmax_max_u8: a tile of %d x %d", TH, TW);
#define L(CM, EX)                                                                                                      \
  hipLaunchKernelGGL((argmax_max_kernel<CM, EX>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)p, \
                     C, TH, TW, (unsigned char*)canvas_u8, CH, CW, y0, x0)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("argmax_max_kernel");
  return 0;
}

}  // extern "C"
