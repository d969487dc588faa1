// Region-overlap losses (Dice / Jaccard / Tversky, focal-Tversky with gamma > 1) on the C-class head, alone or added to one of
// the three pointwise losses of multiclass.hip.  Per group g (the batch, or one image) and class c
//   I = sum p y, P = sum p, Y = sum y,  D = I + a (P - I) + b (Y - I) + s,  T = (I + s) / D,  l = (1 - T)^gamma,
// and dL_region/dp[r,c] = A_gc y[r,c] + B_gc.  So the loss costs two passes over p and y_true, as the pointwise pair does:
//   region_fwd_kernel    one grid-stride pass per image; a thread keeps the pointwise partial and the 3C region partials, a
//                        workgroup writes 1 + 3C floats {point, I[C], P[C], Y[C]} to ws[image][part][1 + 3C]
//   region_final_kernel  one workgroup per image sums the parts column by column in double in a fixed order (thread t owns
//                        column t mod (1 + 3C) of every (256 / (1 + 3C))-th part: consecutive threads read consecutive floats),
//                        then writes that image's {A, B} and, with one image, the three loss scalars
//   region_total_kernel  more than one image: the per-image sums in image order -> the three loss scalars
//   region_bwd_kernel    dp = grad_scale * (lambda_p * pointwise gradient + A y + B), {A, B} read from device memory
// No float atomics anywhere: the same bits from run to run.  fp32, dense rows, dword accesses (4-byte alignment is enough).
#include "loss_head.h"

namespace {

constexpr int MAX_COLS = 1 + 3 * SG_MAX_CLASSES;
constexpr int MAX_IMAGES = 65535;  // gridDim.y

// what the final kernel needs of the descriptor
struct RegionTerm {
  float a, b, smooth, gamma;
  float point_weight, region_weight;
  double inv_gw;  // 1 / (G * sum_c w_c)
  ClassVec w;
};

__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// grid (parts, images); kind < 0: no pointwise term (column 0 of every part is 0)
template <int CM, bool EX>
__global__ __launch_bounds__(256) void region_fwd_kernel(int kind, int64_t rows_per_image, int C, int y_cols, const ClassVec al,
                                                         const float* __restrict__ p, const float* __restrict__ yt,
                                                         float* __restrict__ part) {
  if (EX) C = CM;
  __shared__ float sm[4][MAX_COLS];
  float acc = 0.f, si[CM], sp[CM], sy[CM];
  SG_CLASS_FOR(c) si[c] = sp[c] = sy[c] = 0.f;
  const int64_t row0 = (int64_t)blockIdx.y * rows_per_image;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows_per_image; r += stride) {
    const int64_t i = row0 + r;
    float pv[CM], y[CM];
    SG_CLASS_FOR(c) {
      pv[c] = p[i * C + c];
      y[c] = yt[i * y_cols + c];
    }
    if (kind >= 0) {
      float t = 0.f;
      SG_CLASS_FOR(c) {
        const float w = kind == SG_LOSS_EDGE_FOCAL ? yt[i * y_cols + C + c] : 1.f;
        t += loss_row_term(kind, loss_coeff(kind, al.v[c], y[c], w), pv[c]);
      }
      acc += t;
    }
    SG_CLASS_FOR(c) {
      si[c] += pv[c] * y[c];
      sp[c] += pv[c];
      sy[c] += y[c];
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  acc = wave_sum(acc);
  if (lane == 0) sm[wave][0] = acc;
  SG_CLASS_FOR(c) {
    const float ti = wave_sum(si[c]), tp = wave_sum(sp[c]), ty = wave_sum(sy[c]);
    if (lane == 0) {
      sm[wave][1 + c] = ti;
      sm[wave][1 + C + c] = tp;
      sm[wave][1 + 2 * C + c] = ty;
    }
  }
  __syncthreads();
  const int ncols = 1 + 3 * C;
  if ((int)threadIdx.x < ncols) {
    const int t = threadIdx.x;
    part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ncols + t] = sm[0][t] + sm[1][t] + sm[2][t] + sm[3][t];
  }
}

// grid (images); 256 threads
__global__ __launch_bounds__(256) void region_final_kernel(const float* __restrict__ part, int parts, int C, int kind, int images,
                                                           int64_t rows, const RegionTerm rt, float* __restrict__ loss_out,
                                                           float* __restrict__ coef, float* __restrict__ img_sums) {
  __shared__ double slab[256];
  __shared__ double tot[MAX_COLS];
  __shared__ double term[SG_MAX_CLASSES];
  const int ncols = 1 + 3 * C;
  const int nsl = 256 / ncols;  // >= 2: parts q = sl, sl + nsl, ... go to slab sl
  const int t = threadIdx.x, col = t % ncols, sl = t / ncols;
  const int img = blockIdx.x;
  if (sl < nsl) {
    const float* __restrict__ src = part + (int64_t)img * parts * ncols + col;
    double s = 0.0;
#pragma unroll 4
    for (int q = sl; q < parts; q += nsl) s += (double)src[(int64_t)q * ncols];
    slab[t] = s;
  }
  __syncthreads();
  if (t < ncols) {
    double s = 0.0;
    for (int k = 0; k < nsl; ++k) s += slab[k * ncols + t];
    tot[t] = s;
  }
  __syncthreads();
  if (t < C) {
    const double a = rt.a, b = rt.b, gamma = rt.gamma, w = rt.w.v[t];
    const double I = tot[1 + t], P = tot[1 + C + t], Y = tot[1 + 2 * C + t];
    const double Is = I + (double)rt.smooth;
    const double D = Is + a * (P - I) + b * (Y - I);
    const double u = fmax(1.0 - Is / D, 0.0);  // 1 - T; rounding of the fp32 parts may leave P - I a hair below 0
    const double l = rt.gamma == 1.f ? u : pow(u, gamma);
    const double du = rt.gamma == 1.f ? 1.0 : gamma * pow(u, gamma - 1.0);
    const double k = -(double)rt.region_weight * w * du * rt.inv_gw / (D * D);
    coef[(int64_t)img * 2 * C + t] = (float)(k * (D - Is * (1.0 - a - b)));
    coef[(int64_t)img * 2 * C + C + t] = (float)(-k * Is * a);
    term[t] = w * l;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += term[c];
    if (images == 1) {
      put_loss_terms(loss_out, kind, rt.point_weight, kind >= 0 ? -tot[0] / (double)rows : 0.0, rt.region_weight, s * rt.inv_gw);
    } else {
      img_sums[2 * img] = (float)tot[0];
      img_sums[2 * img + 1] = (float)s;
    }
  }
}

__global__ void region_total_kernel(const float* __restrict__ img_sums, int images, int kind, int64_t rows, const RegionTerm rt,
                                    float* __restrict__ loss_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double sp = 0.0, sr = 0.0;
    for (int g = 0; g < images; ++g) {
      sp += (double)img_sums[2 * g];
      sr += (double)img_sums[2 * g + 1];
    }
    put_loss_terms(loss_out, kind, rt.point_weight, kind >= 0 ? -sp / (double)rows : 0.0, rt.region_weight, sr * rt.inv_gw);
  }
}

// grid (blocks, images).  The pointwise part is lossn_bwd_kernel's k * a * g with k = -(scale * lambda_p) / rows: with
// lambda_p = 1 and {A, B} = 0 the bits of sg_lossn_bwd.
template <int CM, bool EX>
__global__ __launch_bounds__(256) void region_bwd_kernel(int kind, int64_t rows_per_image, int64_t rows, int C, int y_cols,
                                                         const ClassVec al, const float* __restrict__ p,
                                                         const float* __restrict__ yt, const float* __restrict__ coef,
                                                         float* __restrict__ dp, float scale, float point_weight) {
  if (EX) C = CM;
  float A[CM], B[CM];
  SG_CLASS_FOR(c) {
    A[c] = scale * coef[(int64_t)blockIdx.y * 2 * C + c];
    B[c] = scale * coef[(int64_t)blockIdx.y * 2 * C + C + c];
  }
  const float k = -(scale * point_weight) / (float)rows;
  const int64_t row0 = (int64_t)blockIdx.y * rows_per_image;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows_per_image; r += stride) {
    const int64_t i = row0 + r;
    float pv[CM], y[CM];
    SG_CLASS_FOR(c) {
      pv[c] = p[i * C + c];
      y[c] = yt[i * y_cols + c];
    }
    if (kind >= 0) {
      SG_CLASS_FOR(c) {
        const float w = kind == SG_LOSS_EDGE_FOCAL ? yt[i * y_cols + C + c] : 1.f;
        const float a = loss_coeff(kind, al.v[c], y[c], w);
        const float g = loss_row_grad(kind, pv[c]);
        const float pg = k * a * g;
        dp[i * C + c] = pg + (A[c] * y[c] + B[c]);
      }
    } else {
      SG_CLASS_FOR(c) dp[i * C + c] = A[c] * y[c] + B[c];
    }
  }
}

// 0, or SG_EINVAL with the error text set
inline int desc_ok(const char* who, const sg_region_desc* d) {
  SG_CHECK_ARG(d, "%s: no descriptor", who);
  if (const int rc = loss_head_ok(who, d->C, d->y_cols, d->point_kind, true, "pointwise loss", d->point_alpha, "point_alpha")) return rc;
  SG_CHECK_ARG(d->images >= 1 && d->images <= MAX_IMAGES, "%s: %d images outside [1, %d]", who, d->images, MAX_IMAGES);
  SG_CHECK_ARG(d->rows_per_image > 0 && d->rows_per_image <= INT64_MAX / ((int64_t)d->images * 4 * SG_MAX_CLASSES),
               "%s: rows_per_image = %lld", who, (long long)d->rows_per_image);
  SG_CHECK_ARG(nonneg(d->a) && nonneg(d->b), "%s: a = %g, b = %g must be finite and >= 0", who, d->a, d->b);
  SG_CHECK_ARG(nonneg(d->smooth) && d->smooth > 0.f, "%s: smooth = %g must be finite and > 0", who, d->smooth);
  SG_CHECK_ARG(nonneg(d->gamma) && d->gamma >= 1.f, "%s: gamma = %g must be finite and >= 1", who, d->gamma);
  double sw = 0.0;
  for (int c = 0; c < d->C; ++c) {
    SG_CHECK_ARG(nonneg(d->class_w[c]), "%s: class_w[%d] = %g must be finite and >= 0", who, c, d->class_w[c]);
    sw += d->class_w[c];
  }
  SG_CHECK_ARG(sw > 0.0, "%s: the class weights sum to 0", who);
  return loss_weights_ok(who, d->point_kind, d->point_weight, d->region_weight, "region_weight");
}

inline size_t part_floats(const sg_region_desc* d) {
  return (size_t)d->images * (size_t)sg_loss_parts(d->rows_per_image) * (size_t)(1 + 3 * d->C);
}

inline size_t ws_floats(const sg_region_desc* d) { return part_floats(d) + (d->images > 1 ? 2 * (size_t)d->images : 0); }

}  // namespace

extern "C" {

size_t sg_loss_region_ws_bytes(const sg_ctx*, const sg_region_desc* desc) {
  if (desc_ok("sg_loss_region_ws_bytes", desc)) return 0;
  return ws_floats(desc) * sizeof(float);
}

int sg_loss_region_fwd(sg_ctx* ctx, void* stream, const sg_region_desc* desc, const void* p, const void* y_true, void* loss_out,
                       void* coef_out, void* ws, size_t ws_bytes) {
  SG_CHECK_ARG(ctx && p && y_true && loss_out && coef_out, "sg_loss_region_fwd: bad argument");
  if (const int rc = desc_ok("sg_loss_region_fwd", desc)) return rc;
  const size_t need = ws_floats(desc) * sizeof(float);
  if (!ws || ws_bytes < need) {
    sg_set_error("sg_loss_region_fwd: workspace %zu < %zu", ws_bytes, need);
    return SG_EWORKSPACE;
  }
  const int C = desc->C, kind = desc->point_kind, images = desc->images;
  const int parts = sg_loss_parts(desc->rows_per_image);
  const int64_t rows = desc->rows_per_image * images;
  const ClassVec al = class_vec(desc->point_kind, desc->C, desc->point_alpha);
  RegionTerm rt;
  rt.a = desc->a, rt.b = desc->b, rt.smooth = desc->smooth, rt.gamma = desc->gamma;
  rt.point_weight = desc->point_weight, rt.region_weight = desc->region_weight;
  double sw = 0.0;
  for (int c = 0; c < SG_MAX_CLASSES; ++c) {
    rt.w.v[c] = c < C ? desc->class_w[c] : 0.f;
    sw += rt.w.v[c];
  }
  rt.inv_gw = 1.0 / ((double)images * sw);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  float* img_sums = part + part_floats(desc);
#define L(CM, EX)                                                                                                        \
  hipLaunchKernelGGL((region_fwd_kernel<CM, EX>), dim3(parts, images), dim3(256), 0, st, kind, desc->rows_per_image, C, \
                     desc->y_cols, al, (const float*)p, (const float*)y_true, part)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("region_fwd_kernel");
  hipLaunchKernelGGL(region_final_kernel, dim3(images), dim3(256), 0, st, (const float*)part, parts, C, kind, images, rows, rt,
                     (float*)loss_out, (float*)coef_out, img_sums);
  SG_LAUNCH_CHECK("region_final_kernel");
  if (images > 1) {
    hipLaunchKernelGGL(region_total_kernel, dim3(1), dim3(64), 0, st, (const float*)img_sums, images, kind, rows, rt,
                       (float*)loss_out);
    SG_LAUNCH_CHECK("region_total_kernel");
  }
  return 0;
}

int sg_loss_region_bwd(sg_ctx* ctx, void* stream, const sg_region_desc* desc, const void* p, const void* y_true, const void* coef,
                       void* dp, float grad_scale) {
  SG_CHECK_ARG(ctx && p && y_true && coef && dp, "sg_loss_region_bwd: bad argument");
  if (const int rc = desc_ok("sg_loss_region_bwd", desc)) return rc;
  const int C = desc->C, images = desc->images;
  const int64_t rows = desc->rows_per_image * images;
  const ClassVec al = class_vec(desc->point_kind, desc->C, desc->point_alpha);
#define L(CM, EX)                                                                                                            \
  hipLaunchKernelGGL((region_bwd_kernel<CM, EX>), dim3(loss_bwd_blocks(desc->rows_per_image), images), dim3(256), 0, (hipStream_t)stream,         \
                     desc->point_kind, desc->rows_per_image, rows, C, desc->y_cols, al, (const float*)p, (const float*)y_true, \
                     (const float*)coef, (float*)dp, grad_scale, desc->point_weight)
  SG_CLASS_DISPATCH(C, L);
#undef L
  SG_LAUNCH_CHECK("region_bwd_kernel");
  return 0;
}

}  // extern "C"
