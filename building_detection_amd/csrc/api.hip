// libsegengine: context, error reporting and small utility entry points of the C ABI (include/segengine.h).
#include "sg_reduce.h"
#include <string.h>

static thread_local char g_err[512] = "";

void sg_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {
__global__ void fill_f32_kernel(float* __restrict__ p, int64_t n, float v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}
// Empty one-thread kernels whose NAMES bracket a group of launches in a rocprofv3 kernel trace (sg_trace_mark)
template <int TAG, int END>
__global__ void sg_trace_mark_kernel() {}

template <typename TS, typename TD>
__global__ void cast_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int64_t n) {
  const int64_t nv = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) st4<TD>(dst + 4 * i, ld4<TS>(src + 4 * i));
  const int64_t i = (nv << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && i < n) st1<TD>(dst + i, ld1<TS>(src + i));
}

// dst = (float)src / div - sub: the pixel normalisations of decode_img / decode_lbel (DeepLabv3plus.py:36-37, 48)
__global__ void u8_to_f32_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int64_t n, float div, float sub) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = (float)src[i] / div - sub;  // IEEE division, then one rounding: numpy's float32 result
}

__global__ void scale_f32_kernel(float* __restrict__ p, int64_t n, float a) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] *= a;
}
}  // namespace

extern "C" {

int sg_abi_version(void) { return SG_ABI_VERSION; }

const char* sg_last_error(void) { return g_err; }

int sg_create(int device, sg_ctx** out) {
  SG_CHECK_ARG(out != nullptr, "sg_create: null out");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    sg_set_error("sg_create: no HIP device visible (%s); libsegengine has no CPU fallback",
                 e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    return e != hipSuccess ? (int)e : SG_EUNSUPPORTED;
  }
  SG_CHECK_ARG(device >= 0 && device < count, "sg_create: device %d out of range [0,%d)", device, count);
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) {
    sg_set_error("sg_create: hipGetDeviceProperties: %s", hipGetErrorString(e));
    return (int)e;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    sg_set_error("sg_create: device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    return SG_EUNSUPPORTED;
  }
  sg_ctx* c = new sg_ctx();
  c->device = device;
  c->num_cus = prop.multiProcessorCount;
  *out = c;
  return 0;
}

int sg_destroy(sg_ctx* ctx) {
  delete ctx;
  return 0;
}

int sg_num_cus(const sg_ctx* ctx) { return ctx ? ctx->num_cus : 0; }

// the segment reducer's plan (sg_reduce.h) as its users in every translation unit compute it
int sg_seg_plan(const sg_ctx* ctx, int nout, int nseg, int64_t rows, int C, int vec, int wide8, sg_seg_plan_t* out) {
  SG_CHECK_ARG(out, "sg_seg_plan: null out");
  *out = sg_seg_plan_t{};
  SG_CHECK_ARG(ctx && nout > 0 && nseg > 0 && rows > 0 && C > 0, "sg_seg_plan: bad argument");
  *out = seg_plan_n(nout, ctx->num_cus, nseg, rows, C, vec != 0, wide8 != 0);
  return 0;
}

int sg_fill_f32(sg_ctx* ctx, void* stream, void* p, int64_t n, float value) {
  SG_CHECK_ARG(ctx && (p || n == 0), "sg_fill_f32: null argument");
  if (n <= 0) return 0;
  int64_t blocks = sg_cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float*)p, n, value);
  SG_LAUNCH_CHECK("fill_f32_kernel");
  return 0;
}

int sg_cast(sg_ctx* ctx, void* stream, int src_dtype, int dst_dtype, int64_t n, const void* src, void* dst) {
  SG_CHECK_ARG(ctx && (src || n == 0) && (dst || n == 0) && n >= 0, "sg_cast: bad argument");
  SG_CHECK_ARG((src_dtype == SG_F32 || src_dtype == SG_BF16) && (dst_dtype == SG_F32 || dst_dtype == SG_BF16), "sg_cast: dtype");
  SG_CHECK_ARG((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "sg_cast: pointers must be 16-byte aligned");
  if (n == 0) return 0;
  int64_t blocks = sg_cdiv(n / 4 + 1, 256);
  if (blocks > 8192) blocks = 8192;
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == SG_F32 && dst_dtype == SG_BF16)
    hipLaunchKernelGGL((cast_kernel<float, bf16_t>), dim3((unsigned)blocks), dim3(256), 0, st, (const float*)src, (bf16_t*)dst, n);
  else if (src_dtype == SG_BF16 && dst_dtype == SG_F32)
    hipLaunchKernelGGL((cast_kernel<bf16_t, float>), dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)src, (float*)dst, n);
  else if (src_dtype == SG_F32)
    hipLaunchKernelGGL((cast_kernel<float, float>), dim3((unsigned)blocks), dim3(256), 0, st, (const float*)src, (float*)dst, n);
  else
    hipLaunchKernelGGL((cast_kernel<bf16_t, bf16_t>), dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, n);
  SG_LAUNCH_CHECK("cast_kernel");
  return 0;
}

int sg_u8_to_f32(sg_ctx* ctx, void* stream, int64_t n, const void* src_u8, void* dst_f32, float div, float sub) {
  SG_CHECK_ARG(ctx && (src_u8 || n == 0) && (dst_f32 || n == 0) && n >= 0 && div != 0.f, "sg_u8_to_f32: bad argument");
  if (n == 0) return 0;
  int64_t blocks = sg_cdiv(n, 256);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(u8_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)src_u8,
                     (float*)dst_f32, n, div, sub);
  SG_LAUNCH_CHECK("u8_to_f32_kernel");
  return 0;
}

int sg_trace_mark(sg_ctx* ctx, void* stream, int tag, int end) {
  SG_CHECK_ARG(ctx && tag >= 0 && tag <= 1, "sg_trace_mark: tag %d", tag);
  hipStream_t st = (hipStream_t)stream;
  if (tag == 0 && !end) hipLaunchKernelGGL((sg_trace_mark_kernel<0, 0>), dim3(1), dim3(1), 0, st);
  if (tag == 0 && end) hipLaunchKernelGGL((sg_trace_mark_kernel<0, 1>), dim3(1), dim3(1), 0, st);
  if (tag == 1 && !end) hipLaunchKernelGGL((sg_trace_mark_kernel<1, 0>), dim3(1), dim3(1), 0, st);
  if (tag == 1 && end) hipLaunchKernelGGL((sg_trace_mark_kernel<1, 1>), dim3(1), dim3(1), 0, st);
  SG_LAUNCH_CHECK("sg_trace_mark_kernel");
  return 0;
}

int sg_scale_f32(sg_ctx* ctx, void* stream, void* p, int64_t n, float a) {
  SG_CHECK_ARG(ctx && (p || n == 0), "sg_scale_f32: null argument");
  if (n <= 0) return 0;
  int64_t blocks = sg_cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float*)p, n, a);
  SG_LAUNCH_CHECK("scale_f32_kernel");
  return 0;
}

}  // extern "C"
