// Dropout / SpatialDropout2D: y = x * scale where the element's mask word is >= thr, +0 elsewhere.  The mask is never
// stored: element i has the mask index
//   idx = first + i                                  (element form, hwc == 0)
//   idx = first + (i div hwc) * c + i mod c          (spatial form: one decision per image and channel)
// and its word is word idx & 3 of Philox4x32-10 at counter (q mod 2^32, q >> 32, stream, step), q = idx >> 2, key (k0, k1).  The
// forward and the backward are the same call (x -> y, dy -> dx), and {k0, k1, step} are read from device memory, so a captured
// launch sees each replay's values.  One grid-stride element-wise kernel on pointwise.hip's skeleton:
//   vector form   a thread takes the 4 consecutive elements that share one Philox call (fp32: one 16-byte access; bf16: two calls,
//                 8 elements, one 16-byte access).  Needs 16-byte aligned operands, first % 4 == 0 and, in the spatial form,
//                 c % 4 == 0, so that element 4j .. 4j + 3 are mask index 4q .. 4q + 3.  The ragged tail (n mod 4 or 8 elements)
//                 is finished by the scalar form inside the same launch.
//   scalar form   one call per element, word idx & 3.  Everything else.
// Both forms evaluate the same function of (idx, seed words): the same bits whatever the form, the grid or the alignment.  64-bit
// index arithmetic throughout (the divisions take the compiler's 32-bit path when the operands fit).  No LDS, no atomics.
#include "sg_common.h"
#include "sg_philox.h"

namespace {

constexpr int64_t EW_CAP = 8192;   // as pointwise.hip's element-wise launches

struct DropArgs {
  uint64_t n, hwc, first;
  uint32_t c, stream, thr;
  float scale;
};

__device__ __forceinline__ uint64_t mask_index(const DropArgs& a, uint64_t i) {
  if (a.hwc == 0) return a.first + i;
  const uint64_t img = i / a.hwc;
  return a.first + img * a.c + (i - img * a.hwc) % a.c;
}

// x and y may be the same tensor (no __restrict__): a thread reads its elements before it writes them
template <int V, typename T>
__global__ __launch_bounds__(256) void dropout_kernel(const T* x, T* y, const DropArgs a, const uint32_t* __restrict__ rng) {
  const uint32_t k0 = rng[0], k1 = rng[1], step = rng[2];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t done = 0;
  if constexpr (V > 1) {
    const uint64_t nv = a.n / V;
    for (uint64_t i = t0; i < nv; i += stride) {
      float v[V];
      ldv<V>(x + i * V, v);
#pragma unroll
      for (int g = 0; g < V / 4; ++g) {
        const Philox4 w = sg_mask_words(mask_index(a, i * V + 4 * g) >> 2, a.stream, step, k0, k1);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * g + k] = w.w[k] >= a.thr ? v[4 * g + k] * a.scale : 0.f;
      }
      stv<V>(y + i * V, v);
    }
    done = nv * V;
  }
  for (uint64_t i = done + t0; i < a.n; i += stride) {
    const uint64_t idx = mask_index(a, i);
    const Philox4 w = sg_mask_words(idx >> 2, a.stream, step, k0, k1);
    const uint32_t s = (uint32_t)idx & 3u;
    const uint32_t u = s == 0 ? w.w[0] : s == 1 ? w.w[1] : s == 2 ? w.w[2] : w.w[3];
    st1<T>(y + i, u >= a.thr ? ld1<T>(x + i) * a.scale : 0.f);
  }
}

}  // namespace

extern "C" {

int sg_dropout(sg_ctx* ctx, void* stream, int dtype, int64_t n, int64_t hwc, int c, int64_t first, uint32_t rng_stream, uint32_t thr,
               float scale, const void* rng_dev, const void* x, void* y) {
  SG_CHECK_ARG(ctx && rng_dev && x && y, "sg_dropout: null argument");
  SG_CHECK_ARG(n >= 0 && hwc >= 0, "sg_dropout: negative size (n=%lld hwc=%lld)", (long long)n, (long long)hwc);
  if (hwc > 0) {
    SG_CHECK_ARG(c > 0 && hwc % c == 0, "sg_dropout: hwc=%lld is no multiple of c=%d", (long long)hwc, c);
    SG_CHECK_ARG(n % hwc == 0, "sg_dropout: n=%lld is no multiple of hwc=%lld", (long long)n, (long long)hwc);
  }
  SG_CHECK_ARG(((uintptr_t)rng_dev & 3) == 0, "sg_dropout: rng_dev is not 4-byte aligned");
  DropArgs a;
  a.n = (uint64_t)n; a.hwc = (uint64_t)hwc; a.first = (uint64_t)first;
  a.c = hwc > 0 ? (uint32_t)c : 1u; a.stream = rng_stream; a.thr = thr; a.scale = scale;
  const bool vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && (a.first & 3) == 0 && (hwc == 0 || c % 4 == 0);
  hipStream_t st = (hipStream_t)stream;
  SG_DTYPE_SWITCH(dtype, "sg_dropout", {
    if (n == 0) return 0;
    constexpr int V = 16 / (int)sizeof(T);   // elements of one 16-byte access: 4 fp32 (one Philox call), 8 bf16 (two)
    if (vec && n >= V)
      hipLaunchKernelGGL((dropout_kernel<V, T>), dim3(ew_blocks(n / V, EW_CAP)), dim3(256), 0, st, (const T*)x, (T*)y, a,
                         (const uint32_t*)rng_dev);
    else
      hipLaunchKernelGGL((dropout_kernel<1, T>), dim3(ew_blocks(n, EW_CAP)), dim3(256), 0, st, (const T*)x, (T*)y, a,
                         (const uint32_t*)rng_dev);
  });
  SG_LAUNCH_CHECK("dropout_kernel");
  return 0;
}

}  // extern "C"
