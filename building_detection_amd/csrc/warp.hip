// sg_warp_u8 (include/segengine.h): affine warps and colour jitter of uint8 tiles, all in integers (warp_coords.h).
// Memory-bound: per output byte one store and up to four cached source reads.  One output tile per blockIdx.y, its item read
// from the by-value table (a uniform index: scalar loads of the kernel-argument segment); a thread owns WARP_PX consecutive
// pixels of one output row, steps the source position by (a00, a10) along them and stores the WARP_PX * C bytes as C 32-bit
// words when the row is word-aligned, else byte by byte.  The kernel is a template on C, nearest / bilinear, constant /
// reflect and colour on / off, so the plain label path carries none of the colour code; a block whose item asks for another
// combination than its launch returns at once (sg_warp_u8 launches every combination its table holds).
#include "sg_common.h"
#include "warp_coords.h"

namespace {

constexpr int WARP_PX = 4;

struct WarpTable {
  sg_warp_item it[SG_WARP_MAX_ITEMS];
};
static_assert(sizeof(sg_warp_item) == 112, "sg_warp_item is 28 words");
static_assert(sizeof(WarpTable) <= 3584, "the item table and the other arguments stay inside a 4 KB kernel-argument segment");

template <int C, bool NEAREST, bool REFLECT, bool COLOR>
__global__ __launch_bounds__(256) void warp_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                      const unsigned char* __restrict__ luts, const WarpTable tab, int H, int W,
                                                      int OH, int OW, int qw, int packed, uint64_t seed) {
  const sg_warp_item& it = tab.it[blockIdx.y];
  constexpr int mine = (NEAREST ? SG_WARP_NEAREST : 0) | (REFLECT ? SG_WARP_REFLECT : 0) | (COLOR ? SG_WARP_COLOR : 0);
  if (it.flags != mine) return;
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= OH * qw) return;
  const int oy = t / qw;
  const int ox0 = (t - oy * qw) * WARP_PX;
  const unsigned char* __restrict__ img = src + it.src * (H * W * C);
  const int sw = it.sw, sh = it.sh, fill = it.fill;
  // whole-pixel maps (the identity, the symmetries, whole shifts) have wx = wy = 0 everywhere: the blend is its first tap
  const bool whole = !NEAREST && ((it.a00 | it.a01 | it.a10 | it.a11) & 0xFFFF) == 0 && (it.b0 & 0xFF00) == 0 && (it.b1 & 0xFF00) == 0;
  int64_t X = warp_pos(it.a00, it.a01, it.b0, ox0, oy);
  int64_t Y = warp_pos(it.a10, it.a11, it.b1, ox0, oy);
  unsigned int word[C];
#pragma unroll
  for (int j = 0; j < C; ++j) word[j] = 0u;
#pragma unroll
  for (int k = 0; k < WARP_PX; ++k, X += it.a00, Y += it.a10) {
    int v[C];
    if (NEAREST || whole) {
      const int q = NEAREST ? warp_tap<REFLECT>(warp_round(X), warp_round(Y), sw, sh, W, C)
                            : warp_tap<REFLECT>(warp_floor(X), warp_floor(Y), sw, sh, W, C);
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = q >= 0 ? img[q + c] : fill;
    } else {
      const int x0 = warp_floor(X), y0 = warp_floor(Y), wx = warp_weight(X), wy = warp_weight(Y);
      const int q00 = warp_tap<REFLECT>(x0, y0, sw, sh, W, C), q01 = warp_tap<REFLECT>(x0 + 1, y0, sw, sh, W, C);
      const int q10 = warp_tap<REFLECT>(x0, y0 + 1, sw, sh, W, C), q11 = warp_tap<REFLECT>(x0 + 1, y0 + 1, sw, sh, W, C);
#pragma unroll
      for (int c = 0; c < C; ++c)
        v[c] = warp_blend(q00 >= 0 ? img[q00 + c] : fill, q01 >= 0 ? img[q01 + c] : fill, q10 >= 0 ? img[q10 + c] : fill,
                          q11 >= 0 ? img[q11 + c] : fill, wx, wy);
    }
    if constexpr (COLOR && C == 3) {
      int u[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) u[c] = warp_colour(it.m + 3 * c, it.off[c], v[0], v[1], v[2]);
      if (luts != nullptr) {
        const unsigned char* __restrict__ lut = luts + (int)blockIdx.y * 768;
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = lut[c * 256 + u[c]];
      }
      if (it.noise_q12 > 0) {
        const Philox4 w = warp_noise_words((uint32_t)(oy * OW + ox0 + k), it.sample, seed);
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = warp_noise(u[c], it.noise_q12, w.w[c]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = u[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int b = k * C + c;
      word[b >> 2] |= (unsigned int)v[c] << (8 * (b & 3));
    }
  }
  const int off = (int)blockIdx.y * (OH * OW * C) + (oy * OW + ox0) * C;
  if (packed) {
    unsigned int* __restrict__ d = reinterpret_cast<unsigned int*>(dst + off);
#pragma unroll
    for (int j = 0; j < C; ++j) d[j] = word[j];
  } else {
    const int nb = min(WARP_PX, OW - ox0) * C;
#pragma unroll
    for (int b = 0; b < WARP_PX * C; ++b)
      if (b < nb) dst[off + b] = (unsigned char)(word[b >> 2] >> (8 * (b & 3)));
  }
}

template <int C, bool NEAREST, bool REFLECT, bool COLOR>
void warp_launch(hipStream_t st, dim3 grid, const void* src, void* dst, const void* luts, const WarpTable& tab, int H, int W, int OH,
                 int OW, int qw, int packed, uint64_t seed) {
  hipLaunchKernelGGL((warp_u8_kernel<C, NEAREST, REFLECT, COLOR>), grid, dim3(256), 0, st, (const unsigned char*)src,
                     (unsigned char*)dst, (const unsigned char*)luts, tab, H, W, OH, OW, qw, packed, seed);
}

inline bool warp_abs_le(int64_t v, int64_t lim) { return v >= -lim && v <= lim; }

}  // namespace

extern "C" int sg_warp_u8(sg_ctx* ctx, void* stream, int S, int H, int W, int C, const void* src_u8, int N, const sg_warp_item* items,
                          const void* luts_u8, uint64_t seed, int OH, int OW, void* dst_u8) {
  SG_CHECK_ARG(ctx && src_u8 && items && dst_u8 && S > 0 && H > 0 && W > 0, "sg_warp_u8: bad argument");
  SG_CHECK_ARG(C == 1 || C == 3, "sg_warp_u8: C = %d (1 or 3)", C);
  SG_CHECK_ARG(N >= 1 && N <= SG_WARP_MAX_ITEMS, "sg_warp_u8: N = %d outside [1, %d]", N, SG_WARP_MAX_ITEMS);
  SG_CHECK_ARG(OH >= 1 && OH <= SG_WARP_OUT_MAX && OW >= 1 && OW <= SG_WARP_OUT_MAX, "sg_warp_u8: output of %d x %d outside [1, %d]",
               OH, OW, SG_WARP_OUT_MAX);
  SG_CHECK_ARG((int64_t)S * H * W * C < (1ll << 31) && (int64_t)N * OH * OW * C < (1ll << 31),
               "sg_warp_u8: tensors of %d x %d x %d x %d / %d x %d x %d x %d bytes exceed 2 GiB", S, H, W, C, N, OH, OW, C);
  WarpTable tab;
  unsigned combos = 0;   // bit f: some item has flags == f
  for (int i = 0; i < N; ++i) {
    const sg_warp_item& a = items[i];
    SG_CHECK_ARG(a.src >= 0 && a.src < S, "sg_warp_u8: item %d: source %d outside [0, %d)", i, a.src, S);
    SG_CHECK_ARG(a.sh >= 1 && a.sh <= H && a.sw >= 1 && a.sw <= W, "sg_warp_u8: item %d: extent %d x %d outside the %d x %d slot", i,
                 a.sh, a.sw, H, W);
    SG_CHECK_ARG((a.flags & ~(SG_WARP_NEAREST | SG_WARP_REFLECT | SG_WARP_COLOR)) == 0, "sg_warp_u8: item %d: unknown flags %#x", i,
                 a.flags);
    SG_CHECK_ARG(a.fill >= 0 && a.fill <= 255, "sg_warp_u8: item %d: fill = %d outside [0, 255]", i, a.fill);
    SG_CHECK_ARG(warp_abs_le(a.a00, SG_WARP_A_MAX) && warp_abs_le(a.a01, SG_WARP_A_MAX) && warp_abs_le(a.a10, SG_WARP_A_MAX) &&
                     warp_abs_le(a.a11, SG_WARP_A_MAX),
                 "sg_warp_u8: item %d: a coefficient of (%d, %d, %d, %d) exceeds 2^24 in magnitude", i, a.a00, a.a01, a.a10, a.a11);
    SG_CHECK_ARG(warp_abs_le(a.b0, SG_WARP_B_LIM - 1) && warp_abs_le(a.b1, SG_WARP_B_LIM - 1),
                 "sg_warp_u8: item %d: an offset of (%lld, %lld) reaches 2^46 in magnitude", i, (long long)a.b0, (long long)a.b1);
    SG_CHECK_ARG(!(a.flags & SG_WARP_REFLECT) || (a.sh >= 2 && a.sw >= 2), "sg_warp_u8: item %d: reflect needs an extent of at least 2 x 2, got %d x %d",
                 i, a.sh, a.sw);
    if (a.flags & SG_WARP_COLOR) {
      SG_CHECK_ARG(C == 3, "sg_warp_u8: item %d: colour needs C = 3", i);
      for (int k = 0; k < 9; ++k)
        SG_CHECK_ARG(warp_abs_le(a.m[k], SG_WARP_M_MAX), "sg_warp_u8: item %d: m[%d] = %d exceeds 2^18 in magnitude", i, k, a.m[k]);
      for (int k = 0; k < 3; ++k)
        SG_CHECK_ARG(warp_abs_le(a.off[k], SG_WARP_OFF_MAX), "sg_warp_u8: item %d: off[%d] = %d exceeds 2^24 in magnitude", i, k, a.off[k]);
      SG_CHECK_ARG(a.noise_q12 >= 0 && a.noise_q12 <= SG_WARP_NOISE_MAX, "sg_warp_u8: item %d: noise_q12 = %d outside [0, 2^16]", i,
                   a.noise_q12);
    }
    tab.it[i] = a;
    combos |= 1u << a.flags;
  }
  for (int i = N; i < SG_WARP_MAX_ITEMS; ++i) tab.it[i] = tab.it[0];   // never indexed: the grid has N rows
  const int qw = (int)sg_cdiv(OW, WARP_PX);
  const int packed = (OW % 4 == 0 && ((uintptr_t)dst_u8 & 3) == 0) ? 1 : 0;
  const dim3 grid((unsigned)sg_cdiv((int64_t)OH * qw, 256), (unsigned)N);
  hipStream_t st = (hipStream_t)stream;
#define SG_WARP_CASE(CC, NE, RE, CO)                                                                                \
  if (C == CC && (combos & (1u << ((NE ? SG_WARP_NEAREST : 0) | (RE ? SG_WARP_REFLECT : 0) | (CO ? SG_WARP_COLOR : 0))))) { \
    warp_launch<CC, NE, RE, CO>(st, grid, src_u8, dst_u8, luts_u8, tab, H, W, OH, OW, qw, packed, seed);            \
    SG_LAUNCH_CHECK("warp_u8_kernel");                                                                              \
  }
  SG_WARP_CASE(1, false, false, false)
  SG_WARP_CASE(1, true, false, false)
  SG_WARP_CASE(1, false, true, false)
  SG_WARP_CASE(1, true, true, false)
  SG_WARP_CASE(3, false, false, false)
  SG_WARP_CASE(3, true, false, false)
  SG_WARP_CASE(3, false, true, false)
  SG_WARP_CASE(3, true, true, false)
  SG_WARP_CASE(3, false, false, true)
  SG_WARP_CASE(3, true, false, true)
  SG_WARP_CASE(3, false, true, true)
  SG_WARP_CASE(3, true, true, true)
#undef SG_WARP_CASE
  return 0;
}
