// The integer arithmetic of sg_warp_u8 (include/segengine.h), host and device: source positions in 1/65536 pixel, the
// reflect-101 index, the 8-bit bilinear blend, the Q12 colour matrix and the noise term.  Plain C++ on purpose: warp.hip's
// kernel and scripts/warp_emulate.cpp (a host program under the sanitizers) run the same functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/segengine.h"
#include "sg_philox.h"

// The bounds sg_warp_u8 checks before it launches.  With them |a * o| <= 2^24 * 2^14 = 2^38 per product, so
// |X| < 2^46 + 2^39 + 2^15 < 2^47: the int64 sums cannot overflow, and X >> 16 (< 2^31) fits an int with room for its + 1.
constexpr int32_t SG_WARP_A_MAX = 1 << 24;              // |a**| <= 2^24 (256 source pixels per output pixel)
constexpr int64_t SG_WARP_B_LIM = (int64_t)1 << 46;     // |b*| < 2^46
constexpr int SG_WARP_OUT_MAX = 1 << 14;                // OH, OW <= 2^14
constexpr int32_t SG_WARP_M_MAX = 1 << 18;              // |m[c][j]| <= 2^18: 3 * 2^18 * 255 + 2^24 + 2048 < 2^31
constexpr int32_t SG_WARP_OFF_MAX = 1 << 24;            // |off_c| <= 2^24
constexpr int32_t SG_WARP_NOISE_MAX = 1 << 16;          // 0 <= noise_q12 <= 2^16: 2^16 * 510 + 2048 < 2^31

// X (or Y) of output pixel (ox, oy): a_x * ox + a_y * oy + b in int64
__host__ __device__ __forceinline__ int64_t warp_pos(int32_t ax, int32_t ay, int64_t b, int ox, int oy) {
  return (int64_t)ax * ox + (int64_t)ay * oy + b;
}
__host__ __device__ __forceinline__ int warp_floor(int64_t X) { return (int)(X >> 16); }              // x0 of the bilinear form
__host__ __device__ __forceinline__ int warp_weight(int64_t X) { return (int)((X & 0xFFFF) >> 8); }   // wx, 0 .. 255
__host__ __device__ __forceinline__ int warp_round(int64_t X) { return (int)((X + 32768) >> 16); }    // the nearest tap

// reflect-101 (... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...) of any int index, n >= 2: period 2 (n - 1)
__host__ __device__ __forceinline__ int warp_reflect(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  const int p = 2 * (n - 1);
  int r = i % p;
  if (r < 0) r += p;
  return r < n ? r : p - r;
}

// one tap of one pixel: the byte offset of its first channel inside the source's H x W x C slot, or -1 for the fill
template <bool REFLECT>
__host__ __device__ __forceinline__ int warp_tap(int x, int y, int sw, int sh, int W, int C) {
  if (REFLECT) return (warp_reflect(y, sh) * W + warp_reflect(x, sw)) * C;
  return ((unsigned)x < (unsigned)sw && (unsigned)y < (unsigned)sh) ? (y * W + x) * C : -1;
}

// the four weights sum to 65536, so the value stays in 0 .. 255 and the sum below 2^24
__host__ __device__ __forceinline__ int warp_blend(int p00, int p01, int p10, int p11, int wx, int wy) {
  return ((256 - wx) * (256 - wy) * p00 + wx * (256 - wy) * p01 + (256 - wx) * wy * p10 + wx * wy * p11 + 32768) >> 16;
}

__host__ __device__ __forceinline__ int warp_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// row c of the Q12 colour matrix: clamp((m0 v0 + m1 v1 + m2 v2 + off + 2048) >> 12) with an arithmetic shift
__host__ __device__ __forceinline__ int warp_colour(const int32_t* m3, int32_t off, int v0, int v1, int v2) {
  return warp_clamp8((m3[0] * v0 + m3[1] * v1 + m3[2] * v2 + off + 2048) >> 12);
}

// t of one 32-bit word: the sum of its four bytes minus 510 (-510 .. 510, mean 0, standard deviation 147.80)
__host__ __device__ __forceinline__ int warp_noise_t(uint32_t w) {
  return (int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24)) - 510;
}
__host__ __device__ __forceinline__ int warp_noise(int u, int noise_q12, uint32_t w) {
  return warp_clamp8(u + ((noise_q12 * warp_noise_t(w) + 2048) >> 12));
}

// the four words of output pixel `pixel` = oy * OW + ox of sample `sample` under the call's `seed`
__host__ __device__ __forceinline__ Philox4 warp_noise_words(uint32_t pixel, uint64_t sample, uint64_t seed) {
  return sg_philox4x32_10(pixel, (uint32_t)sample, (uint32_t)(sample >> 32), SG_WARP_NOISE_STREAM, (uint32_t)seed,
                          (uint32_t)(seed >> 32) ^ SG_WARP_NOISE_KEY);
}
