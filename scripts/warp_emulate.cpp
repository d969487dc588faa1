// Host walk of csrc/warp_coords.h, the integer arithmetic sg_warp_u8's kernel calls: positions at the extreme coefficient
// bounds, the reflect index far outside, whole tiles cut from 1-pixel and 2-pixel sources, the blend, the colour matrix and
// the noise at their extremes.  Every source is a heap block of exactly its slot's size, so a tap that leaves it is an
// AddressSanitizer report here instead of an out-of-bounds read on a GPU, and an overflowing sum is an UndefinedBehavior-
// Sanitizer report.  A development aid, not a pytest test:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I. scripts/warp_emulate.cpp -o warp_emulate && ./warp_emulate
// (the header is HIP: hipcc compiles this file's host half with the sanitizers; nothing here touches a device).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "building_detection_amd/csrc/warp_coords.h"

static int fails = 0;
#define REQUIRE(cond, ...)                \
  do {                                    \
    if (!(cond)) {                        \
      std::printf("FAIL: " __VA_ARGS__);  \
      std::printf("\n");                  \
      if (++fails > 20) std::exit(1);     \
    }                                     \
  } while (0)

// the definition, one step at a time: walk |i| steps over ... 2 1 0 1 2 ... n-1 n-2 ...
static int reflect_walk(long long i, int n) {
  const long long p = 2LL * (n - 1);
  long long j = ((i % p) + p) % p;
  return (int)(j < n ? j : p - j);
}

static void positions() {
  const int32_t as[] = {-SG_WARP_A_MAX, -65536, -1, 0, 1, 65536, SG_WARP_A_MAX};
  const int64_t bs[] = {-(SG_WARP_B_LIM - 1), -65537, -65536, -1, 0, 1, 255, 256, 65535, 65536, SG_WARP_B_LIM - 1};
  const int os[] = {0, 1, 3, SG_WARP_OUT_MAX - 4, SG_WARP_OUT_MAX - 1};
  long n = 0;
  for (int32_t ax : as)
    for (int32_t ay : as)
      for (int64_t b : bs)
        for (int ox : os)
          for (int oy : os) {
            int64_t X = warp_pos(ax, ay, b, ox, oy);
            for (int k = 0; k < 4; ++k, X += ax) {   // the kernel's own stepping along four pixels
              const int x0 = warp_floor(X), w = warp_weight(X), xn = warp_round(X);
              REQUIRE((int64_t)x0 * 65536 <= X && X < ((int64_t)x0 + 1) * 65536, "floor of %lld is %d", (long long)X, x0);
              REQUIRE(w >= 0 && w <= 255 && w == (int)((X - (int64_t)x0 * 65536) >> 8), "weight of %lld is %d", (long long)X, w);
              REQUIRE(xn == x0 || xn == x0 + 1, "nearest of %lld is %d beside %d", (long long)X, xn, x0);
              const int x1 = x0 + 1;   // the second tap's index must not overflow
              for (int nn : {2, 3, 512}) {
                REQUIRE(warp_reflect(x0, nn) == reflect_walk(x0, nn) && warp_reflect(x1, nn) == reflect_walk(x1, nn),
                        "reflect(%d or %d, %d)", x0, x1, nn);
              }
              ++n;
            }
          }
  std::printf("positions: %ld walked\n", n);
}

static void reflections() {
  for (int n : {2, 3, 4, 5, 17, 512, 16384}) {
    std::vector<unsigned char> row((size_t)n, 1);
    for (long long i = -5LL * n - 3; i <= 5LL * n + 3; ++i) {
      const int r = warp_reflect((int)i, n);
      REQUIRE(r == reflect_walk(i, n), "reflect(%lld, %d) = %d", i, n, r);
      REQUIRE(row[(size_t)r] == 1, "reflect(%lld, %d) reads outside", i, n);
    }
    for (long long i : {(long long)INT32_MIN, (long long)INT32_MIN + 1, -1099511627LL, 1099511627LL, (long long)INT32_MAX - 1, (long long)INT32_MAX}) {
      const int r = warp_reflect((int)i, n);
      REQUIRE(r == reflect_walk(i, n) && row[(size_t)r] == 1, "reflect(%lld, %d) = %d", i, n, r);
    }
  }
  std::printf("reflections: done\n");
}

// one output tile through the kernel's tap / blend calls; the source is a heap block of exactly S * H * W * C bytes
template <bool NEAREST, bool REFLECT>
static void tile(int H, int W, int C, int sh, int sw, const int32_t a[4], const int64_t b[2], int OH, int OW, int fill) {
  std::vector<unsigned char> src((size_t)H * W * C);
  for (size_t i = 0; i < src.size(); ++i) src[i] = (unsigned char)(i * 37 + 11);
  std::vector<unsigned char> dst((size_t)OH * OW * C);
  const unsigned char* img = src.data();
  for (int oy = 0; oy < OH; ++oy)
    for (int ox = 0; ox < OW; ++ox) {
      const int64_t X = warp_pos(a[0], a[1], b[0], ox, oy), Y = warp_pos(a[2], a[3], b[1], ox, oy);
      for (int c = 0; c < C; ++c) {
        int v;
        if (NEAREST) {
          const int q = warp_tap<REFLECT>(warp_round(X), warp_round(Y), sw, sh, W, C);
          v = q >= 0 ? img[q + c] : fill;
          bool from_source = q < 0;
          for (int y = 0; y < sh && !from_source; ++y)
            for (int x = 0; x < sw; ++x) from_source |= img[(y * W + x) * C + c] == v;
          REQUIRE(from_source, "nearest value %d is neither a source value nor the fill", v);
        } else {
          const int x0 = warp_floor(X), y0 = warp_floor(Y);
          const int q00 = warp_tap<REFLECT>(x0, y0, sw, sh, W, C), q01 = warp_tap<REFLECT>(x0 + 1, y0, sw, sh, W, C);
          const int q10 = warp_tap<REFLECT>(x0, y0 + 1, sw, sh, W, C), q11 = warp_tap<REFLECT>(x0 + 1, y0 + 1, sw, sh, W, C);
          REQUIRE(!REFLECT || (q00 >= 0 && q01 >= 0 && q10 >= 0 && q11 >= 0), "a reflected tap fell outside");
          v = warp_blend(q00 >= 0 ? img[q00 + c] : fill, q01 >= 0 ? img[q01 + c] : fill, q10 >= 0 ? img[q10 + c] : fill,
                         q11 >= 0 ? img[q11 + c] : fill, warp_weight(X), warp_weight(Y));
        }
        REQUIRE(v >= 0 && v <= 255, "value %d", v);
        dst[((size_t)oy * OW + ox) * C + c] = (unsigned char)v;
      }
    }
}

static void tiny_sources() {
  const int32_t maps[][4] = {{65536, 0, 0, 65536},      {21845, 3000, -3000, 21845},       {-65536, 0, 0, -65536},
                             {0, 65536, -65536, 0},     {SG_WARP_A_MAX, -SG_WARP_A_MAX, SG_WARP_A_MAX, SG_WARP_A_MAX},
                             {1, 0, 0, 1}};
  const int64_t offs[][2] = {{0, 0},          {-10 * 65536 - 1, 7 * 65536 + 32768}, {32768, 32768}, {SG_WARP_B_LIM - 1, -(SG_WARP_B_LIM - 1)},
                             {-(SG_WARP_B_LIM - 1), SG_WARP_B_LIM - 1}};
  int n = 0;
  for (const auto& a : maps)
    for (const auto& b : offs)
      for (int C : {1, 3}) {
        // the source fills its slot exactly: any index past the extent is past the heap block
        tile<false, false>(1, 1, C, 1, 1, a, b, 9, 11, 128);
        tile<true, false>(1, 1, C, 1, 1, a, b, 9, 11, 0);
        tile<false, false>(2, 2, C, 2, 2, a, b, 9, 11, 128);
        tile<true, false>(2, 2, C, 2, 2, a, b, 9, 11, 0);
        tile<false, true>(2, 2, C, 2, 2, a, b, 9, 11, 128);
        tile<true, true>(2, 2, C, 2, 2, a, b, 9, 11, 0);
        tile<false, true>(3, 2, C, 3, 2, a, b, 9, 11, 128);
        tile<false, false>(2, 1, C, 2, 1, a, b, 9, 11, 128);
        n += 8;
      }
  std::printf("tiny sources: %d tiles\n", n);
}

static void values() {
  for (int wx = 0; wx < 256; ++wx)
    for (int wy = 0; wy < 256; ++wy) {
      REQUIRE(warp_blend(255, 255, 255, 255, wx, wy) == 255 && warp_blend(0, 0, 0, 0, wx, wy) == 0, "blend at (%d, %d)", wx, wy);
      REQUIRE(warp_blend(7, 255, 255, 255, 0, 0) == 7, "a tap of weight 0 contributes");
    }
  REQUIRE(warp_blend(10, 21, 0, 0, 128, 0) == 16, "the half-pixel blend is (p0 + p1 + 1) >> 1");
  const int32_t ms[] = {-SG_WARP_M_MAX, -4096, 0, 4096, SG_WARP_M_MAX};
  const int32_t offs[] = {-SG_WARP_OFF_MAX, 0, SG_WARP_OFF_MAX};
  for (int32_t m0 : ms)
    for (int32_t m1 : ms)
      for (int32_t m2 : ms)
        for (int32_t off : offs)
          for (int v : {0, 1, 128, 255}) {
            const int32_t m3[3] = {m0, m1, m2};
            const int u = warp_colour(m3, off, v, v, 255 - v);
            REQUIRE(u >= 0 && u <= 255, "colour value %d", u);
          }
  const int32_t id[3] = {4096, 0, 0};
  for (int v = 0; v < 256; ++v) REQUIRE(warp_colour(id, 0, v, 255 - v, 3) == v, "the identity matrix changes %d", v);
  REQUIRE(warp_noise_t(0u) == -510 && warp_noise_t(0xFFFFFFFFu) == 510 && warp_noise_t(0x80FF007Fu) == 0, "t of a word");
  for (uint32_t w : {0u, 0xFFFFFFFFu, 0x12345678u})
    for (int q : {0, 1, 4096, SG_WARP_NOISE_MAX})
      for (int u : {0, 128, 255}) {
        const int r = warp_noise(u, q, w);
        REQUIRE(r >= 0 && r <= 255, "noise value %d", r);
      }
  // Random123's known answer through the kernel's own generator call: counter (pixel, sample), key (seed) with both
  // constants folded back out
  const Philox4 z = warp_noise_words(0x243F6A88u, ((uint64_t)0x13198A2Eu << 32) | 0x85A308D3u,
                                     ((uint64_t)(0x299F31D0u ^ SG_WARP_NOISE_KEY) << 32) | 0xA4093822u);
  const Philox4 k = sg_philox4x32_10(0x243F6A88u, 0x85A308D3u, 0x13198A2Eu, 0x03707344u, 0xA4093822u, 0x299F31D0u);
  REQUIRE(k.w[0] == 0xd16cfe09u && k.w[1] == 0x94fdccebu && k.w[2] == 0x5001e420u && k.w[3] == 0x24126ea1u, "Philox known answer");
  const Philox4 z2 = sg_philox4x32_10(0x243F6A88u, 0x85A308D3u, 0x13198A2Eu, SG_WARP_NOISE_STREAM, 0xA4093822u, 0x299F31D0u);
  REQUIRE(z.w[0] == z2.w[0] && z.w[3] == z2.w[3], "the noise words' counter and key layout");
  std::printf("values: done\n");
}

int main() {
  positions();
  reflections();
  tiny_sources();
  values();
  std::printf(fails ? "%d FAILURES\n" : "warp_emulate: all checks passed\n", fails);
  return fails ? 1 : 0;
}
