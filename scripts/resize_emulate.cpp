// Host walk of csrc/resize_coords.h, the integer arithmetic that sg_resize_fwd / _bwd and sg_prob_resize_accumulate call:
// every (n, m) in 1 ... 96 and the extremes (1, 16384), (16384, 1), (16384, 16383), (16383, 16384).  Taps are read from heap
// blocks of exactly n elements, so a tap that leaves its axis is an AddressSanitizer report here instead of an out-of-bounds
// read on a GPU; every product is repeated in 64 bits and compared, and a signed overflow is an UndefinedBehaviorSanitizer
// report.  The spans of the transpose are checked against a brute-force scan of all outputs, and the weights of every output
// against 1.  A development aid, not a pytest test:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I. scripts/resize_emulate.cpp -o resize_emulate && ./resize_emulate
// (the header is HIP: hipcc compiles this file's host half with the sanitizers; nothing here touches a device).
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "building_detection_amd/csrc/resize_coords.h"

static int fails = 0;
#define REQUIRE(cond, ...)                \
  do {                                    \
    if (!(cond)) {                        \
      std::printf("FAIL: " __VA_ARGS__);  \
      std::printf("\n");                  \
      if (++fails > 20) std::exit(1);     \
    }                                     \
  } while (0)

static long long floor_div_ll(long long a, long long d) {
  long long q = a / d;
  return q - ((a % d) < 0 ? 1 : 0);
}

static long pairs = 0, outputs = 0;

static void walk(int n, int m) {
  ++pairs;
  // heap blocks of exactly n (the input axis) and m (the output axis) elements: x[i] = i, hit[o] counts the reads of dy[o]
  std::vector<int>* xs = new std::vector<int>((size_t)n);
  int* x = xs->data();
  for (int i = 0; i < n; ++i) x[i] = i;
  std::vector<int> span_lo((size_t)n, INT_MAX), span_hi((size_t)n, -1), nrun_lo((size_t)n, INT_MAX), nrun_hi((size_t)n, -1);
  std::vector<float> wsum((size_t)n, 0.f);   // sum over o of the weight onto i, brute force
  for (int o = 0; o < m; ++o) {
    ++outputs;
    // every product again in 64 bits
    const long long num = (2LL * o + 1) * n - m, den = 2LL * m;
    REQUIRE(num <= INT_MAX && num >= INT_MIN && (2LL * o + 1) * n <= INT_MAX, "(%d,%d) o=%d: num %lld leaves int", n, m, o, num);
    const long long fl = floor_div_ll(num, den);
    const RsTap t = rs_taps(o, n, m);
    REQUIRE(rs_fl(o, n, m) == fl, "(%d,%d) o=%d: fl %d != %lld", n, m, o, rs_fl(o, n, m), fl);
    REQUIRE(t.den == den && t.r == num - fl * den && t.r >= 0 && t.r < t.den, "(%d,%d) o=%d: r %d den %d", n, m, o, t.r, t.den);
    // the same taps from the half-pixel definition in exact rationals: in = num / den
    const long long lo = fl < 0 ? 0 : fl, ce = fl + (t.r != 0), hi = ce < 0 ? 0 : (ce > n - 1 ? n - 1 : ce);
    REQUIRE(t.lo == lo && t.hi == hi, "(%d,%d) o=%d: taps (%d,%d) != (%lld,%lld)", n, m, o, t.lo, t.hi, lo, hi);
    REQUIRE(x[t.lo] == t.lo && x[t.hi] == t.hi && t.lo <= t.hi && t.hi - t.lo <= 1, "(%d,%d) o=%d: taps (%d,%d)", n, m, o, t.lo, t.hi);
    // the unsigned form the kernels divide by a FastDiv: num + den > 0 and fl = (num + den) / den - 1
    REQUIRE(num + den > 0 && (num + den) / den - 1 == fl && num + den <= INT_MAX, "(%d,%d) o=%d: unsigned form", n, m, o);
    // weights: numerators sum to den, the floats to 1 within an ulp
    const float f = rs_frac(t);
    REQUIRE(f >= 0.f && f < 1.f, "(%d,%d) o=%d: f = %g", n, m, o, (double)f);
    float ws = 0.f;
    for (int i = t.lo; i <= t.hi; ++i) {
      const float w = rs_weight(t, i);
      ws += w;
      wsum[(size_t)i] += w;
      if (w != 0.f || t.lo == i || t.hi == i) {
        if (o < span_lo[(size_t)i]) span_lo[(size_t)i] = o;
        if (o > span_hi[(size_t)i]) span_hi[(size_t)i] = o;
      }
    }
    REQUIRE(std::fabs(ws - 1.f) <= 1.2e-7f, "(%d,%d) o=%d: weights sum to %.9g", n, m, o, (double)ws);
    if (m == n) REQUIRE(t.lo == o && t.hi == o && t.r == 0, "(%d,%d) o=%d: not the identity", n, m, o);
    // nearest
    const int s = rs_nearest(o, n, m);
    const long long sref = ((2LL * o + 1) * n) / (2LL * m);
    REQUIRE(s == (sref > n - 1 ? n - 1 : sref) && x[s] == s, "(%d,%d) o=%d: nearest %d", n, m, o, s);
    if (o < nrun_lo[(size_t)s]) nrun_lo[(size_t)s] = o;
    if (o > nrun_hi[(size_t)s]) nrun_hi[(size_t)s] = o;
  }
  // the transpose: spans against the brute-force scan; heap block of exactly m elements for the reads of dy
  std::vector<int>* dys = new std::vector<int>((size_t)m);
  int* dy = dys->data();
  for (int o = 0; o < m; ++o) dy[o] = o;
  for (int i = 0; i < n; ++i) {
    for (int k = i > 0 ? i - 1 : 0; k <= i + 1 && k < n; ++k) {
      const long long fn = (2LL * k + 1) * m - n + 2LL * n - 1;
      REQUIRE(fn >= 0 && fn <= INT_MAX && rs_first_num(k, n, m) == fn, "(%d,%d) k=%d: first_num %lld", n, m, k, fn);
    }
    const long long nn = 2LL * m * (i + 1) - n + 2LL * n - 1;
    REQUIRE(nn >= 0 && nn <= INT_MAX && rs_nfirst_num(i + 1, n, m) == nn, "(%d,%d) i=%d: nfirst_num %lld", n, m, i, nn);
    int o0, o1;
    rs_span(i, n, m, o0, o1);
    REQUIRE(o0 >= 0 && o1 <= m, "(%d,%d) i=%d: span [%d,%d)", n, m, i, o0, o1);
    REQUIRE(o1 - o0 <= 2 * m / n + 1, "(%d,%d) i=%d: span of %d > %d", n, m, i, o1 - o0, 2 * m / n + 1);
    if (span_hi[(size_t)i] >= 0)
      REQUIRE(o0 <= span_lo[(size_t)i] && span_hi[(size_t)i] < o1, "(%d,%d) i=%d: span [%d,%d) misses [%d,%d]", n, m, i, o0, o1,
              span_lo[(size_t)i], span_hi[(size_t)i]);
    float acc = 0.f;
    for (int o = o0; o < o1; ++o) {
      REQUIRE(dy[o] == o, "read");
      acc += rs_weight(rs_taps(o, n, m), i);
    }
    REQUIRE(acc == wsum[(size_t)i], "(%d,%d) i=%d: gathered weight %.9g != scattered %.9g", n, m, i, (double)acc, (double)wsum[(size_t)i]);
    // first(k) is the smallest o with fl(o) >= k
    const int q = rs_first(i, n, m);
    REQUIRE((q == m || rs_fl(q, n, m) >= i) && (q == 0 || rs_fl(q - 1, n, m) < i), "(%d,%d) first(%d) = %d", n, m, i, q);
    // nearest runs: exactly the scanned ones
    const int r0 = rs_nfirst(i, n, m), r1 = rs_nfirst(i + 1, n, m);
    REQUIRE(r0 >= 0 && r1 <= m && r0 <= r1, "(%d,%d) i=%d: run [%d,%d)", n, m, i, r0, r1);
    if (nrun_hi[(size_t)i] >= 0)
      REQUIRE(r0 == nrun_lo[(size_t)i] && r1 == nrun_hi[(size_t)i] + 1, "(%d,%d) i=%d: run [%d,%d) != [%d,%d]", n, m, i, r0, r1,
              nrun_lo[(size_t)i], nrun_hi[(size_t)i]);
    else
      REQUIRE(r0 == r1, "(%d,%d) i=%d: run [%d,%d) of a source no output reads", n, m, i, r0, r1);
    for (int o = r0; o < r1; ++o) REQUIRE(dy[o] == o, "read");
  }
  REQUIRE(rs_nfirst(n, n, m) == m, "(%d,%d): nfirst(n) = %d", n, m, rs_nfirst(n, n, m));
  delete xs;
  delete dys;
}

int main() {
  for (int n = 1; n <= 96; ++n)
    for (int m = 1; m <= 96; ++m) walk(n, m);
  walk(1, RS_MAX_EXTENT);
  walk(RS_MAX_EXTENT, 1);
  walk(RS_MAX_EXTENT, RS_MAX_EXTENT - 1);
  walk(RS_MAX_EXTENT - 1, RS_MAX_EXTENT);
  walk(RS_MAX_EXTENT, RS_MAX_EXTENT);
  std::printf("%ld size pairs, %ld outputs walked, %d failures\n", pairs, outputs, fails);
  return fails ? 1 : 0;
}
