// Arbitrary-size resize (sg_resize_fwd / _bwd, sg_prob_resize_accumulate): the per-axis coordinate arithmetic, stated once
// and in integers, so that the forward and the gather that is its transpose agree on every tap by construction.  For input
// extent n, output extent m (both in [1, RS_MAX_EXTENT]) and output index o:
//     num = (2o + 1) n - m      den = 2m      fl = floor(num / den)      r = num - fl den    (0 <= r < den)
//   bilinear:  lo = max(fl, 0)   hi = min(max(fl + (r != 0), 0), n - 1)   f = (float)r / (float)den
//   nearest:   src = min(floor((2o + 1) n / (2m)), n - 1)
// which is tf.image.resize's half-pixel rule in = (o + 1/2) n / m - 1/2, lo = max(floor(in), 0), hi = min(ceil(in), n - 1),
// f = in - floor(in).  Every product stays below 2^31: (2o + 1) n <= 32767 * 16384 < 2^29 + 2^24.  r < den <= 2^15, so f is
// one correctly rounded division; m == n gives lo = hi = o, f = 0.
// Host and device: scripts/resize_emulate.cpp walks this header on the host.  A divisor comes either as a plain int (the
// host walk, tests) or as a FastDiv (the kernels): rs_floor_div is the one place that differs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

#define RS_MAX_EXTENT 16384

// floor(a / d) for d > 0 and any a
RS_HD int rs_floor_div(int a, int d) {
  const int q = a / d;
  return q - ((a % d) < 0 ? 1 : 0);
}

struct RsTap {
  int lo, hi;   // the two input positions, lo <= hi
  int r, den;   // f = r / den; the weight of lo is (den - r) / den
};

// the bilinear taps of output o, given fl = floor(((2o + 1) n - m) / (2m)) (rs_fl below, or a fast division of the same integers)
RS_HD RsTap rs_taps_from_fl(int o, int n, int m, int fl) {
  RsTap t;
  t.den = 2 * m;
  t.r = (2 * o + 1) * n - m - fl * t.den;
  const int up = fl + (t.r != 0 ? 1 : 0);
  t.lo = fl < 0 ? 0 : fl;
  t.hi = up < 0 ? 0 : (up > n - 1 ? n - 1 : up);
  return t;
}

RS_HD int rs_fl(int o, int n, int m) { return rs_floor_div((2 * o + 1) * n - m, 2 * m); }

RS_HD RsTap rs_taps(int o, int n, int m) { return rs_taps_from_fl(o, n, m, rs_fl(o, n, m)); }

RS_HD float rs_frac(const RsTap& t) { return (float)t.r / (float)t.den; }

// what dy[o] contributes to dx[i]: (lo == i ? 1 - f : 0) + (hi == i ? f : 0)
RS_HD float rs_weight(const RsTap& t, int i) {
  const float f = rs_frac(t);
  return (t.lo == i ? 1.0f - f : 0.0f) + (t.hi == i ? f : 0.0f);
}

RS_HD int rs_nearest(int o, int n, int m) {
  const int s = ((2 * o + 1) * n) / (2 * m);
  return s > n - 1 ? n - 1 : s;
}

// ---- the transpose: which outputs can touch input i -----------------------------------------------------------------------
// first(k) = clamp(ceil(((2k + 1) m - n) / (2n)), 0, m): the smallest o with fl(o) >= k (m if there is none), k >= 0.
// rs_first_num is the numerator of the floor form, >= 0 for k >= 0: first = clamp(floor(rs_first_num / (2n)), 0, m).
RS_HD int rs_first_num(int k, int n, int m) { return (2 * k + 1) * m - n + 2 * n - 1; }

RS_HD int rs_clamp_first(int q, int m) { return q < 0 ? 0 : (q > m ? m : q); }

RS_HD int rs_first(int k, int n, int m) { return rs_clamp_first(rs_first_num(k, n, m) / (2 * n), m); }

// bilinear: outputs o in [o0, o1) have lo(o) == i or hi(o) == i (a superset: an o of the span may weigh 0); at most
// floor(2m / n) + 1 of them, none at all for some i when m < n.  q_prev = first(i - 1) and q_next = first(i + 1) where they
// are needed.
RS_HD void rs_span_from_first(int i, int n, int m, int q_prev, int q_next, int& o0, int& o1) {
  o0 = i == 0 ? 0 : q_prev;
  o1 = i == n - 1 ? m : q_next;
}

RS_HD void rs_span(int i, int n, int m, int& o0, int& o1) {
  rs_span_from_first(i, n, m, i == 0 ? 0 : rs_first(i - 1, n, m), i == n - 1 ? m : rs_first(i + 1, n, m), o0, o1);
}

// nearest: src(o) == i exactly for o in [nfirst(i), nfirst(i + 1)), nfirst(i) = max(0, ceil((2 m i - n) / (2n))) (the smallest o
// with (2o + 1) n >= 2 m i); nfirst(n) = m.  rs_nfirst_num >= 0 for i >= 0.
RS_HD int rs_nfirst_num(int i, int n, int m) { return 2 * m * i - n + 2 * n - 1; }

RS_HD int rs_nfirst(int i, int n, int m) { return rs_clamp_first(rs_nfirst_num(i, n, m) / (2 * n), m); }
