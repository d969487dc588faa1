// Implicit-GEMM NHWC convolution on the gfx950 matrix cores (fp32-in / fp32-acc MFMA 32x32x2).
//
//   forward  y[M = N*Ho*Wo][Cout]  = A[M][K = KH*KW*Cin] * W[K][Cout]      A gathered from x (im2col on the fly)
//   dgrad    dx[M = N*H*W][Cin]    = A'[M][K' = KH*KW*Cout] * Wt[K'][Cin]  A' gathered from dy, Wt = per-tap
//                                                                         transpose of W (built in workspace)
//   wgrad    dw[K][Cout]           = sum_p A[p][K]^T * dy[p][Cout]         reduction over p = N*Ho*Wo, split
//                                                                         over workgroups, fixed-order reduce
//
// One gather formula serves forward and dgrad (and therefore Conv2DTranspose forward):
//     ih = (oh * a_mul + kh * k_mul + off_h);  valid iff ih % div == 0 and 0 <= ih/div < H
//   forward: a_mul = stride, k_mul = dilation,  off = -pad_before, div = 1
//   dgrad  : a_mul = 1,      k_mul = -dilation, off = +pad_before, div = stride (1 or 2)
//
// Tiling (wave64; BM = 128 rows, BK = 32):
//   128x128 and 128x64 tiles with 8 waves (2 waves per SIMD from ONE workgroup, so one wave's gather /
//   LDS traffic overlaps its partner's MFMAs even at one workgroup per CU) or 4 waves; 128x32 with 4 waves.
//   A slab [128][32] is staged k-contiguous in LDS with a 36-float row stride (ds_read_b128 conflict-free:
//   16-B slot = 9*row mod 16), the B slab [32][BN] n-contiguous (ds_read_b32, lanes = consecutive dwords).
//   The k index inside a group of 8 is split across the two lane halves (lanes 0-31: k..k+3, lanes 32-63:
//   k+4..k+7) so one ds_read_b128 feeds four MFMAs; A and B use the same split, so the GEMM is unchanged.
//   Global -> register -> LDS staging with the loads of slab s+PF issued before the MFMAs of slab s (PF = 1 or 2
//   register sets; fp32 MFMA makes a slab only ~1.7 us of work, so two slabs in flight cover HBM/MALL latency
//   under load), LDS double-buffered, ONE barrier per slab.  All gathers are branch-free (out-of-range taps
//   read element 0 and are zeroed by a select) so a slab is a single basic block for the scheduler.
//   Block ids are remapped so each XCD owns a contiguous run of M-tiles (shared halo / weights hit one L2).
//   Tile width and the wgrad split are chosen per launch to fill whole "waves" of 2 workgroups per CU.
//
// These are the native kernels: any shape, any alignment, fp32 or bf16 storage - the fallback of every other family (conv_native.h).
#include "conv_native.h"

using namespace sgconv;

namespace {

// UT ("uniform tap"): Cin % 32 == 0 or a 1x1 kernel, so every 32-deep slab lies inside ONE filter tap.  The
// per-row source offsets and bounds flags then change only when the slab stream crosses a tap boundary (every
// Cin/32 slabs) and a slab's gather costs a handful of adds instead of ~170 VALU/SALU instructions of
// div/mod, bounds and 64-bit address arithmetic ahead of the first MFMA.
template <int BN, int WGM, int WGN, int PF, bool VEC, bool UT, typename TA = float, typename TY = TA>
__global__ __launch_bounds__(64 * WGM * WGN, WGM * WGN / 2) void igemm_conv_kernel(const IgemmParams p) {
  // TA = storage type of the activations x and y (bf16: widened to fp32 on load, rounded on store; the arithmetic is
  // the fp32 MFMA either way).  The buffer-addressed UT path exists for fp32 storage only: bf16 tensors that qualify
  // for it run on the bf16 matrix-pipe kernels instead (conv_x6.h), this kernel is their any-shape fallback.
  static_assert(!UT || std::is_same<TA, float>::value, "the UT gather is fp32-only");
  const TA* __restrict__ px = reinterpret_cast<const TA*>(p.x);
  TY* __restrict__ py = reinterpret_cast<TY*>(p.y);  // TY != TA: the fp32 softmax head of a bf16 model and its backward
  constexpr int NT = 64 * WGM * WGN;        // 4 or 8 waves; two workgroups per CU => 2 or 4 waves per SIMD
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int LDB = BN;
  constexpr int NA = (BM * BK / 4) / NT;    // float4 A chunks per thread (rows r0 + RS*j)
  constexpr int RS = NT / 8;
  constexpr int NB = (BK * BN / 4) / NT;    // float4 B chunks per thread
  static_assert(NA >= 1 && NB >= 1 && TM >= 1 && TN >= 1, "tile too small for the wave layout");
  static_assert(PF == 1 || PF == 2, "prefetch depth");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = reinterpret_cast<float*>(smem);  // [2][BM*LDA]
  float* Bs = As + 2 * BM * LDA;                // [2][BK*LDB]

  const int t = threadIdx.x;
  const uint32_t ntn = (p.Nout + BN - 1) / BN;
  // Tile order.  xcd_remap hands every XCD one contiguous range of the ordered tile ids; inside it either the
  // column tile runs fastest (the few column tiles of a row tile run together and share its A rows), or - wide
  // outputs, ntn >= 4 - tiles are walked in groups of group_m row tiles with the ROW tile fastest, so that the
  // ~64 tiles an XCD has in flight form a block that shares both operands through its L2 (ASPP dgrad: the
  // 18 MB transposed kernel is fetched once per XCD instead of once per four row tiles).
  const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  uint32_t tile_m, tile_n;
  if (p.group_m > 1) {
    const uint32_t ntm = gridDim.x / ntn, gm = (uint32_t)p.group_m;
    const uint32_t per = gm * ntn, g = bid / per, r = bid - g * per;
    const uint32_t left = ntm - g * gm, gsz = left < gm ? left : gm;
    tile_n = r / gsz;
    tile_m = g * gm + (r - tile_n * gsz);
  } else {
    tile_m = bid / ntn;
    tile_n = bid - tile_m * ntn;
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // ---- per-thread A rows: NA rows (r0 + RS j), one 4-wide k chunk (kc) ------------------------------
  const int kc = t & 7, r0 = t >> 3;
  // (oh, ow) of a row, scaled and offset, are packed as two signed 16-bit halves of one register (maps are at
  // most a few thousand pixels wide): the kernel runs at the 128-VGPR cap of 4 waves per SIMD and every live
  // register counts (a spill inside the MFMA loop costs a vmcnt(0) that drains the prefetch).
  // row_lin = n*H*W + oh'*W + ow' (the source pixel of tap (0,0) when div == 1) is needed only when the tap
  // changes: it lives in LDS (one private slot per thread and row), not in a register - and not in scratch,
  // whose reload would wait on vmcnt(0) and drain the prefetched slabs.
  int row_hw[NA];
  int* row_lin_lds = reinterpret_cast<int*>(Bs + 2 * BK * LDB) + 64;  // [NA][NT], after tapinfo[64]
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int m = m0 + r0 + RS * j;
    if (m < p.M) {
      uint32_t n, rem, oh, ow;
      fd_divmod((uint32_t)m, p.fd_ohow, n, rem);
      fd_divmod(rem, p.fd_ow, oh, ow);
      const int ohs = (int)oh * p.a_mul + p.off_h, ows = (int)ow * p.a_mul + p.off_w;
      row_lin_lds[j * NT + t] = (int)n * p.H * p.W + ohs * p.W + ows;
      row_hw[j] = (ohs << 16) | (ows & 0xffff);
    } else {
      row_lin_lds[j * NT + t] = 0;
      row_hw[j] = (int)0x80008000u;  // (-32768, -32768): out of bounds for every tap
    }
  }

  f32x4 ra[PF][NA];
  f32x4 rb[PF][NB];

  auto gather_elem_addr = [&](int j, int dh, int dw, bool kvalid, int64_t& off) -> bool {
    const int ohs = row_hw[j] >> 16, ows = (int)(short)(row_hw[j] & 0xffff);
    int ih = ohs + dh, iw = ows + dw;
    bool v = kvalid;
    const int rl = row_lin_lds[j * NT + t];
    int pix = rl + dh * p.W + dw;
    if (p.div == 2) {  // only strides 1 and 2 occur on this path (host rejects others for dgrad)
      v = v && (((ih | iw) & 1) == 0);
      ih >>= 1;
      iw >>= 1;
      pix = rl - ohs * p.W - ows + ih * p.W + iw;
    }
    v = v && ((unsigned)ih < (unsigned)p.H) && ((unsigned)iw < (unsigned)p.W);
    off = (int64_t)pix * p.x_ld;
    return v;
  };

  // ---- UT path: hardware buffer addressing ------------------------------------------------------------
  // Per row, the byte offset of the current tap's source pixel (plus this lane's 16-byte chunk) lives in a
  // VGPR for the whole tap; the slab's channel advance is the scalar soffset of the buffer load; rows whose tap
  // is out of bounds carry an offset beyond num_records, for which the hardware returns 0 (no select, no
  // branch).
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  constexpr unsigned OOB = 0x80000000u;
  int cur_tap = -1;
  unsigned tap_voff[NA];
  unsigned b_voff[NB];
#pragma unroll
  for (int j = 0; j < NA; ++j) tap_voff[j] = OOB;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int idx = t + NT * i;
    const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
    b_voff[i] = (n0 + 4 * c4) < p.Nout ? (unsigned)(kr * p.Nout + n0 + 4 * c4) * 4u : OOB;
  }
  const int ntaps = p.K / p.C;
  const bool ktail = (p.K % BK) != 0;
  __amdgpu_buffer_rsrc_t rsrc_x, rsrc_w;
  if constexpr (VEC && UT) {
    rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, (int)p.w_bytes, 0x00020000);
  }

  // loads of slab k0 into register set S (compile-time): branch-free, invalid lanes read element 0
  auto load_AB = [&](int k0, auto SET) {
    constexpr int S = decltype(SET)::value;
    if constexpr (VEC && UT) {
      const int tap = (int)fd_div((uint32_t)k0, p.fd_c);  // uniform: scalar unit
      if (tap != cur_tap) {                                // uniform branch, taken once per Cin/32 slabs
        cur_tap = tap;
        uint32_t kh, kw;
        fd_divmod((uint32_t)tap, p.fd_kw, kh, kw);
        const int dh = (int)kh * p.k_mul, dw = (int)kw * p.k_mul;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
          int64_t off;
          const bool ok = gather_elem_addr(j, dh, dw, tap < ntaps, off);
          tap_voff[j] = ok ? (unsigned)off * 4u + 16u * kc : OOB;
        }
      }
      const int soff_a = (k0 - tap * p.C) * 4;             // channel offset inside the tap, bytes (scalar)
      const int soff_b = k0 * p.Nout * 4;
      const bool kvalid = !ktail || (k0 + 4 * kc < p.K);   // only a ragged last slab (e.g. K = 728) masks lanes
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)(kvalid ? tap_voff[j] : OOB), soff_a, 0);
        ra[S][j] = __builtin_bit_cast(f32x4, v);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        // the scalar offset takes no part in the hardware range check, so a ragged last slab masks its rows
        const bool bv = !ktail || (k0 + (t + NT * i) / (BN / 4) < p.K);
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, (int)(bv ? b_voff[i] : OOB), soff_b, 0);
        rb[S][i] = __builtin_bit_cast(f32x4, v);
      }
      return;
    }
    if constexpr (VEC) {
      const int k = k0 + 4 * kc;
      const bool kvalid = k < p.K;
      uint32_t tap, ci, kh, kw;
      fd_divmod((uint32_t)k, p.fd_c, tap, ci);
      fd_divmod(tap, p.fd_kw, kh, kw);
      const int dh = (int)kh * p.k_mul, dw = (int)kw * p.k_mul;
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        int64_t off;
        const bool v = gather_elem_addr(j, dh, dw, kvalid, off);
        const f32x4 val = ld4<TA>(px + (v ? off + ci : 0));
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        ra[S][j] = v ? val : z;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 4 * kc + e;
        const bool kvalid = k < p.K;
        uint32_t tap, ci, kh, kw;
        fd_divmod((uint32_t)k, p.fd_c, tap, ci);
        fd_divmod(tap, p.fd_kw, kh, kw);
        const int dh = (int)kh * p.k_mul, dw = (int)kw * p.k_mul;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
          int64_t off;
          const bool v = gather_elem_addr(j, dh, dw, kvalid, off);
          const float val = ld1<TA>(px + (v ? off + ci : 0));
          ra[S][j][e] = v ? val : 0.f;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = t + NT * i;
      const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
      const int k = k0 + kr, n = n0 + 4 * c4;
      if constexpr (VEC) {
        const bool v = (k < p.K) && (n < p.Nout);
        const f32x4 val = *reinterpret_cast<const f32x4*>(p.w + (v ? (int64_t)k * p.Nout + n : 0));
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        rb[S][i] = v ? val : z;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool v = (k < p.K) && (n + e < p.Nout);
          const float val = p.w[v ? (int64_t)k * p.Nout + n + e : 0];
          rb[S][i][e] = v ? val : 0.f;
        }
      }
    }
  };

  auto store_AB = [&](int buf, auto SET) {
    constexpr int S = decltype(SET)::value;
    float* a = As + buf * BM * LDA;
    float* b = Bs + buf * BK * LDB;
#pragma unroll
    for (int j = 0; j < NA; ++j) *reinterpret_cast<f32x4*>(a + (r0 + RS * j) * LDA + 4 * kc) = ra[S][j];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = t + NT * i;
      const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
      *reinterpret_cast<f32x4*>(b + kr * LDB + 4 * c4) = rb[S][i];
    }
  };

  // ---- MFMA side -------------------------------------------------------------------------------------
  const int wave = t >> 6, lane = t & 63;
  const int wm = (wave / WGN) * WM, wn = (wave % WGN) * WN;
  const int lr = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // The B fragment reads are 4-byte ds_read2st64 pairs whose immediate reaches 255 * 256 bytes from the address
  // register.  Measured from LDS offset 0 the upper rows of B buffer 1 lie beyond that (A takes the first
  // 36 KB), which cost three extra address registers - spilled, and reloaded behind a vmcnt(0) in the middle of
  // the MFMA block.  So the lane's B base carries the region offset itself and is hidden from constant folding.
  int b_lane_off = 2 * BM * LDA + (4 * lh) * LDB + wn + lr;  // floats from the start of LDS (= As)
  asm volatile("" : "+v"(b_lane_off));
  const float* b_lane = As + b_lane_off;
  auto compute = [&](int buf) {
    const float* a = As + buf * BM * LDA;
    const float* b = b_lane + buf * BK * LDB;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      f32x4 af[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        af[i] = *reinterpret_cast<const f32x4*>(a + (wm + 32 * i + lr) * LDA + kk * 8 + 4 * lh);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float bf[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = b[(kk * 8 + e) * LDB + 32 * j];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j], acc[i][j], 0, 0, 0);
      }
    }
  };

  // ---- slab stream ------------------------------------------------------------------------------------
  // Dilated convolutions on small maps gather mostly zero padding (rate 18 on 32x32: only 39 % of the taps are in
  // bounds).  A tap for which ALL 128 rows of this tile fall outside the input contributes exactly nothing, so
  // its Cin/32 slabs are dropped from the stream: one block-wide vote per tap up front, then the slab index
  // runs over the surviving taps only (tapinfo[] in LDS maps it back to k0).
  int nslab = (p.K + BK - 1) / BK;
  bool use_map = false;
  int* tapinfo = reinterpret_cast<int*>(Bs + 2 * BK * LDB);
  if constexpr (VEC && UT) {
    if (p.skip_taps && ntaps > 1) {  // uniform
      int nact = 0;
      for (int tap = 0; tap < ntaps; ++tap) {
        uint32_t kh, kw;
        fd_divmod((uint32_t)tap, p.fd_kw, kh, kw);
        const int dh = (int)kh * p.k_mul, dw = (int)kw * p.k_mul;
        bool any = false;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
          int64_t off;
          any = any || gather_elem_addr(j, dh, dw, true, off);
        }
        if (__syncthreads_or(any ? 1 : 0)) {
          if (t == 0) tapinfo[nact] = tap;
          ++nact;
        }
      }
      __syncthreads();
      nslab = __builtin_amdgcn_readfirstlane(nact) * spt_of(p);
      use_map = true;
    }
  }
  // Slab iterator: the stream only ever asks for the next slab (the tail repeats the last one), so the
  // (channel block, tap, slab-in-run) counters advance incrementally on the scalar unit.  Order: for every
  // channel block of `run` slabs, for every surviving tap, the block's slabs.  run = Cin/32 gives the plain
  // tap-major order; a short run (p.cb) makes the taps of one channel block consecutive in time, so that x is
  // fetched over the fabric once and re-read by the other taps from L2.
  const int last = nslab - 1;
  bool it_lin = true;
  int it_run = 1, it_ntap = 1, it_ci = 0, it_ti = 0, it_cb = 0, it_s = 0;
  if constexpr (VEC && UT) {
    if (ntaps > 1) {  // uniform
      it_lin = false;
      it_ntap = use_map ? nslab / spt_of(p) : ntaps;
      it_run = p.cb > 0 ? p.cb : spt_of(p);
    }
  }
  auto next_k0 = [&]() -> int {
    int k0;
    if (it_lin) {
      k0 = it_s * BK;
    } else {
      const int tap = use_map ? __builtin_amdgcn_readfirstlane(tapinfo[it_ti]) : it_ti;
      k0 = tap * p.C + (it_cb * it_run + it_ci) * BK;
    }
    if (it_s < last) {
      ++it_s;
      if (!it_lin && ++it_ci == it_run) {
        it_ci = 0;
        if (++it_ti == it_ntap) { it_ti = 0; ++it_cb; }
      }
    }
    return k0;
  };
  // Stagger (MI355X_MICROARCH "two waves per SIMD", item 9): waves i and i + nwaves/2 share a SIMD and run the
  // same program between the same barriers; the upper half defers its gather (address math + global loads)
  // until after its MFMAs, so on every SIMD one wave's VALU phase overlaps its partner's matrix phase.
  const bool late = (p.stagger != 0) && (__builtin_amdgcn_readfirstlane(t >> 6) >= (NT / 128));
  if (nslab > 0) {
  if constexpr (PF == 1) {
    load_AB(next_k0(), IC<0>{});
    store_AB(0, IC<0>{});
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
      const int buf = s & 1;
      load_AB(next_k0(), IC<0>{});  // tail reloads the last slab (unused): no branch
      compute(buf);
      store_AB(buf ^ 1, IC<0>{});
      __syncthreads();
    }
  } else {
    // two register sets: while slab s is computed from LDS, slab s+1 sits in one set (landing) and slab s+2
    // is being fetched into the other; the store of a set waits only for that set's (older) loads
    load_AB(next_k0(), IC<0>{});
    load_AB(next_k0(), IC<1>{});
    store_AB(0, IC<0>{});
    __syncthreads();
    const bool do_ld = !(p.ablate & 1), do_st = !(p.ablate & 2);
    for (int s = 0; s < nslab; s += 2) {
      const int ka = next_k0();
      const int kb = next_k0();
      if (!late && do_ld) load_AB(ka, IC<0>{});
      compute(0);
      if (late && do_ld) load_AB(ka, IC<0>{});
      if (do_st) {
        store_AB(1, IC<1>{});
        __syncthreads();
      }
      if (s + 1 >= nslab) break;
      if (!late && do_ld) load_AB(kb, IC<1>{});
      compute(1);
      if (late && do_ld) load_AB(kb, IC<1>{});
      if (do_st) {
        store_AB(0, IC<0>{});
        __syncthreads();
      }
    }
  }
  }  // nslab > 0

  // ---- epilogue: bias, relu, store (each store: 2 x 128 contiguous bytes per wave) -------------------
  const bool has_bias = (p.flags & SG_EPI_BIAS) != 0;
  const bool do_relu = (p.flags & SG_EPI_RELU) != 0;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn + 32 * j + lr;
    const bool cv = col < p.Nout;
    const float bv = (has_bias && cv) ? p.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (cv && row < p.M) {
          float v = acc[i][j][r] + bv;
          if (do_relu) v = fmaxf(v, 0.f);
          st1<TY>(py + (int64_t)row * p.y_ld + col, v);
        }
      }
    }
  }
}

// ---- per-tap transpose of the kernel: w[tap][ci][co] -> wt[tap][co][ci] ------------------------------
__global__ void transpose_taps_kernel(const float* __restrict__ w, float* __restrict__ wt, int Cin, int Cout) {
  __shared__ float tile[32][33];
  const int tap = blockIdx.z;
  const float* src = w + (int64_t)tap * Cin * Cout;
  float* dst = wt + (int64_t)tap * Cin * Cout;
  const int ci0 = blockIdx.y * 32, co0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 8 rows at a time
  for (int r = ty; r < 32; r += 8) {
    const int ci = ci0 + r, co = co0 + tx;
    tile[r][tx] = (ci < Cin && co < Cout) ? src[(int64_t)ci * Cout + co] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    if (co < Cout && ci < Cin) dst[(int64_t)co * Cin + ci] = tile[tx][r];
  }
}

// ---- wgrad --------------------------------------------------------------------------------------------
// FAST: stride-1 "same" convolution (H == Ho, W == Wo) with 16-byte-aligned channel runs: the source pixel of
// output pixel p under tap (dh,dw) is p + dh*W + dw, i.e. LINEAR in p, so the gather offset advances by a constant
// per slab; only the tap's bounds flags depend on (oh, ow), which are carried incrementally (no div/mod), and
// invalid taps / rows are sent to an out-of-range buffer offset (hardware returns 0).
//
// FAST == 2 ("aligned slabs"): additionally OW % 32 == 0, so a 32-pixel slab lies in ONE image row, and the
// tile's 128 r-rows lie in ONE tap (1x1 kernel, or Cin % 128 == 0).  Then everything that changes from slab to
// slab is wave-uniform: the image row (bounds of ih), the first column ow0 and the byte offset of the slab's
// source pixels, all computed on the scalar unit and passed as the buffer load's soffset; a thread keeps only
// two CONSTANT voffsets (pixel-in-slab x channel) and tests its column against W.  No per-thread running
// state, no div/mod, ~10 fewer VGPRs: the kernel runs at the 128-VGPR cap and the state used to spill, and a
// spill reload inside the slab loop waits on vmcnt(0), i.e. drains the prefetch.
template <int BN, int WGM, int WGN, int PF, bool VEC, int FAST, typename TA = float, typename TD = TA>
__global__ __launch_bounds__(64 * WGM * WGN, WGM * WGN / 2) void igemm_wgrad_kernel(const WgradParams p) {
  static_assert(FAST == 0 || std::is_same<TA, float>::value, "the buffer-addressed wgrad paths are fp32-only");
  const TA* __restrict__ px = reinterpret_cast<const TA*>(p.x);
  const TD* __restrict__ pdy = reinterpret_cast<const TD*>(p.dy);  // TD != TA: fp32 dy of the softmax head of a bf16 model
  constexpr int NT = 64 * WGM * WGN;
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int LDAW = BM;  // A' slab is [32 pixels][128 r], r contiguous
  constexpr int LDB = BN;
  constexpr int NA = (BK * BM / 4) / NT;   // float4 A' chunks per thread (pixel rows pr0 + PS*j)
  constexpr int PS = NT / 32;
  constexpr int NB = (BK * BN / 4) / NT;
  static_assert(NA >= 1 && NB >= 1 && TM >= 1 && TN >= 1, "tile too small for the wave layout");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = reinterpret_cast<float*>(smem);  // [2][BK*LDAW]
  float* Bs = As + 2 * BK * LDAW;               // [2][BK*LDB]

  const int t = threadIdx.x;
  const uint32_t ntn = (p.Cout + BN - 1) / BN;
  // Workgroup order.  The hardware deals workgroups round-robin to the XCDs in linear (z, x) order; the remap
  // gives each XCD one contiguous range of (split, tile) pairs, i.e. mostly ONE pixel split, whose dy stays in
  // that XCD's L2 for the whole range.  Inside a split, with tap_inner the tiles of one 128-channel block come
  // together: all taps x all column tiles read the same x columns (shifted by the tap) and share them through
  // L2, and every XCD gets the same mix of cheap and expensive taps when padding slabs are skipped.
  uint32_t bid, split;
  {
    const uint32_t lin = blockIdx.z * gridDim.x + blockIdx.x;
    const uint32_t o = xcd_remap(lin, gridDim.x * gridDim.z);
    split = o / gridDim.x;
    bid = o - split * gridDim.x;
  }
  uint32_t tile_r, tile_n;
  if (p.tap_inner) {
    const uint32_t per = (uint32_t)p.KH_KW * ntn, ncib = (uint32_t)p.Cin / BM;
    const uint32_t cib = bid / per, rem = bid - cib * per, tap = rem / ntn;
    tile_n = rem - tap * ntn;
    tile_r = tap * ncib + cib;
  } else {
    tile_r = bid / ntn;
    tile_n = bid - tile_r * ntn;
  }
  const int rbase = tile_r * BM, n0 = tile_n * BN;

  // A' chunk owned by this thread: r = rbase + 4*rc (fixed tap / channel), pixel rows (t>>5) + PS j
  const int rc = t & 31, pr0 = t >> 5;
  constexpr int NV = VEC ? 1 : 4;
  int dh[NV], dw[NV], ci_e[NV];
  bool rvalid[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    const int r = rbase + 4 * rc + e;
    rvalid[e] = r < p.K;
    uint32_t tap, ci, kh, kw;
    fd_divmod((uint32_t)r, p.fd_c, tap, ci);
    fd_divmod(tap, p.fd_kw, kh, kw);
    dh[e] = (int)kh * p.dil - p.pad_t;
    dw[e] = (int)kw * p.dil - p.pad_l;
    ci_e[e] = (int)ci;
  }

  const int slab_begin = (int)split * p.slabs_per_split;
  const int nslab_total = (p.P + BK - 1) / BK;
  int slab_end = slab_begin + p.slabs_per_split;
  if (slab_end > nslab_total) slab_end = nslab_total;

  f32x4 ra[PF][NA];
  f32x4 rb[PF][NB];

  // ---- FAST path state --------------------------------------------------------------------------------
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  constexpr unsigned OOB = 0x80000000u;
  int f_oh[NA], f_ow[NA], f_p[NA];   // (oh, ow) and pixel index of this thread's rows in the NEXT slab to load
  unsigned f_voff[NA];               // byte offset of x[p + dh*W + dw][ci] for that slab
  unsigned b_voff[NB];
  int f_next = slab_begin * BK;      // pixel index the running state corresponds to
  __amdgpu_buffer_rsrc_t rsrc_x, rsrc_dy;
  const int adv_oh = BK / p.OW, adv_ow = BK % p.OW;
  // FAST == 2 state: constant voffsets; the descriptor's base sits SH pixels BEFORE x so that the scalar offset
  // (p0 + dh*W + dw + SH) * x_ld * 4 is non-negative whenever a lane of the slab is in bounds
  constexpr int SH = 32;
  unsigned a_voffc[NA];
  int s_dh = 0, s_dw = 0;
  if constexpr (FAST == 2) {
    // num_records spans the whole (shifted) tensor: whether or not the hardware adds soffset into its range
    // check, in-bounds lanes pass and the OOB voffset fails
    rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x) - (int64_t)SH * p.x_ld, 0,
                                               (int)(p.x_bytes + (uint32_t)(SH * p.x_ld * 4)), 0x00020000);
    rsrc_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dy), 0, (int)p.dy_bytes, 0x00020000);
    {
      const int tap = rbase / p.Cin;  // uniform: the whole tile lies in this tap
      uint32_t kh, kw;
      fd_divmod((uint32_t)tap, p.fd_kw, kh, kw);
      s_dh = (int)kh * p.dil - p.pad_t;
      s_dw = (int)kw * p.dil - p.pad_l;
    }
#pragma unroll
    for (int j = 0; j < NA; ++j)
      a_voffc[j] = rvalid[0] ? (unsigned)((pr0 + PS * j) * p.x_ld + ci_e[0]) * 4u : OOB;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = t + NT * i;
      const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
      b_voff[i] = (n0 + 4 * c4) < p.Cout ? (unsigned)(kr * p.y_ld + n0 + 4 * c4) * 4u : OOB;
    }
  }
  if constexpr (FAST == 1) {
    rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    rsrc_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dy), 0, (int)p.dy_bytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int pp = f_next + pr0 + PS * j;
      uint32_t n, rem, oh, ow;
      fd_divmod((uint32_t)pp, p.fd_ohow, n, rem);
      fd_divmod(rem, p.fd_ow, oh, ow);
      f_oh[j] = (int)oh; f_ow[j] = (int)ow; f_p[j] = pp;
      f_voff[j] = (unsigned)((pp + dh[0] * p.W + dw[0]) * p.x_ld + ci_e[0]) * 4u;  // may wrap when the tap is invalid
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = t + NT * i;
      const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
      b_voff[i] = (n0 + 4 * c4) < p.Cout ? (unsigned)(kr * p.y_ld + n0 + 4 * c4) * 4u : OOB;
    }
  }

  auto load_AB = [&](int p0, auto SET) {
    constexpr int S = decltype(SET)::value;
    if constexpr (FAST == 2) {
      uint32_t q, ow0, n_, oh;
      fd_divmod((uint32_t)p0, p.fd_ow, q, ow0);   // all scalar: p0 is wave-uniform
      fd_divmod(q, p.fd_oh, n_, oh);
      const int ih = (int)oh + s_dh;
      const bool row_ok = (unsigned)ih < (unsigned)p.H;
      const int soff_a = row_ok ? (p0 + s_dh * p.W + s_dw + SH) * p.x_ld * 4 : 0;
      const int col0 = (int)ow0 + s_dw + pr0;
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        const bool v = row_ok && ((unsigned)(col0 + PS * j) < (unsigned)p.W);
        const u32x4 val = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)(v ? a_voffc[j] : OOB), soff_a, 0);
        ra[S][j] = __builtin_bit_cast(f32x4, val);
      }
      const int soff_b = p0 * p.y_ld * 4;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const u32x4 val = __builtin_amdgcn_raw_buffer_load_b128(rsrc_dy, (int)b_voff[i], soff_b, 0);  // P % 32 == 0
        rb[S][i] = __builtin_bit_cast(f32x4, val);
      }
      return;
    }
    if constexpr (FAST == 1) {
      // the slab stream is sequential except for the repeated (unused) tail slab: advance only when it moves on
      if (p.skip_slabs) {  // uniform: slabs are visited with gaps, so derive the state from p0 directly
        if (p0 != f_next) {
          f_next = p0;
#pragma unroll
          for (int j = 0; j < NA; ++j) {
            const int pp = p0 + pr0 + PS * j;
            uint32_t n, rem, oh, ow;
            fd_divmod((uint32_t)pp, p.fd_ohow, n, rem);
            fd_divmod(rem, p.fd_ow, oh, ow);
            f_oh[j] = (int)oh; f_ow[j] = (int)ow; f_p[j] = pp;
            f_voff[j] = (unsigned)((pp + dh[0] * p.W + dw[0]) * p.x_ld + ci_e[0]) * 4u;
          }
        }
      } else if (p0 != f_next) {  // uniform
        f_next = p0;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
          f_p[j] += BK;
          f_voff[j] += (unsigned)(BK * p.x_ld) * 4u;
          f_ow[j] += adv_ow;
          f_oh[j] += adv_oh;
          if (f_ow[j] >= p.OW) { f_ow[j] -= p.OW; f_oh[j] += 1; }
          while (f_oh[j] >= p.OH) f_oh[j] -= p.OH;
        }
      }
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        const int ih = f_oh[j] + dh[0], iw = f_ow[j] + dw[0];
        const bool v = rvalid[0] && (f_p[j] < p.P) && ((unsigned)ih < (unsigned)p.H) && ((unsigned)iw < (unsigned)p.W);
        const u32x4 val = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, (int)(v ? f_voff[j] : OOB), 0, 0);
        ra[S][j] = __builtin_bit_cast(f32x4, val);
      }
      const int soff_b = p0 * p.y_ld * 4;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const bool bv = (p0 + (t + NT * i) / (BN / 4)) < p.P;  // soffset is not range-checked
        const u32x4 val = __builtin_amdgcn_raw_buffer_load_b128(rsrc_dy, (int)(bv ? b_voff[i] : OOB), soff_b, 0);
        rb[S][i] = __builtin_bit_cast(f32x4, val);
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int pp = p0 + pr0 + PS * j;
      const bool pv = pp < p.P;
      uint32_t n, rem, oh, ow;
      fd_divmod((uint32_t)(pv ? pp : 0), p.fd_ohow, n, rem);
      fd_divmod(rem, p.fd_ow, oh, ow);
      const int pixbase = n * p.H * p.W;
      if constexpr (VEC) {
        const int ih = (int)oh * p.stride + dh[0], iw = (int)ow * p.stride + dw[0];
        const bool v = pv && rvalid[0] && ((unsigned)ih < (unsigned)p.H) && ((unsigned)iw < (unsigned)p.W);
        const f32x4 val = ld4<TA>(px + (v ? (int64_t)(pixbase + ih * p.W + iw) * p.x_ld + ci_e[0] : 0));
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        ra[S][j] = v ? val : z;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ih = (int)oh * p.stride + dh[e], iw = (int)ow * p.stride + dw[e];
          const bool v = pv && rvalid[e] && ((unsigned)ih < (unsigned)p.H) && ((unsigned)iw < (unsigned)p.W);
          const float val = ld1<TA>(px + (v ? (int64_t)(pixbase + ih * p.W + iw) * p.x_ld + ci_e[e] : 0));
          ra[S][j][e] = v ? val : 0.f;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = t + NT * i;
      const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
      const int pp = p0 + kr, n = n0 + 4 * c4;
      if constexpr (VEC) {
        const bool v = (pp < p.P) && (n < p.Cout);
        const f32x4 val = ld4<TD>(pdy + (v ? (int64_t)pp * p.y_ld + n : 0));
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        rb[S][i] = v ? val : z;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool v = (pp < p.P) && (n + e < p.Cout);
          const float val = ld1<TD>(pdy + (v ? (int64_t)pp * p.y_ld + n + e : 0));
          rb[S][i][e] = v ? val : 0.f;
        }
      }
    }
  };

  auto store_AB = [&](int buf, auto SET) {
    constexpr int S = decltype(SET)::value;
    float* a = As + buf * BK * LDAW;
    float* b = Bs + buf * BK * LDB;
#pragma unroll
    for (int j = 0; j < NA; ++j) *reinterpret_cast<f32x4*>(a + (pr0 + PS * j) * LDAW + 4 * rc) = ra[S][j];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = t + NT * i;
      const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
      *reinterpret_cast<f32x4*>(b + kr * LDB + 4 * c4) = rb[S][i];
    }
  };

  const int wave = t >> 6, lane = t & 63;
  const int wm = (wave / WGN) * WM, wn = (wave % WGN) * WN;
  const int lr = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto compute = [&](int buf) {
    const float* a = As + buf * BK * LDAW;
    const float* b = Bs + buf * BK * LDB;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int pk = 2 * kk + lh;
      float af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = a[pk * LDAW + wm + 32 * i + lr];
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = b[pk * LDB + wn + 32 * j + lr];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };

  // ---- slab stream: with dilation, whole 32-pixel slabs can be padding for every tap this tile covers
  // (rate 18 on a 32x32 map: 18 of 32 image rows per vertical tap); those are dropped.  Each thread classifies
  // slabs in parallel, thread 0 compacts the survivors into an LDS list that the stream then walks.
  int nslab = slab_end - slab_begin;  // >= 1 by construction of the split plan
  int* slist = reinterpret_cast<int*>(Bs + 2 * BK * LDB);  // [1 + 1024]
  bool use_list = false;
  if constexpr (FAST) {
    if (p.skip_slabs && nslab <= 1024) {  // uniform
      use_list = true;
      const int tap_lo = rbase / p.Cin;
      int tap_hi = (rbase + BM - 1 < p.K ? rbase + BM - 1 : p.K - 1) / p.Cin;
      if (tap_hi >= p.KH_KW) tap_hi = p.KH_KW - 1;
      int* flags = slist + 1 + 1024;  // [1024]
      for (int i = t; i < nslab; i += NT) {
        const int pa = (slab_begin + i) * BK;
        int pb = pa + BK - 1;
        if (pb > p.P - 1) pb = p.P - 1;
        uint32_t na, ra_, nb, rb_, oha, ohb, tmp;
        fd_divmod((uint32_t)pa, p.fd_ohow, na, ra_);
        fd_divmod((uint32_t)pb, p.fd_ohow, nb, rb_);
        fd_divmod(ra_, p.fd_ow, oha, tmp);
        fd_divmod(rb_, p.fd_ow, ohb, tmp);
        bool act = na != nb;
        for (int tap = tap_lo; tap <= tap_hi && !act; ++tap) {
          uint32_t kh, kw;
          fd_divmod((uint32_t)tap, p.fd_kw, kh, kw);
          const int ddh = (int)kh * p.dil - p.pad_t, ddw = (int)kw * p.dil - p.pad_l;
          act = ((int)ohb + ddh >= 0) && ((int)oha + ddh < p.H) && (ddw > -p.W) && (ddw < p.W);
        }
        flags[i] = act ? 1 : 0;
      }
      __syncthreads();
      if (t == 0) {
        int n = 0;
        for (int i = 0; i < nslab; ++i)
          if (flags[i]) slist[1 + n++] = slab_begin + i;
        slist[0] = n;
      }
      __syncthreads();
      nslab = slist[0];
    }
  }
  auto slab_of = [&](int i) -> int { return use_list ? slist[1 + i] : slab_begin + i; };
  const int lasti = nslab - 1;
  if (nslab > 0) {
    if constexpr (PF == 1) {
      load_AB(slab_of(0) * BK, IC<0>{});
      store_AB(0, IC<0>{});
      __syncthreads();
      for (int s = 0; s < nslab; ++s) {
        const int buf = s & 1;
        load_AB(slab_of(s < lasti ? s + 1 : lasti) * BK, IC<0>{});
        compute(buf);
        store_AB(buf ^ 1, IC<0>{});
        __syncthreads();
      }
    } else {
      load_AB(slab_of(0) * BK, IC<0>{});
      load_AB(slab_of(1 < lasti ? 1 : lasti) * BK, IC<1>{});
      store_AB(0, IC<0>{});
      __syncthreads();
      const bool late = (p.stagger != 0) && (__builtin_amdgcn_readfirstlane(t >> 6) >= (NT / 128));
      for (int s = 0; s < nslab; s += 2) {
        const int pa = slab_of(s + 2 < lasti ? s + 2 : lasti) * BK, pb = slab_of(s + 3 < lasti ? s + 3 : lasti) * BK;
        if (!late) load_AB(pa, IC<0>{});
        compute(0);
        if (late) load_AB(pa, IC<0>{});
        store_AB(1, IC<1>{});
        __syncthreads();
        if (s + 1 >= nslab) break;
        if (!late) load_AB(pb, IC<1>{});
        compute(1);
        if (late) load_AB(pb, IC<1>{});
        store_AB(0, IC<0>{});
        __syncthreads();
      }
    }
  }

  float* out = p.out + (int64_t)split * p.K * p.Cout;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn + 32 * j + lr;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rbase + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (col < p.Cout && row < p.K) out[(int64_t)row * p.Cout + col] = acc[i][j][r];
      }
    }
  }
}

// out[i] = sum_z part[z][i]  in fixed z order (V = 4: 16-byte accesses, n % 4 == 0 and aligned pointers; the z loop is
// unrolled so that the partial rows' loads are in flight together - the adds stay in z order)
template <int V>
__global__ __launch_bounds__(256) void reduce_splits_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t n, int S) {
  int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * V;
  for (; i < n; i += stride) {
    float s[V];
    ldv<V>(part + i, s);
#pragma unroll 8
    for (int z = 1; z < S; ++z) {
      float v[V];
      ldv<V>(part + (int64_t)z * n + i, v);
#pragma unroll
      for (int k = 0; k < V; ++k) s[k] += v[k];
    }
    stv<V>(out + i, s);
  }
}

template <int BN, int WGM, int WGN, int PF, bool VEC, bool UT, typename TA = float, typename TY = TA>
int launch_igemm_ut(const IgemmParams& p, hipStream_t st) {
  // + tapinfo[64] + row_lin[NA][NT] (NA * NT = BM * BK / 4 ints)
  constexpr size_t lds = (size_t)(2 * BM * LDA + 2 * BK * BN) * sizeof(float) + 256 + (size_t)(BM * BK / 4) * sizeof(int);
  static bool attr_done = false;  // idempotent; racing threads set the same value
  if (!attr_done) {
    int rc = set_dyn_lds(igemm_conv_kernel<BN, WGM, WGN, PF, VEC, UT, TA, TY>, lds);
    if (rc) return rc;
    attr_done = true;
  }
  const int64_t tiles = sg_cdiv(p.M, BM) * sg_cdiv(p.Nout, BN);
  if (tiles <= 0 || tiles > 0x7fffffff) {
    sg_set_error("igemm: bad tile count %lld", (long long)tiles);
    return SG_EINVAL;
  }
  hipLaunchKernelGGL((igemm_conv_kernel<BN, WGM, WGN, PF, VEC, UT, TA, TY>), dim3((unsigned)tiles), dim3(64 * WGM * WGN), lds, st, p);
  SG_LAUNCH_CHECK("igemm_conv_kernel");
  return 0;
}

template <int BN, int WGM, int WGN, int PF, bool VEC>
int launch_igemm(const IgemmParams& p, hipStream_t st) {
  if constexpr (VEC) {
    const bool ut = igemm_ut_of(p);
    if (ut) return launch_igemm_ut<BN, WGM, WGN, PF, true, true>(p, st);
  }
  return launch_igemm_ut<BN, WGM, WGN, PF, VEC, false>(p, st);
}

int dispatch_igemm_f32(const IgemmParams& p_in, bool vec, int num_cus, hipStream_t st) {
  IgemmParams p = p_in;
  const int bn = native_common(p, vec, num_cus);
  // the structure that won every A/B: 8-wave workgroups, two-slab prefetch, staggered wave halves (the 4-wave and one-slab
  // forms are gone: DESIGN.md, retired)
  p.stagger = 1;
  p.ablate = sg_switch<SW_CONV_ABLATE>() & 3;
  if (!vec) {
    if (bn == 128) return launch_igemm<128, 2, 4, 1, false>(p, st);
    if (bn == 64) return launch_igemm<64, 4, 2, 1, false>(p, st);
    return launch_igemm<32, 4, 1, 1, false>(p, st);
  }
  if (bn == 128) return launch_igemm<128, 2, 4, 2, true>(p, st);
  if (bn == 64) return launch_igemm<64, 4, 2, 2, true>(p, st);
  return launch_igemm<32, 4, 1, 2, true>(p, st);
}

template <int BN, int WGM, int WGN, int PF, bool VEC, int FAST, typename TA = float, typename TD = TA>
int launch_wgrad_f(const WgradParams& p, int S, hipStream_t st) {
  constexpr size_t lds = (size_t)(2 * BK * BM + 2 * BK * BN) * sizeof(float) + (FAST ? (2 * 1024 + 4) * sizeof(int) : 0);
  static bool attr_done = false;
  if (!attr_done) {
    int rc = set_dyn_lds(igemm_wgrad_kernel<BN, WGM, WGN, PF, VEC, FAST, TA, TD>, lds);
    if (rc) return rc;
    attr_done = true;
  }
  const int64_t tiles = sg_cdiv(p.K, BM) * sg_cdiv(p.Cout, BN);
  hipLaunchKernelGGL((igemm_wgrad_kernel<BN, WGM, WGN, PF, VEC, FAST, TA, TD>), dim3((unsigned)tiles, 1, (unsigned)S), dim3(64 * WGM * WGN), lds, st, p);
  SG_LAUNCH_CHECK("igemm_wgrad_kernel");
  return 0;
}

// any-shape fallback for bf16 storage: the native fp32-MFMA kernel with widening loads (TA) and a rounding store (TY).
// <bf16, bf16> is the plain fallback; <bf16, float> the forward of a softmax head that is not a thin 1x1 convolution
// (Res34-UNet: Conv2D(2, 3, activation='softmax'), res34.py:156), <float, bf16> its dgrad (fp32 dy in, bf16 dx out).
template <typename TA, typename TY>
int dispatch_igemm_mixed_t(const IgemmParams& p_in, bool vec, int num_cus, hipStream_t st) {
  IgemmParams p = p_in;
  const int bn = mixed_common(p, num_cus);
  if (vec) {
    if (bn == 128) return launch_igemm_ut<128, 2, 4, 1, true, false, TA, TY>(p, st);
    if (bn == 64) return launch_igemm_ut<64, 4, 2, 1, true, false, TA, TY>(p, st);
    return launch_igemm_ut<32, 4, 1, 1, true, false, TA, TY>(p, st);
  }
  if (bn == 128) return launch_igemm_ut<128, 2, 4, 1, false, false, TA, TY>(p, st);
  if (bn == 64) return launch_igemm_ut<64, 4, 2, 1, false, false, TA, TY>(p, st);
  return launch_igemm_ut<32, 4, 1, 1, false, false, TA, TY>(p, st);
}

// the template instantiation the plan names, for the three tile widths
#define WG_TILE(FN, ...)                                                         \
  (bn == 128 ? FN<128, 2, 4, __VA_ARGS__>(p, S, st)                             \
             : bn == 64 ? FN<64, 4, 2, __VA_ARGS__>(p, S, st) : FN<32, 4, 1, __VA_ARGS__>(p, S, st))

}  // namespace

namespace sgconv {

int dispatch_igemm(const IgemmParams& p, bool x_b16, bool y_b16, bool vec, int num_cus, hipStream_t st) {
  if (!x_b16 && !y_b16) return dispatch_igemm_f32(p, vec, num_cus, st);
  if (x_b16 && y_b16) return dispatch_igemm_mixed_t<bf16_t, bf16_t>(p, vec, num_cus, st);
  if (x_b16) return dispatch_igemm_mixed_t<bf16_t, float>(p, vec, num_cus, st);
  return dispatch_igemm_mixed_t<float, bf16_t>(p, vec, num_cus, st);
}

int launch_transpose_taps(const float* w, float* wt, int Cin, int Cout, int taps, hipStream_t st) {
  dim3 grid((unsigned)sg_cdiv(Cout, 32), (unsigned)sg_cdiv(Cin, 32), (unsigned)taps);
  hipLaunchKernelGGL(transpose_taps_kernel, grid, dim3(256), 0, st, w, wt, Cin, Cout);
  SG_LAUNCH_CHECK("transpose_taps_kernel");
  return 0;
}

int launch_wgrad_native(const WgradParams& p, int bn, int S, bool x_b16, bool dy_b16, bool vec, int fast, hipStream_t st) {
  if (x_b16 && !dy_b16) return vec ? WG_TILE(launch_wgrad_f, 1, true, 0, bf16_t, float) : WG_TILE(launch_wgrad_f, 1, false, 0, bf16_t, float);
  if (x_b16) return vec ? WG_TILE(launch_wgrad_f, 1, true, 0, bf16_t) : WG_TILE(launch_wgrad_f, 1, false, 0, bf16_t);
  if (!vec) return WG_TILE(launch_wgrad_f, 1, false, 0);
  if (fast == 2) return WG_TILE(launch_wgrad_f, 2, true, 2);
  return fast == 1 ? WG_TILE(launch_wgrad_f, 2, true, 1) : WG_TILE(launch_wgrad_f, 2, true, 0);
}
#undef WG_TILE

int launch_reduce_splits(const float* part, float* out, int64_t n, int S, bool v4, hipStream_t st) {
  int64_t blocks = sg_cdiv(n, v4 ? 1024 : 256);
  if (blocks > 2048) blocks = 2048;
  // (a four-lanes-per-quad kernel measured no gain - the reduce launches sit on the side stream behind their filter gradient
  // and hide either way - and is gone: DESIGN.md, retired)
  if (v4) hipLaunchKernelGGL(reduce_splits_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, part, out, n, S);
  else hipLaunchKernelGGL(reduce_splits_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, part, out, n, S);
  SG_LAUNCH_CHECK("reduce_splits_kernel");
  return 0;
}

}  // namespace sgconv
