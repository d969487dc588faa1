// The convolutions' plans (plan_conv, plan_wgrad), parameter filling and entry points, and - still included below, inside this file's
// anonymous namespace - the kernels of the x6, bf16, planes-in x6 and wide pointwise families.  The shared types live in conv_common.h
// (namespace sgconv).  Units of their own, reached through plain host functions: the native kernels with the description of the
// implicit GEMM (conv_native.hip), the thin 1x1 kernels with the segmented reductions (conv_thin.hip), the patch family (conv_x6p.hip).
#include "conv_common.h"
#include "conv_native.h"
#include "conv_thin.h"
#include "conv_x6p.h"
#include "conv_x6wp.h"

using namespace sgconv;

namespace {

// Convolution arithmetic on fp32 storage (conv_x6.h: x6_mode()), the one piece of state that can be set at run time
// (sg_set_conv_x6): -1 = not yet read from the environment
int g_x6_mode = -1;

#include "conv_x6.h"
#include "conv_b16.h"
#include "conv_pw.h"
#include "conv_b16w.h"
#include "conv_x6w.h"

// conv_x6_kernel's structure for a launch of `tiles` tiles (1: double-buffered, one workgroup per CU; 0: single-buffered, two per
// CU; the measurements: in dispatch_x6) and its product shape (16x16x32 for the multi-tap convolutions of the six-pass arithmetic).
// dispatch_x6 and the plan query (sg_conv2d_plan) both ask here.
inline int x6_var_of(int64_t tiles, int num_cus) {
  const int var = x6_variant();
  return var < 0 ? ((tiles <= 3 * (int64_t)num_cus) ? 1 : 0) : var;
}
inline bool x6_mf16_of(const IgemmParams& p) { return sg_switch<SW_X6_MF16>() && p.K != p.C; }

template <int NPL, typename TA>
int dispatch_x6(const IgemmParams& p_in, int num_cus, hipStream_t st) {
  IgemmParams p = p_in;
  const int bn = slab_common(p, SLAB_X6, EL<TA>::BYTES, num_cus);
  p.stagger = sg_switch<SW_X6_INTERLEAVE>() ? 2 : 0;  // 0: staggered halves instead of the hand-interleaved step (A/B switch)
  p.ablate = sg_switch<SW_X6_ABLATE>() & 15;
  // Structure by tile count (measured, profiles/r01_ab_x6.txt, r01_ab_x6_interleave.txt, r01_ab_tiles1024.txt): up to
  // 3 tiles per CU the double-buffered one-workgroup-per-CU form with the hand-interleaved step wins (ASPP forward
  // 1.02 -> 0.89 ms, pointwise 728 forward 0.150 -> 0.137 ms); from 4 tiles per CU - i.e. two full rounds of the
  // two-workgroups-per-CU single-buffer form - that one does (1024 tiles: 64x64 512->256 forward 887 vs 930 us,
  // 1024->1024 pointwise 233 vs 252 us; ASPP dgrad 0.83 vs 0.94 ms, decoder 128->64 dgrad 0.92 vs 1.03 ms).
  // SG_X6_VARIANT overrides.  (4-wave workgroups, 64x64 per wave, lost to both 8-wave structures and are gone: DESIGN.md, retired.)
  const int64_t tiles = sg_cdiv(p.M, BM) * sg_cdiv(p.Nout, bn);
  const int var = x6_var_of(tiles, num_cus);
  if constexpr (NPL == 1) {  // the one-plane (bf16 product) kernels come in the two 8-wave structures only
    if (bn == 128) return (var & 1) ? launch_x6<128, 2, 4, 2, 1, TA>(p, st) : launch_x6<128, 2, 4, 1, 1, TA>(p, st);
    if (bn == 64) return (var & 1) ? launch_x6<64, 4, 2, 2, 1, TA>(p, st) : launch_x6<64, 4, 2, 1, 1, TA>(p, st);
    return (var & 1) ? launch_x6<32, 4, 1, 2, 1, TA>(p, st) : launch_x6<32, 4, 1, 1, 1, TA>(p, st);
  } else {
  // 16x16x32 products for the multi-tap convolutions (conv_x6_kernel, MF): a property of the layer, never of the batch.
  // SG_X6_MF16=0 keeps every launch on 32x32x16 (A/B runs).
  const bool mf = x6_mf16_of(p);
  if (bn == 128) {
    if (mf) return var ? launch_x6<128, 2, 4, 2, 3, float, 1>(p, st) : launch_x6<128, 2, 4, 1, 3, float, 1>(p, st);
    return var ? launch_x6<128, 2, 4, 2>(p, st) : launch_x6<128, 2, 4, 1>(p, st);
  }
  if (bn == 64) {
    if (mf) return var ? launch_x6<64, 4, 2, 2, 3, float, 1>(p, st) : launch_x6<64, 4, 2, 1, 3, float, 1>(p, st);
    return var ? launch_x6<64, 4, 2, 2>(p, st) : launch_x6<64, 4, 2, 1>(p, st);
  }
  if (mf) return var ? launch_x6<32, 4, 1, 2, 3, float, 1>(p, st) : launch_x6<32, 4, 1, 1, 3, float, 1>(p, st);
  return var ? launch_x6<32, 4, 1, 2>(p, st) : launch_x6<32, 4, 1, 1>(p, st);
  }
}

// ---- who chooses the kernel --------------------------------------------------------------------------------------------
// plan_conv() decides which kernel family a forward convolution or an input gradient takes and how its weight planes and the
// scratch behind them are laid out - from the descriptor, the storage type, the arithmetic mode and the experiment switches, and
// from nothing else: no pointers, no `res`.  The workspace queries, sg_conv2d_caps, sg_conv2d_planes_job and the launch
// all read this one plan (the filter gradient's counterpart is plan_wgrad), so they cannot disagree.  What the descriptor does
// not say - the alignment of the operands, the workspace a launch was handed - is checked once, at the launch, against the plan.
// Run a launch of the plan's family (>= CONV_SLAB) on its weight planes in `ws`; the scratch of a wide slab form lies behind them.
// prepared: `ws` already holds the planes (sg_prepare_planes, once per optimiser step), no split here.
// NPL = 3: the exact fp32 emulation; NPL = 1: bf16 products (TA = float: fp32 storage rounded on the way into LDS,
// TA = bf16_t: SG_BF16 storage).
template <int NPL, typename TA>
int run_x6(const ConvPlan& pl, IgemmParams& p, const float* w, bool dgrad, int Cin, int Cout, void* ws, int num_cus, hipStream_t st,
           bool prepared) {
  constexpr bool B16 = !std::is_same<TA, float>::value;
  const int N = p.Nout;
  switch (pl.family) {
    case CONV_PATCH:
      if constexpr (NPL == 3) return run_x6p(p, w, dgrad, Cin, Cout, ws, num_cus, st, prepared);
      break;
    case CONV_WIDE:
      // 1x1 / stride 1 with enough columns for 384- or 256-wide tiles (the 728-wide middle flow and the exit flow)
      if constexpr ((NPL == 3 && !B16) || (NPL == 1 && B16)) {
        p.Kpad = pl.Kpad;
        p.Npad = pl.Npad;
        p.wq = (const unsigned short*)ws;
        p.w_bytes = (uint32_t)pl.w_bytes;
        if (!prepared) {
          dim3 grid((unsigned)sg_cdiv(p.Kpad, 32), (unsigned)sg_cdiv(p.Npad, 32));
          hipLaunchKernelGGL(split3_weights_kernel, grid, dim3(256), 0, st, w, (unsigned short*)ws, pl.K, N, p.Kpad, p.Npad, pl.K,
                             Cin * Cout, dgrad ? 1 : Cout, dgrad ? Cout : 1, NPL, pl.K, pl.kd);
          SG_LAUNCH_CHECK("split3_weights_kernel");
        }
        if constexpr (NPL == 3) {
          if (p.bnb.x)   // the BatchNormalization backward in the A path (sg_conv_opts.bnb)
            return pl.wbn == 256 ? launch_pw_wide<NPL, TA, 256, true>(p, st) : launch_pw_wide<NPL, TA, 384, true>(p, st);
        }
        return pl.wbn == 256 ? launch_pw_wide<NPL, TA, 256>(p, st) : launch_pw_wide<NPL, TA, 384>(p, st);
      }
      break;
    case CONV_SLAB: {
      const int Ck = p.C;
      slab_fill(p, pl);
      p.wq = (const unsigned short*)ws;
      if (!prepared) {
        dim3 grid((unsigned)(p.Kpad / 32), (unsigned)(p.Npad / 32));
        hipLaunchKernelGGL(split3_weights_kernel, grid, dim3(256), 0, st, w, (unsigned short*)ws, pl.K, N, p.Kpad, p.Npad, Ck,
                           Cin * Cout, dgrad ? 1 : Cout, dgrad ? Cout : 1, NPL, pl.Ckp, p.kd);
        SG_LAUNCH_CHECK("split3_weights_kernel");
      }
      char* scratch = (char*)ws + ((pl.w_bytes + 255) & ~(size_t)255);
      const SlabKernel sk = slab_kernel_of(pl, B16, p.res != nullptr);
      if constexpr (NPL == 3 && !B16) {
        if (sk == SLAB_X6W) {   // scratch: the planes of A, then split-K partial slabs
          IgemmParams q = p;
          slab_common(q, sk, 4, num_cus);
          q.ablate = sg_switch<SW_X6W_ABLATE>();
          return launch_x6w(q, pl.x6w_S, scratch, st);
        }
      }
      if constexpr (NPL == 1 && B16) {
        if (sk == SLAB_B16W) {
          IgemmParams q = p;
          slab_common(q, sk, 2, num_cus);
          return launch_b16w(q, pl.b16w_S, pl.b16w_S > 1 ? reinterpret_cast<float*>(scratch) : nullptr, st);
        }
        if (sk == SLAB_B16) return dispatch_b16(p, num_cus, st);
      }
      if (sk != SLAB_X6) break;   // (a plan of another arithmetic than this instantiation's)
      return dispatch_x6<NPL, TA>(p, num_cus, st);
    }
    default:
      break;
  }
  sg_set_error("run_x6: kernel family %d does not read weight planes in this arithmetic (%d planes)", (int)pl.family, NPL);
  return SG_EINVAL;
}

// workspace of the weight planes for a launch with `taps` taps of depth C (virtual padding included), N columns
inline size_t x6_ws_bytes(int taps, int C, int N) {
  const int k = taps > 1 ? taps * x6_vpad_c(C) : C;
  const size_t rows = x6_planes_bytes(k, N, 3, 64);   // (the deepest k-block any kernel asks for)
  // the wide pointwise kernel pads N to its tile width, 384 or 256.  The second term still pads to 512, the width of a tile form
  // that is gone: it decides the value for e.g. 728 columns, and callers' workspaces keep the size they had
  const size_t w384 = taps == 1 ? pw_planes_bytes(C, N, 3, 384) : 0, w512 = taps == 1 ? pw_planes_bytes(C, N, 3, 512) : 0;
  const size_t wide = w384 > w512 ? w384 : w512;
  return rows > wide ? rows : wide;
}

// images per sub-batch such that both activation tensors stay under 2 GiB (>= N: no split needed); ebx / eby = bytes per element of x / y
inline int64_t images_limit_bytes() {
  // test hook: SG_CONV_MAX_BYTES lowers the 2 GiB limit so that small tensors exercise the sub-batch paths
  const int64_t lim = sg_switch_ll<SW_CONV_MAX_BYTES>();
  return lim > 0 ? lim : (1ll << 31) - (1ll << 20);
}
inline int images_per_2gib(const sg_conv_desc* d, int ebx, int eby) {
  const int64_t xl = d->x_ld ? d->x_ld : d->Cin, yl = d->y_ld ? d->y_ld : d->Cout;
  const int64_t xi = (int64_t)d->H * d->W * xl * ebx, yi = (int64_t)d->Ho * d->Wo * yl * eby;
  const int64_t per = xi > yi ? xi : yi;
  const int64_t lim = images_limit_bytes();
  if (per * d->N < lim) return d->N;
  const int64_t nb = lim / per;
  return (int)(nb < 1 ? 0 : nb);
}

void fill_fwd_params(IgemmParams& p, const sg_conv_desc* d, const void* x, const void* w, const void* bias, void* y,
                     int flags, int eb) {
  p.x = (const float*)x;
  p.w = (const float*)w;
  p.bias = (const float*)bias;
  p.y = (float*)y;
  p.H = d->H; p.W = d->W; p.C = d->Cin; p.x_ld = d->x_ld ? d->x_ld : d->Cin;
  p.OH = d->Ho; p.OW = d->Wo;
  p.Nout = d->Cout; p.y_ld = d->y_ld ? d->y_ld : d->Cout;
  p.a_mul = d->stride; p.k_mul = d->dilation; p.off_h = -d->pad_t; p.off_w = -d->pad_l; p.div = 1;
  p.K = d->KH * d->KW * d->Cin;
  p.M = d->N * d->Ho * d->Wo;
  p.flags = flags;
  p.fd_ohow = make_fastdiv((uint32_t)(d->Ho * d->Wo));
  p.fd_ow = make_fastdiv((uint32_t)d->Wo);
  p.fd_c = make_fastdiv((uint32_t)d->Cin);
  p.fd_kw = make_fastdiv((uint32_t)d->KW);
  const int64_t xb = (((int64_t)d->N * d->H * d->W - 1) * p.x_ld + d->Cin) * eb, wb = (int64_t)p.K * d->Cout * 4;
  p.x_bytes = xb < (1ll << 31) ? (uint32_t)xb : 0;
  p.w_bytes = wb < (1ll << 31) ? (uint32_t)wb : 0;
  p.stats = nullptr;
  p.perm2 = 0;
  p.res = nullptr;
  p.a_planes = nullptr;
  p.bn.mean = nullptr;
  p.bnb.x = nullptr;
}

void fill_dgrad_params(IgemmParams& p, const sg_conv_desc* d, const void* dy, const void* wt, const void* bias, void* dx,
                       int flags, int eb) {
  p.x = (const float*)dy;
  p.w = (const float*)wt;
  p.bias = (const float*)bias;
  p.y = (float*)dx;
  p.H = d->Ho; p.W = d->Wo; p.C = d->Cout; p.x_ld = d->y_ld ? d->y_ld : d->Cout;
  p.OH = d->H; p.OW = d->W;
  p.Nout = d->Cin; p.y_ld = d->x_ld ? d->x_ld : d->Cin;
  p.a_mul = 1; p.k_mul = -d->dilation; p.off_h = d->pad_t; p.off_w = d->pad_l; p.div = d->stride;
  p.K = d->KH * d->KW * d->Cout;
  p.M = d->N * d->H * d->W;
  p.flags = flags;
  p.fd_ohow = make_fastdiv((uint32_t)(d->H * d->W));
  p.fd_ow = make_fastdiv((uint32_t)d->W);
  p.fd_c = make_fastdiv((uint32_t)d->Cout);
  p.fd_kw = make_fastdiv((uint32_t)d->KW);
  const int64_t xb = (((int64_t)d->N * d->Ho * d->Wo - 1) * p.x_ld + d->Cout) * eb, wb = (int64_t)p.K * d->Cin * 4;
  p.x_bytes = xb < (1ll << 31) ? (uint32_t)xb : 0;
  p.w_bytes = wb < (1ll << 31) ? (uint32_t)wb : 0;
  p.stats = nullptr;
  p.perm2 = 0;
  p.res = nullptr;
  p.a_planes = nullptr;
  p.bn.mean = nullptr;
  p.bnb.x = nullptr;
}

// ---- plan_conv(): fills the ConvPlan that every query and launch reads (the struct: conv_common.h; run_x6: above) ----
// `mode`: the arithmetic on fp32 storage (x6_mode(); the workspace queries, which know neither it nor the storage type, ask for 1)
ConvPlan plan_conv_mode(int mode, int dtype, const sg_conv_desc* d, bool dgrad, int flags) {
  ConvPlan pl;
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  const bool f32 = dt_storage(dtype) == SG_F32 && !head32;
  const int eb = dt_bytes(dtype);
  const bool x_dense = !d->x_ld || d->x_ld == d->Cin, y_dense = !d->y_ld || d->y_ld == d->Cout;
  pl.up2 = f32 && mode == 1 && x6p_up2_geom(d) && x6wp_geom(d);   // (forward and filter gradient both take the patch kernels)
  const bool thin = thin_ok(d) && !(flags & PLAN_NOT_THIN) && !(dgrad && (flags & (SG_EPI_BIAS | SG_EPI_RELU)));
  if (head32) {   // the thin head goes in one launch, the other one in sub-batches of bf16 x / fp32 y
    pl.family = thin ? CONV_THIN : CONV_HEAD;
    pl.nb = thin ? d->N : images_per_2gib(d, 2, 4);
    return pl;
  }
  pl.nb = images_per_2gib(d, eb, eb);
  if (thin) {
    pl.family = CONV_THIN;
    pl.res = dgrad;
    pl.bn_in = !dgrad && f32 && !(dtype & SG_X_UP2) && x_dense;
    return pl;
  }
  if (pl.nb < 1 || (dgrad && d->stride != 1 && d->stride != 2)) return pl;
  // the GEMM view of one launch (C = the depth of one tap of the reduction: Cin forward, Cout dgrad); geometry fields only
  sg_conv_desc one = *d;
  if (pl.nb < d->N) one.N = pl.nb;
  IgemmParams g;
  if (!dgrad) fill_fwd_params(g, &one, nullptr, nullptr, nullptr, nullptr, 0, eb);
  else fill_dgrad_params(g, &one, nullptr, nullptr, nullptr, nullptr, 0, eb);
  const int ch = b16 ? 8 : 4;
  pl.vec = (g.C % ch == 0) && (g.x_ld % ch == 0) && (g.Nout % 4 == 0);
  const bool vpad_safe = (g.C % BK == 0) || (g.K == g.C) || (g.x_ld == g.C);   // padded reads must stay inside the tensor
  if (!(vpad_safe && x6_ok(g, pl.vec, b16 || mode != 0))) return pl;
  const int perm_on = sg_switch<SW_DGRAD_PERM2>();
  pl.perm2 = (dgrad && perm_on && d->stride == 2 && d->dilation == 1 && d->H % 2 == 0 && d->W % 2 == 0 && d->KH * d->KW <= 64) ? 1 : 0;
  pl.npl = (b16 || mode == 2) ? 1 : 3;   // 3: the exact fp32 emulation, 1: bf16 products
  pl.Ck = pl.Ckp = g.C;
  pl.K = g.K;
  if (g.C % BK != 0 && g.K != g.C) {   // virtual channel padding: whole slabs inside one tap (slab family; the others never need it)
    pl.Ckp = x6_vpad_c(g.C);
    pl.K = (g.K / g.C) * pl.Ckp;
    g.C = pl.Ckp;
    g.K = pl.K;
  }
  const int N = g.Nout;
  const int xw = (pl.npl == 3) ? x6w_shares(g) : 0;
  if (pl.npl == 3 && pl.Ckp == pl.Ck && x6p_geom(g, d->KH, d->KW) && !(g.C > 64 && xw > 0)) {
    pl.family = CONV_PATCH;
    pl.Kpad = pl.K;
    pl.Npad = N;
    pl.nblocks = (int)sg_cdiv((int64_t)(pl.K / 16) * (N / 32) * 64, 256);
    pl.w_bytes = (size_t)3 * pl.K * N * 2;
    pl.bn_in = !dgrad && !(dtype & SG_X_UP2) && x_dense && (g.C == 32 || g.C == 64);   // (not the 64-channel-chunk form)
    return pl;
  }
  const int wbn = (pl.nb >= d->N && (pl.npl == 3 || b16)) ? pw_wide_width(g) : 0;
  if (wbn) {   // k-block-major planes (conv_pw.h)
    pl.family = CONV_WIDE;
    pl.wbn = wbn;
    pl.Ckp = pl.K;
    pl.kd = pw_kd(pl.npl);
    pl.Kpad = pw_kpad(pl.K, pl.npl);
    pl.Npad = pw_npad(N, wbn);
    pl.nblocks = (int)(sg_cdiv(pl.Kpad, 32) * sg_cdiv(pl.Npad, 32));
    pl.w_bytes = pw_planes_bytes(pl.K, N, pl.npl, wbn);
    // (launch_pw_wide reads the same two switches: the BatchNormalization-backward form needs the default schedule, no ablation)
    pl.bnb = dgrad && pl.npl == 3 && !(dtype & SG_X_UP2) && x_dense && y_dense && d->Cout + 16 <= PW_BNB_MAXK &&
             sg_switch<SW_PW_VAR>() == 1 && sg_switch<SW_PW_ABLATE>() == 0;
    return pl;
  }
  pl.family = CONV_SLAB;
  pl.res = dgrad;
  pl.deep = b16 && sg_switch<SW_B16_DEEP>();   // A/B switch
  pl.kd = x6_plane_kd(b16, pl.Ckp, pl.K == pl.Ckp);
  pl.Kpad = x6_kpad(pl.K, pl.kd);
  pl.Npad = x6_npad(N);
  pl.nblocks = (pl.Kpad / 32) * (pl.Npad / 32);
  pl.w_bytes = x6_planes_bytes(pl.K, N, pl.npl, pl.kd);
  const size_t img_part = (size_t)g.OH * g.OW * N * sizeof(float);   // one K share's partial slab of one image
  if (pl.npl == 3 && pl.kd == XW_KD && xw > 0) {
    // the long-K multi-tap convolutions: the activation split once into bf16 planes, 128 x 256 tiles with both operands by LDS-DMA
    pl.x6w_S = xw;
    pl.a_img_bytes = (size_t)3 * g.H * g.W * g.C * 2;
    pl.part_img_bytes = xw > 1 ? xw * img_part : 0;
    pl.planes_in = pl.Ckp == pl.Ck && x_dense && y_dense;   // (planes are dense and have the unpadded depth)
  }
  if (pl.deep && pl.kd == BW_KD) {
    // long reductions with 192+ output columns: 256 x 256 tiles, both operands by LDS-DMA, split-K where the tiles are few
    pl.b16w_S = b16w_shares(g);
    pl.part_img_bytes = pl.b16w_S > 1 ? pl.b16w_S * img_part : 0;
  }
  return pl;
}

// num_cus: no choice depends on it today (the tile shapes that do - pick_bn, the 1024-tile crossover - are picked per launch)
ConvPlan plan_conv(int num_cus, int dtype, const sg_conv_desc* d, bool dgrad, int flags) {
  (void)num_cus;
  return plan_conv_mode(x6_mode(), dtype, d, dgrad, flags);
}

// ---- plan_wgrad(): the filter gradient's counterpart of plan_conv() -----------------------------------------------------
// Everything a filter-gradient call decides - the kernel family, the slab kernel's form, the pixel split, the sub-batches, the
// workspace layout, the fused operands it can take - from what a call knows: the CU count, the storage type (SG_HEAD_F32 and
// SG_X_UP2 included), the descriptor, the alignment CLASS of x and of dy (16, 8 or 0 bytes; never the pointers) and whether the
// operands are bf16 planes.  sg_conv2d_wgrad, sg_conv2d_wgrad_planes, both workspace queries, sg_conv2d_caps and
// sg_conv2d_wgrad_plan read this one plan; run_wgrad() launches what it names and decides nothing.
// WgradParams' x_bytes / dy_bytes for a launch of `d`: the operands' extents, 0 = beyond the 2 GiB of a buffer descriptor
inline void wgrad_extents(int dtype, const sg_conv_desc* d, uint32_t& x_bytes, uint32_t& dy_bytes) {
  const int up = (dtype & SG_X_UP2) ? 1 : 0, eb = dt_bytes(dtype), eby = (dtype & SG_HEAD_F32) ? 4 : eb;
  const int64_t xl = d->x_ld ? d->x_ld : d->Cin, yl = d->y_ld ? d->y_ld : d->Cout;
  const int64_t xb = (((int64_t)d->N * (d->H >> up) * (d->W >> up) - 1) * xl + d->Cin) * eb;
  const int64_t yb = (((int64_t)d->N * d->Ho * d->Wo - 1) * yl + d->Cout) * eby;
  x_bytes = xb < (1ll << 31) ? (uint32_t)xb : 0;
  dy_bytes = yb < (1ll << 31) ? (uint32_t)yb : 0;
}

// Split of the pixel reduction over S workgroups per tile of the slab kernels.  Modelled time = MFMA work / (fraction of the
// 2*CUs workgroup slots kept busy over whole waves) + the traffic of writing and re-adding S partial slabs; the S with the
// smallest modelled time wins (e.g. ASPP: 288 tiles -> S = 7: 2016 workgroups = 3.94 waves).  It knows the descriptor and the
// storage type, no pointers and no byte limits.
static int wgrad_slab_split(int num_cus, const sg_conv_desc* d, bool b16) {
  const int64_t K = (int64_t)d->KH * d->KW * d->Cin, P = (int64_t)d->N * d->Ho * d->Wo;
  const int bn = wgrad_bn(d->Cout);
  const int64_t tiles = sg_cdiv(K, BM) * sg_cdiv(d->Cout, bn);
  const int64_t nslab = sg_cdiv(P, BK);
  const int64_t slots = 2 * (int64_t)num_cus;
  const double flops = 2.0 * (double)tiles * BM * bn * (double)P;  // padded tile work
  // Sustained rate of the kernel that will run: wgrad_x6_kernel's or the fp32 MFMA one's.  The test is wgrad_x6_geom, the
  // geometry half of wgrad_x6_ok, loosened in two ways that stay because S - and with it the order of the sum - hangs on them:
  // a stride-2 layer counts whatever its padding (wgrad_x6_ok also wants Ho = ceil(H / 2)), and of the launch's 16-byte test
  // only Cin % 4 is asked, not the pixel strides, Cout % 4, the alignment or the arithmetic switch.
  const bool x6_rate = (wgrad_x6_geom(d) || (d->stride == 2 && d->dilation == 1 && d->Wo % BK == 0 && d->Cout >= 16)) && d->Cin % 4 == 0;
  const double rate_x6 = sg_switch_f<SW_WGRAD_PLAN_RATE>() * 1e12;
  // the one-pass bf16 kernel multiplies ~4x faster than the six-pass one: the split's partial-slab traffic weighs more
  const double rate_b16 = sg_switch_f<SW_WGRAD_PLAN_RATE_B16>() * 1e12;  // measured 110 / 250 / 450 / 900: no gain from a higher rate (profiles/r02_b16_deep_ab.txt)
  const double rate = x6_rate ? (b16 ? rate_b16 : rate_x6) : 110e12;
  int64_t maxS = nslab / 8;  // at least 8 slabs per split
  if (maxS < 1) maxS = 1;
  if (maxS > 512) maxS = 512;
  double best_t = 1e300;
  int64_t best_S = 1;
  for (int64_t S = 1; S <= maxS; ++S) {
    const int64_t wgs = tiles * S;
    const double eff = (double)wgs / (double)(sg_cdiv(wgs, slots) * slots);
    const double part_bytes = S > 1 ? (double)S * (double)K * d->Cout * 4.0 : 0.0;
    if (part_bytes > (double)(384ll << 20)) break;
    const double t = flops / (eff * rate) + 2.0 * part_bytes / 3.0e12 + (S > 1 ? 3e-6 : 0.0);
    if (t < best_t * 0.999) { best_t = t; best_S = S; }
  }
  return (int)best_S;
}

// One launch of the plan: `n` images of `dm`, the descriptor of the whole batch or of a full sub-batch (n < dm->N: the last,
// smaller sub-batch).  The family and the share count S0 come from dm, so that the last sub-batch takes the kernel of the others
// and never writes more partial slabs than one of them; its own size only shortens the shares.  ax / ay: alignment class of x / dy.
static WgradLaunch plan_wgrad_launch(int num_cus, int dtype, const sg_conv_desc* dm, int n, int ax, int ay) {
  WgradLaunch f = {};
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  sg_conv_desc dd = *dm;
  dd.N = n;
  const sg_conv_desc* d = &dd;
  const int xl = d->x_ld ? d->x_ld : d->Cin, yl = d->y_ld ? d->y_ld : d->Cout, taps = d->KH * d->KW;
  const int64_t P = (int64_t)n * d->Ho * d->Wo, nslab = sg_cdiv(P, BK);
  const bool thin = thin_ok(dm);
  if (thin && ax == 16) {   // (dy is read by scalar loads)
    f.family = SG_WG_THIN;
    f.S = 1;
    return f;
  }
  uint32_t xb, yb;
  wgrad_extents(dtype, d, xb, yb);
  const bool a16 = ax == 16 && ay == 16;
  const bool dma = a16 && xb != 0 && yb != 0 && !head32;   // what the wide pointwise and the patch kernel ask of their operands
  const bool wide = !thin && (b16 || x6_mode() == 1) && wgrad_pw_wide_geom(dm, b16 ? 2 : 4);   // 1x1, stride 1, wide enough (conv_pw.h)
  const bool patch = !thin && !wide && x6wp_geom(dm) && (b16 || x6_enabled()) && xl % (b16 ? 8 : 4) == 0 && yl % (b16 ? 8 : 4) == 0;
  int S0;   // shares of the family's own kernel on dm
  if (thin) {
    S0 = 1;   // (unaligned x: one share of the slab kernels straight into dw, which needs no more workspace than the thin plan)
  } else if (wide) {
    const int kp = b16 ? WPB_KP : 16;
    int k0;
    wgrad_pw_wide_plan(num_cus, dm, S0, k0, kp);
    if (dma) {
      f.family = SG_WG_WIDE;
      f.planes = (b16 || x6_mode() == 2) ? 1 : 3;
      f.step_px = kp;
      wgrad_pw_wide_plan(num_cus, d, f.S, f.steps, kp);   // its own k-steps: a last, smaller sub-batch has fewer
      if (f.S > S0) {   // never more partial slabs than a full sub-batch
        f.steps = (int)sg_cdiv(sg_cdiv(P, kp), S0);
        f.S = (int)sg_cdiv(sg_cdiv(P, kp), f.steps);
      }
      return f;
    }
  } else if (patch) {
    S0 = x6wp_grid(num_cus, dm);
    if (dma) {
      f.family = SG_WG_PATCH;
      f.planes = (b16 || x6_mode() == 2) ? 1 : 3;
      f.S = x6wp_grid(num_cus, d);   // (a last, smaller sub-batch may have fewer tiles than slots)
      f.step_px = BK;
      f.steps = (int)sg_cdiv(nslab, f.S);
      return f;
    }
  } else {
    S0 = wgrad_slab_split(num_cus, dm, b16);
  }
  // The slab kernels: the layer's own family, or the fallback of a thin / wide / patch layer whose operands miss that kernel's
  // alignment or byte limit.  A fallback cuts ITS slabs into at most S0 shares (<= the aligned plan's partial slabs: no fallback
  // needs more workspace than the aligned plan); the slab family proper keeps the shares of a full sub-batch for the last one too.
  const int64_t ns = (thin || wide || patch) ? nslab : sg_cdiv((int64_t)dm->N * d->Ho * d->Wo, BK);
  f.steps = (int)sg_cdiv(ns, S0);
  f.S = (int)sg_cdiv(ns, f.steps);
  f.step_px = BK;
  f.bn = wgrad_bn(d->Cout);
  const bool g4 = d->Cin % 4 == 0 && xl % 4 == 0 && d->Cout % 4 == 0 && yl % 4 == 0;
  const bool g8 = d->Cin % 8 == 0 && xl % 8 == 0 && d->Cout % 8 == 0 && yl % 8 == 0;
  if (head32) {   // x bf16, dy fp32 (not a thin 1x1 convolution)
    f.family = SG_WG_HEAD32;
    f.vec = (g4 && ax >= 8 && ay == 16) ? 4 : 0;
    return f;
  }
  const bool vec = (b16 ? g8 : g4) && a16;
  const int skip = (!sg_switch<SW_CONV_NOSKIP>() && d->dilation > 1 && taps > 1) ? 1 : 0;
  if (wgrad_x6_ok(d, vec, b16, xb, yb)) {
    f.family = SG_WG_SLAB_X6;
    f.vec = b16 ? 8 : 4;
    f.planes = (b16 || x6_mode() == 2) ? 1 : 3;   // 1 on fp32 storage: bf16 products in one pass
    f.skip_slabs = skip;
    f.tap_inner = ((conv_l2(true) & 4) && taps > 1 && d->Cin % BM == 0) ? 1 : 0;
    f.stagger = b16 ? 0 : sg_switch<SW_X6_ABLATE>() & 7;  // the x6 wgrad kernel has no stagger; the field carries the ablation mask
    return f;
  }
  f.family = SG_WG_SLAB_NATIVE;
  if (b16) {   // widening loads, no buffer addressing
    f.vec = (g4 && ax >= 8 && ay >= 8) ? 4 : 0;
    return f;
  }
  f.vec = vec ? 4 : 0;
  f.skip_slabs = skip;
  f.tap_inner = ((conv_l2() & 4) && taps > 1 && d->Cin % BM == 0) ? 1 : 0;
  f.stagger = 1;
  if (vec && d->stride == 1 && d->Ho == d->H && d->Wo == d->W && xb != 0 && yb != 0) {   // FAST: see igemm_wgrad_kernel
    const bool force1 = sg_switch<SW_WGRAD_FAST1>();  // A/B switch
    f.fast = (!force1 && (d->Wo % BK == 0) && (taps == 1 || d->Cin % BM == 0) && ((int64_t)xb + 2 * 32 * (int64_t)xl * 4 < (1ll << 31))) ? 2 : 1;
  }
  return f;
}

// planes: the plan of sg_conv2d_wgrad_planes (fp32 layers, both operands as 16-byte aligned bf16 planes); family 0 = not covered
WgradPlan plan_wgrad(int num_cus, int dtype, const sg_conv_desc* d, int ax, int ay, bool planes) {
  WgradPlan pl = {};
  const int64_t K = (int64_t)d->KH * d->KW * d->Cin, P = (int64_t)d->N * d->Ho * d->Wo;
  if (planes) {
    if (x6_mode() != 1) return pl;
    if (d->stride != 1 || d->Ho != d->H || d->Wo != d->W || (d->Wo % 32) || (d->Cin % 8) || (d->Cout % 8) || d->Cout < 16) return pl;
    if ((d->x_ld && d->x_ld != d->Cin) || (d->y_ld && d->y_ld != d->Cout)) return pl;   // planes are dense
    const int64_t xp = (int64_t)d->N * d->H * d->W * d->Cin * 2, yp = P * d->Cout * 2;
    const int64_t sh = ((int64_t)d->pad_t * d->W + d->pad_l + 64) * d->Cin * 4;
    if (3 * xp + 2 * sh >= (1ll << 31) || 3 * yp >= (1ll << 31)) return pl;
    dtype = SG_F32;   // the shares below are those of the layer's fp32-operand launch: the same sum in the same order
    ax = ay = 16;
  }
  // Sub-batches of whole images keep every launch's operands inside a 2 GiB buffer descriptor.  images_per_2gib counts 4-byte
  // elements for bf16 storage too: that fixes the chunking, and with it the order of the sum, for both storage types alike.
  const int nb = images_per_2gib(d, 4, 4);
  const bool chunked = nb >= 1 && nb < d->N && !thin_ok(d);
  pl.nb = chunked ? nb : d->N;
  pl.chunks = chunked ? (int)sg_cdiv(d->N, nb) : 1;
  pl.tail_n = d->N - (pl.chunks - 1) * pl.nb;
  sg_conv_desc dm = *d;
  dm.N = pl.nb;
  pl.main = plan_wgrad_launch(num_cus, dtype, &dm, pl.nb, ax, ay);
  pl.tail = pl.tail_n == pl.nb ? pl.main : plan_wgrad_launch(num_cus, dtype, &dm, pl.tail_n, ax, ay);
  if (planes) {
    if (pl.main.family != SG_WG_SLAB_X6 || pl.chunks > 1) return WgradPlan{};   // a thin, wide pointwise or patch layer, or beyond 2 GiB
    WgradLaunch& f = pl.main;
    f.family = SG_WG_PLANES;
    f.vec = 8;
    f.stagger = sg_switch<SW_X6_ABLATE>() & 15;   // timing-only diagnostics
    // SG_WGRAD_PIN_SMUL: more, shorter pixel shares than the fp32-operand plan (the planes are 1.5 x the bytes per pixel: the share
    // of x that the workgroups of an XCD walk together should still fit its L2)
    const int smul = sg_switch<SW_WGRAD_PIN_SMUL>();
    if (smul > 1 && f.S > 1) {
      const int64_t nslab = sg_cdiv(P, BK);
      int64_t S = (int64_t)f.S * smul;
      if (S > nslab / 4) S = nslab / 4 > 0 ? nslab / 4 : 1;
      f.steps = (int)sg_cdiv(nslab, S);
      f.S = (int)sg_cdiv(nslab, f.steps);
    }
    pl.tail = f;
  }
  pl.max_parts = (pl.chunks - 1) * pl.main.S + pl.tail.S;
  if (pl.chunks > 1) pl.dw_part_bytes = (size_t)pl.chunks * pl.main.S * K * d->Cout * 4;   // every sub-batch writes partial slabs
  else if (pl.main.family == SG_WG_THIN) pl.dw_part_bytes = thin_part_bytes(num_cus, d);
  else pl.dw_part_bytes = pl.main.S > 1 ? (size_t)pl.main.S * K * d->Cout * 4 : 0;
  pl.bias_part_bytes = planes ? 0 : colsum_ws_bytes(num_cus, P, d->Cout);   // (the planes-in call has no bias gradient)
  pl.bias_off = (pl.dw_part_bytes + 255) & ~(size_t)255;   // 256-byte aligned, after the dw partials
  pl.ws_bytes = pl.dw_part_bytes + pl.bias_part_bytes + 512;
  // the fused operands: only the thin and the patch kernel apply a BatchNormalization to x (fp32 storage, dense pixels), only the
  // patch kernel gathers from the source of an up-sampling
  const bool f32 = dt_storage(dtype) == SG_F32 && !(dtype & SG_HEAD_F32);
  const bool x_dense = !d->x_ld || d->x_ld == d->Cin;
  // (a layer's forward and filter gradient take the BatchNormalization together or not at all: the forward's plan is asked too)
  pl.bn_in = (pl.main.family == SG_WG_THIN || pl.main.family == SG_WG_PATCH) && f32 && !(dtype & SG_X_UP2) && x_dense &&
             plan_conv(num_cus, dtype, d, false, 0).bn_in;
  pl.up2 = pl.main.family == SG_WG_PATCH && !(dtype & SG_HEAD_F32) && x6p_up2_geom(d);
  return pl;
}

}  // namespace

extern "C" {

int sg_set_conv_x6(int on) {
  const int prev = x6_mode();
  g_x6_mode = (on < 0 || on > 2) ? 1 : on;
  return prev;
}

// scratch behind the weight planes (0: none).  The workspace queries know neither the storage type nor the arithmetic: the larger
// of the bf16 plan and the fp32 six-pass plan, for the whole batch
static size_t conv_ws_scratch(const sg_conv_desc* d, bool dgrad) {
  if (check_desc(d, "sg_conv2d_ws_bytes")) return 0;
  const size_t b = plan_conv_mode(1, SG_BF16, d, dgrad, 0).scratch_bytes(d->N), f = plan_conv_mode(1, SG_F32, d, dgrad, 0).scratch_bytes(d->N);
  const size_t n = b > f ? b : f;
  return n ? n + 256 : 0;
}

size_t sg_conv2d_fwd_ws_bytes(const sg_conv_desc* d) {
  if (!d) return 0;
  size_t n = x6_ws_bytes(d->KH * d->KW, d->Cin, d->Cout) + 256 + conv_ws_scratch(d, false);
  if (n < x6p_up2_ws_bytes()) n = x6p_up2_ws_bytes();
  return n;
}

size_t sg_conv2d_fwd_stats_bytes(const sg_conv_desc* d) {
  if (!d) return 0;
  return (size_t)sg_cdiv((int64_t)d->N * d->Ho * d->Wo, BM) * 2 * d->Cout * sizeof(float);
}

// stride 1, SAME, 32 / 64 input channels: conv_x6p.h forward, conv_x6wp.h filter gradient), fp32 storage.  Forward AND filter
// gradient must both take the operand: the filter gradient's plan answers for the pair
static bool bn_in_geom(const sg_ctx* ctx, int dtype, const sg_conv_desc* d) {
  return plan_wgrad(ctx->num_cus, dtype, d, 16, 16, false).bn_in != 0;
}

// sg_conv_opts: a NULL pointer is the plain launch
static const sg_conv_opts kNoOpts = {};

// alignment class of a pointer, as plan_wgrad and sg_conv2d_plan take it
static int align_class(const void* p) { return aligned16(p) ? 16 : ((reinterpret_cast<uintptr_t>(p) & 7) == 0 ? 8 : 0); }

// Channel runs of a launch of the native kernel (16 bytes of fp32, 8 of bf16): from the descriptor, the alignment class of the
// activation operand it reads (x; dgrad: dy) and, where the kernel reads w itself (the fp32 forward), that of w.  The launches and
// sg_conv2d_plan both ask here.
static bool native_vec_of(int dtype, const sg_conv_desc* d, bool dgrad, int a_class, bool w16) {
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  const int ca = dgrad ? d->Cout : d->Cin, cn = dgrad ? d->Cin : d->Cout;
  const int ld = dgrad ? (d->y_ld ? d->y_ld : d->Cout) : (d->x_ld ? d->x_ld : d->Cin);
  if ((ca % 4) || (ld % 4)) return false;
  if (head32 && dgrad) return a_class == 16;   // (fp32 dy)
  if (b16) return a_class >= 8;                // the 4-channel loads of bf16 storage
  return cn % 4 == 0 && a_class == 16 && (dgrad || w16);
}

// A thin launch's operands against its kernels' alignment: the tensor with Cin channels (x; dgrad: dx) 16-byte aligned, in every
// sub-batch.  Where this fails the plan is taken again with PLAN_NOT_THIN.
static bool thin_operands_ok(const ConvPlan& pl, const sg_conv_desc* d, bool a16, int ebx) {
  const int xl = d->x_ld ? d->x_ld : d->Cin;
  return a16 && (pl.nb >= d->N || pl.nb < 1 || ((int64_t)d->H * d->W * xl * ebx) % 16 == 0);
}

// one launch of the plan: the whole batch or one sub-batch of it (`d`: its images).  The caller has checked the operands against
// the plan: `fast` = they allow the plan's plane kernel (else: the native kernel)
static int conv2d_fwd_launch(sg_ctx* ctx, hipStream_t st, int dtype, const sg_conv_desc* d, const ConvPlan& pl, bool fast,
                             const void* x, const void* w, const void* bias, void* y, int flags, void* ws, bool prepared, void* stats,
                             int* tiles_out, const void* x_planes, const sg_bn_in* bn) {
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  if (pl.family == CONV_THIN)   // (only the fp32 kernel applies a BatchNormalization)
    return launch_thin_fwd(d, b16, b16 && !head32, x, (const float*)w, (const float*)bias, y, flags, st, b16 ? bn_in_none() : bn_in_of(bn));
  IgemmParams p;
  fill_fwd_params(p, d, x, w, bias, y, flags, dt_bytes(dtype));
  if (pl.family == CONV_HEAD) {   // a head that is not a 1x1 convolution: the any-shape kernel, bf16 in, fp32 out
    return dispatch_igemm(p, true, false, native_vec_of(dtype, d, false, align_class(x), true), ctx->num_cus, st);
  }
  if (fast) {
    if (!b16 && p.x_ld == d->Cin) p.a_planes = (const unsigned short*)x_planes;
    p.bn = bn_in_of(bn);
    if (stats && tiles_out && !(flags & SG_EPI_RELU)) {  // the statistics ride in the x6 kernel's epilogue only
      p.stats = (float*)stats;
      *tiles_out = (int)sg_cdiv(p.M, BM);
    }
    if (b16) return run_x6<1, bf16_t>(pl, p, (const float*)w, false, d->Cin, d->Cout, ws, ctx->num_cus, st, prepared);
    if (pl.npl == 1) return run_x6<1, float>(pl, p, (const float*)w, false, d->Cin, d->Cout, ws, ctx->num_cus, st, prepared);
    return run_x6<3, float>(pl, p, (const float*)w, false, d->Cin, d->Cout, ws, ctx->num_cus, st, prepared);
  }
  const bool vec4 = native_vec_of(dtype, d, false, align_class(x), aligned16(w));
  return dispatch_igemm(p, b16, b16, vec4, ctx->num_cus, st);
}

int sg_conv2d_fwd(sg_ctx* ctx, void* stream, int dtype, const sg_conv_desc* d, const void* x, const void* w,
                  const void* bias, void* y, int flags, const sg_conv_opts* opts) {
  const sg_conv_opts& o = opts ? *opts : kNoOpts;
  void* const ws = o.ws;
  const size_t ws_bytes = o.ws_bytes;
  void* const stats = o.stats;
  int* const tiles_out = o.tiles_out;
  const void* const x_planes = o.a_planes;
  const sg_bn_in* const bn = o.bn_in;
  SG_CHECK_ARG(!o.res && !o.bnb, "sg_conv2d_fwd: res / bnb are operands of the input gradient");
  SG_CHECK_ARG(!(bn && x_planes), "sg_conv2d_fwd: bn_in with a_planes (the planes hold the raw tensor's split)");
  if (bn) {
    SG_CHECK_ARG(bn->mean && bn->invstd && bn->gamma && bn->beta, "sg_conv2d_fwd: bn_in with null BatchNormalization parameters");
    SG_CHECK_ARG(ctx && d, "sg_conv2d_fwd: null argument");
    if (check_desc(d, "sg_conv2d_fwd") || !bn_in_geom(ctx, dtype, d) || (flags & SG_PRO_UP2)) {
      sg_set_error("sg_conv2d_fwd: bn_in, but this launch takes neither a thin 1x1 nor a patch kernel (3x3 s1 SAME, 32 / 64 input "
                   "channels, fp32 storage): no kernel to apply the BatchNormalization in");
      return SG_EUNSUPPORTED;
    }
  }
  SG_CHECK_ARG(!x_planes || aligned16(x_planes), "sg_conv2d_fwd: a_planes must be 16-byte aligned");
  if (tiles_out) *tiles_out = 0;
  SG_CHECK_ARG(ctx != nullptr, "sg_conv2d_fwd: null ctx");
  SG_CHECK_ARG(dt_ok(dtype), "sg_conv2d_fwd: dtype %d", dtype);
  int rc = check_desc(d, "sg_conv2d_fwd");
  if (rc) return rc;
  SG_CHECK_ARG(x && w && y, "sg_conv2d_fwd: null tensor");
  SG_CHECK_ARG(!(flags & SG_EPI_BIAS) || bias, "sg_conv2d_fwd: SG_EPI_BIAS without bias");
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  const int eb = dt_bytes(dtype);
  SG_CHECK_ARG(!head32 || (b16 && d->Cout <= 4), "sg_conv2d_fwd: SG_HEAD_F32 needs Cout <= 4 (a softmax head) on bf16 storage");
  SG_CHECK_ARG(!(dtype & SG_X_UP2), "sg_conv2d_fwd: SG_X_UP2 is the filter gradient's flag (forward: SG_PRO_UP2)");
  hipStream_t st = (hipStream_t)stream;
  ConvPlan pl = plan_conv(ctx->num_cus, dtype, d, false, flags);
  const int xl = d->x_ld ? d->x_ld : d->Cin, yl = d->y_ld ? d->y_ld : d->Cout;
  if (flags & SG_PRO_UP2) {
    // UpSampling2D(2) -> Conv2D 3x3, sub-pixel form (conv_x6p.h): x is the SOURCE [N, H/2, W/2, Cin]; the kernel sees a
    // convolution on the source grid with 4 phases x Cout columns.  (The patch kernel addresses with 64-bit pointers: no
    // 2 GiB sub-batches.)
    if (!pl.up2 || !aligned16(x) || (xl % 4)) {
      sg_set_error("sg_conv2d_fwd: SG_PRO_UP2 on a launch the fused up-sampling kernel does not cover (3x3 s1 SAME, 64 -> 32, "
                   "H %% 16 = 0, W %% 32 = 0, fp32 storage, x6 arithmetic)");
      return SG_EUNSUPPORTED;
    }
    if (!ws || !aligned16(ws) || ws_bytes == SG_WS_PREPARED || ws_bytes < x6p_up2_ws_bytes()) {
      sg_set_error("sg_conv2d_fwd: SG_PRO_UP2 needs a plain workspace of %zu bytes (its summed-tap planes are made per launch)", x6p_up2_ws_bytes());
      return SG_EWORKSPACE;
    }
    sg_conv_desc sd = *d;
    sd.H = d->H / 2; sd.W = d->W / 2; sd.Ho = sd.H; sd.Wo = sd.W; sd.Cout = 4 * d->Cout;
    sd.x_ld = xl; sd.y_ld = yl;
    IgemmParams p;
    fill_fwd_params(p, &sd, x, w, bias, y, flags & (SG_EPI_BIAS | SG_EPI_RELU), eb);
    p.K = 4 * d->Cin;
    p.y_ld = yl;
    if (stats && tiles_out && !(flags & SG_EPI_RELU)) {
      p.stats = (float*)stats;
      *tiles_out = (int)sg_cdiv((int64_t)d->N * d->Ho * d->Wo, BM);   // one statistics tile per phase and source tile
    }
    return run_x6p_up2(p, (const float*)w, ws, ctx->num_cus, st);
  }
  // ---- the operands against the plan, once and before anything is written
  const bool prepared = ws_bytes == SG_WS_PREPARED;
  const int ebx = head32 ? 2 : eb, eby = head32 ? 4 : eb;
  if (pl.family == CONV_THIN && !thin_operands_ok(pl, d, aligned16(x), ebx))
    pl = plan_conv(ctx->num_cus, dtype, d, false, flags | PLAN_NOT_THIN);   // (every sub-batch's x must meet the thin kernels' alignment)
  if (pl.family == CONV_HEAD) SG_CHECK_ARG(pl.nb >= 1, "sg_conv2d_fwd: one image of the softmax head beyond 2 GiB");
  // The fast kernels address their operands through 2 GiB buffer descriptors.  A larger batch is run as sub-batches of whole
  // images (independent in a forward conv), so every image takes the same kernel - and therefore the same rounding - whatever
  // batch it travels in.  Sub-batches leave no statistics and read no activation planes.
  const int nb = (pl.nb >= 1 && pl.nb < d->N) ? pl.nb : d->N;
  bool fast = false;
  if (pl.family >= CONV_SLAB) {
    const bool have_ws = ws && aligned16(ws) && (prepared || ws_bytes >= x6_ws_bytes(d->KH * d->KW, d->Cin, d->Cout));
    fast = have_ws && pl.vec && aligned16(x) && aligned16(w);
  }
  if (pl.family != CONV_THIN && pl.family != CONV_HEAD) {
    if (bn && bn->mean && !(fast && pl.bn_in)) {   // only the patch kernel applies it
      sg_set_error("sg_conv2d_fwd: bn_in, but the launch does not take the patch kernel after all (alignment / workspace)");
      return SG_EUNSUPPORTED;
    }
    if (prepared && !fast) {
      sg_set_error("sg_conv2d_fwd: SG_WS_PREPARED planes given, but this launch does not take a prepared-planes kernel");
      return SG_EINVAL;
    }
    if (fast && !prepared && ws_bytes < pl.ws_bytes(nb)) {
      sg_set_error("sg_conv2d_fwd: workspace %zu < %zu (weight planes + activation planes + split-K partial slabs of %d + %d shares)",
                   ws_bytes, pl.ws_bytes(nb), pl.x6w_S, pl.b16w_S);
      return SG_EWORKSPACE;
    }
  }
  if (nb >= d->N) return conv2d_fwd_launch(ctx, st, dtype, d, pl, fast, x, w, bias, y, flags, ws, prepared, stats, tiles_out, x_planes, bn);
  for (int n0 = 0; n0 < d->N; n0 += nb) {
    sg_conv_desc sub = *d;
    sub.N = (d->N - n0 < nb) ? d->N - n0 : nb;
    const char* xs = (const char*)x + (int64_t)n0 * d->H * d->W * xl * ebx;
    char* ys = (char*)y + (int64_t)n0 * d->Ho * d->Wo * yl * eby;
    rc = conv2d_fwd_launch(ctx, st, dtype, &sub, pl, fast, xs, w, bias, ys, flags, ws, prepared, nullptr, nullptr, nullptr, bn);
    if (rc) return rc;
  }
  return 0;
}

int sg_get_conv_x6(void) { return x6_mode(); }

int sg_conv2d_planes_job(const sg_ctx* ctx, int dtype, const sg_conv_desc* d, int dgrad, sg_planes_job* out, size_t* bytes) {
  SG_CHECK_ARG(ctx && d && out && bytes && dt_ok(dtype), "sg_conv2d_planes_job: bad argument");
  memset(out, 0, sizeof(*out));
  *bytes = 0;
  int rc = check_desc(d, "sg_conv2d_planes_job");
  if (rc) return rc;
  // geometry only: the pointers are assumed 16-byte aligned, as the host's arenas and torch's allocator make them; a launch for
  // which that does not hold refuses the prepared planes (SG_EINVAL)
  const ConvPlan pl = plan_conv(ctx->num_cus, dtype, d, dgrad != 0, 0);
  if (pl.family < CONV_SLAB) return 0;   // kind 0: streaming kernels, no planes
  out->kind = pl.family == CONV_SLAB ? 1 : (pl.family == CONV_PATCH ? 2 : 3);
  out->s_tap = d->Cin * d->Cout;
  out->s_k = dgrad ? 1 : d->Cout;
  out->s_n = dgrad ? d->Cout : 1;
  out->N = dgrad ? d->Cin : d->Cout;
  out->npl = pl.npl;
  out->K = pl.K;
  out->Ck = pl.Ck;
  out->Ckp = pl.Ckp;
  out->kd = pl.kd;
  out->Kpad = pl.Kpad;
  out->Npad = pl.Npad;
  out->nblocks = pl.nblocks;
  *bytes = pl.ws_bytes(d->N);   // (a launch in sub-batches: the arena slot is sized for the whole batch all the same)
  return 0;
}

int sg_prepare_planes(sg_ctx* ctx, void* stream, const void* w_arena, void* planes_arena, const sg_planes_job* jobs_dev,
                      int njobs, int total_blocks) {
  SG_CHECK_ARG(ctx && w_arena && planes_arena && jobs_dev && njobs > 0 && total_blocks > 0, "sg_prepare_planes: bad argument");
  SG_CHECK_ARG(aligned16(planes_arena), "sg_prepare_planes: planes arena must be 16-byte aligned");
  return launch_prepare_planes((const float*)w_arena, (char*)planes_arena, jobs_dev, njobs, total_blocks, (hipStream_t)stream);
}

size_t sg_bn_tiles_ws_bytes(const sg_ctx* ctx, int tiles, int C) {
  if (!ctx) return 0;
  return bn_tiles_ws_bytes(ctx->num_cus, tiles, C);
}

int sg_bn_train_fwd_tiles(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, const void* stats, int tiles,
                          void* moving_mean, void* moving_var, void* save_mean, void* save_invstd, float momentum,
                          float eps, int unbiased_update, void* ws, size_t ws_bytes) {
  // dtype names the storage of the activations the statistics belong to; the statistics themselves are fp32
  SG_CHECK_ARG(ctx && (dtype == SG_F32 || dtype == SG_BF16), "sg_bn_train_fwd_tiles: bad ctx/dtype");
  SG_CHECK_ARG(rows > 0 && C > 0 && stats && tiles == (int)sg_cdiv(rows, BM) && moving_mean && moving_var && save_mean && save_invstd,
               "sg_bn_train_fwd_tiles: bad argument");
  const size_t need = bn_tiles_part_bytes(ctx->num_cus, tiles, C, stats);
  if (!ws || ws_bytes < need) {
    sg_set_error("sg_bn_train_fwd_tiles: workspace %zu < %zu", ws_bytes, need);
    return SG_EWORKSPACE;
  }
  return launch_bn_tiles(ctx->num_cus, (const float*)stats, tiles, C, rows, (float*)moving_mean, (float*)moving_var, (float*)save_mean,
                         (float*)save_invstd, momentum, eps, unbiased_update, (float*)ws, (hipStream_t)stream);
}

size_t sg_conv2d_dgrad_ws_bytes(const sg_conv_desc* d) {
  if (!d) return 0;
  const size_t native = (size_t)d->KH * d->KW * d->Cin * d->Cout * sizeof(float);
  const size_t x6 = x6_ws_bytes(d->KH * d->KW, d->Cout, d->Cin) + 256 + conv_ws_scratch(d, true);
  return native > x6 ? native : x6;
}

// the input gradient of a pointwise convolution with the BatchNormalization backward apply in its A path (conv_pw.h, BNB form)
static bool dgrad_bnb_geom(const sg_ctx* ctx, int dtype, const sg_conv_desc* d) {
  return plan_conv(ctx->num_cus, dtype, d, true, 0).bnb;
}

// one launch of the plan: the whole batch or one sub-batch of it (see conv2d_fwd_launch)
static int conv2d_dgrad_launch(sg_ctx* ctx, hipStream_t st, int dtype, const sg_conv_desc* d, const ConvPlan& pl, bool fast,
                               const void* dy, const void* w, const void* bias, void* dx, int flags, void* ws, bool prepared,
                               const void* res, const void* dy_planes, const sg_bn_bwd_in* bnb) {
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  if (pl.family == CONV_THIN) return launch_thin_dgrad(d, b16, b16 && !head32, dy, (const float*)w, dx, st, res);
  float* wt = (float*)ws;   // the native kernels read the per-tap transpose of w
  IgemmParams p;
  fill_dgrad_params(p, d, dy, wt, bias, dx, flags, head32 ? 4 : dt_bytes(dtype));
  if (fast) {
    p.res = (const float*)res;
    if (!b16 && p.x_ld == d->Cout) p.a_planes = (const unsigned short*)dy_planes;
    if (bnb) {
      p.bnb.x = (const float*)bnb->x; p.bnb.mean = (const float*)bnb->mean; p.bnb.invstd = (const float*)bnb->invstd;
      p.bnb.gamma = (const float*)bnb->gamma; p.bnb.beta = (const float*)bnb->beta; p.bnb.dgamma = (const float*)bnb->dgamma;
      p.bnb.dbeta = (const float*)bnb->dbeta; p.bnb.dz = (float*)bnb->dz; p.bnb.relu = bnb->relu ? 1 : 0;
      p.bnb.relu |= sg_switch<SW_BNB_ABLATE>() & 6;   // timing only: 2 = no dz store, 4 = no x load
      p.bnb.inv_n = 1.0f / (float)bnb->rows;
    }
    if (pl.perm2) {   // rows in parity-class order: see IgemmParams::perm2
      p.perm2 = 1;
      p.fd_mc = make_fastdiv((uint32_t)(p.M / 4));
      p.fd_hcwc = make_fastdiv((uint32_t)((d->H / 2) * (d->W / 2)));
      p.fd_wc = make_fastdiv((uint32_t)(d->W / 2));
    }
    if (b16) return run_x6<1, bf16_t>(pl, p, (const float*)w, true, d->Cin, d->Cout, ws, ctx->num_cus, st, prepared);
    if (pl.npl == 1) return run_x6<1, float>(pl, p, (const float*)w, true, d->Cin, d->Cout, ws, ctx->num_cus, st, prepared);
    return run_x6<3, float>(pl, p, (const float*)w, true, d->Cin, d->Cout, ws, ctx->num_cus, st, prepared);
  }
  const int rc = launch_transpose_taps((const float*)w, wt, d->Cin, d->Cout, d->KH * d->KW, st);
  if (rc) return rc;
  const bool vec4 = native_vec_of(dtype, d, true, align_class(dy), true);
  if (pl.family == CONV_HEAD) return dispatch_igemm(p, false, true, vec4, ctx->num_cus, st);   // fp32 dy in, bf16 dx out, any shape
  return dispatch_igemm(p, b16, b16, vec4, ctx->num_cus, st);
}

int sg_conv2d_dgrad(sg_ctx* ctx, void* stream, int dtype, const sg_conv_desc* d, const void* dy, const void* w,
                    const void* bias, void* dx, int flags, const sg_conv_opts* opts) {
  const sg_conv_opts& o = opts ? *opts : kNoOpts;
  void* const ws = o.ws;
  const size_t ws_bytes = o.ws_bytes;
  const void* const res = o.res;
  const void* const dy_planes = o.a_planes;
  const sg_bn_bwd_in* const bnb = o.bnb;
  SG_CHECK_ARG(!o.stats && !o.tiles_out && !o.bn_in, "sg_conv2d_dgrad: stats / tiles_out / bn_in are operands of the forward");
  SG_CHECK_ARG(!(res && dy_planes), "sg_conv2d_dgrad: res with a_planes (no kernel takes both)");
  if (bnb) {
    SG_CHECK_ARG(!res && !dy_planes, "sg_conv2d_dgrad: bnb with res / a_planes (the wide pointwise kernel takes neither)");
    SG_CHECK_ARG(!bias && !flags, "sg_conv2d_dgrad: bnb with a bias / flags (the BNB form has no epilogue)");
    SG_CHECK_ARG(ctx && d, "sg_conv2d_dgrad: null argument");
    SG_CHECK_ARG(bnb->x && bnb->mean && bnb->invstd && bnb->gamma && bnb->dgamma && bnb->dbeta && bnb->dz && bnb->rows > 0,
                 "sg_conv2d_dgrad: bnb with a null BatchNormalization operand");
    SG_CHECK_ARG(!bnb->relu || bnb->beta, "sg_conv2d_dgrad: bnb with a fused ReLU needs beta (the mask is recomputed from x)");
    if (check_desc(d, "sg_conv2d_dgrad") || !dgrad_bnb_geom(ctx, dtype, d) || !aligned16(bnb->x) || !aligned16(bnb->dz)) {
      sg_set_error("sg_conv2d_dgrad: bnb, but not a launch of the wide pointwise kernel (1x1, stride 1, dense fp32 operands, >= 6144 "
                   "rows, x6 arithmetic, default schedule)");
      return SG_EUNSUPPORTED;
    }
  }
  SG_CHECK_ARG(!dy_planes || aligned16(dy_planes), "sg_conv2d_dgrad: a_planes must be 16-byte aligned");
  SG_CHECK_ARG(ctx != nullptr, "sg_conv2d_dgrad: null ctx");
  SG_CHECK_ARG(dt_ok(dtype), "sg_conv2d_dgrad: dtype %d", dtype);
  int rc = check_desc(d, "sg_conv2d_dgrad");
  if (rc) return rc;
  SG_CHECK_ARG(dy && w && dx, "sg_conv2d_dgrad: null tensor");
  SG_CHECK_ARG(!(flags & SG_EPI_BIAS) || bias, "sg_conv2d_dgrad: SG_EPI_BIAS without bias");
  if (d->stride != 1 && d->stride != 2) {
    sg_set_error("sg_conv2d_dgrad: stride %d unsupported (the path uses strides 1 and 2 only)", d->stride);
    return SG_EUNSUPPORTED;
  }
  const size_t need = sg_conv2d_dgrad_ws_bytes(d);
  const bool prepared = ws_bytes == SG_WS_PREPARED;
  if (!ws || (!prepared && ws_bytes < need)) {
    sg_set_error("sg_conv2d_dgrad: workspace %zu < %zu", ws_bytes, need);
    return SG_EWORKSPACE;
  }
  SG_CHECK_ARG(aligned16(ws), "sg_conv2d_dgrad: workspace must be 16-byte aligned");
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  const int eb = dt_bytes(dtype);
  SG_CHECK_ARG(!head32 || (b16 && d->Cout <= 4), "sg_conv2d_dgrad: SG_HEAD_F32 needs Cout <= 4 (a softmax head) on bf16 storage");
  hipStream_t st = (hipStream_t)stream;
  if (res && head32) {
    sg_set_error("sg_conv2d_dgrad: res, but softmax-head launches do not add a collected gradient");
    return SG_EUNSUPPORTED;
  }
  SG_CHECK_ARG(!(dtype & SG_X_UP2) && !(flags & SG_PRO_UP2), "sg_conv2d_dgrad: the up-sampling flag of the input gradient is SG_EPI_DOWN2");
  // ---- the operands against the plan, once and before anything is written
  const int xl = d->x_ld ? d->x_ld : d->Cin, yl = d->y_ld ? d->y_ld : d->Cout;
  const int ebx = head32 ? 2 : eb, eby = head32 ? 4 : eb;   // dx (the forward's x) / dy
  ConvPlan pl = plan_conv(ctx->num_cus, dtype, d, true, flags);
  if (pl.family == CONV_THIN && !thin_operands_ok(pl, d, aligned16(dx), ebx))
    pl = plan_conv(ctx->num_cus, dtype, d, true, flags | PLAN_NOT_THIN);   // (every sub-batch's dx must meet the thin kernels' alignment)
  if (pl.family == CONV_HEAD) SG_CHECK_ARG(pl.nb >= 1, "sg_conv2d_dgrad: one image of the softmax head beyond 2 GiB");
  const int nb = (pl.nb >= 1 && pl.nb < d->N) ? pl.nb : d->N;   // sub-batches of whole images: see sg_conv2d_fwd
  const bool fast = pl.family >= CONV_SLAB && pl.vec && aligned16(dy);
  const bool down2 = (flags & SG_EPI_DOWN2) != 0;
  if (down2) {  // dx = the SOURCE's gradient [N, H/2, W/2, Cin]: the patch kernel's epilogue adds the 2 x 2 cells (conv_x6p.h)
    if (!pl.up2 || res || (flags & (SG_EPI_BIAS | SG_EPI_RELU)) || !aligned16(dy) || (yl % 4)) {
      sg_set_error("sg_conv2d_dgrad: SG_EPI_DOWN2 on a launch the fused up-sampling kernel does not cover (3x3 s1 SAME, 64 -> 32, "
                   "H %% 16 = 0, W %% 32 = 0, fp32 storage, x6 arithmetic, no bias / ReLU / collected gradient)");
      return SG_EUNSUPPORTED;
    }
    if (!(fast && pl.family == CONV_PATCH)) {  // only the patch kernel knows the flag
      sg_set_error("sg_conv2d_dgrad: SG_EPI_DOWN2, but this launch does not take the patch kernel");
      return SG_EUNSUPPORTED;
    }
  }
  if (pl.family != CONV_THIN && pl.family != CONV_HEAD) {
    if (prepared && !fast) {
      sg_set_error("sg_conv2d_dgrad: SG_WS_PREPARED planes given, but this launch does not take a prepared-planes kernel");
      return SG_EINVAL;
    }
    if (res && !(fast && pl.res)) {   // of the plane kernels only the slab family adds a collected gradient (callers ask sg_conv2d_planes_job: kind 1)
      sg_set_error("sg_conv2d_dgrad: res, but this launch takes the %s, which do not add a collected gradient (reduction channels per tap %d, "
                   "K %d, output columns %d, %d x %d outputs per image)",
                   !fast ? "fp32-MFMA kernels" : (pl.family == CONV_PATCH ? "patch kernels" : "wide pointwise kernels"), d->Cout,
                   d->KH * d->KW * d->Cout, d->Cin, d->H, d->W);
      return SG_EUNSUPPORTED;
    }
    if (bnb && !(fast && pl.family == CONV_WIDE && pl.bnb)) {   // only the wide pointwise kernel evaluates the BatchNormalization backward in its A path
      sg_set_error("sg_conv2d_dgrad: bnb, but this launch does not take the wide pointwise kernel");
      return SG_EUNSUPPORTED;
    }
    if (fast && !prepared && !res && ws_bytes < pl.ws_bytes(nb)) {
      sg_set_error("sg_conv2d_dgrad: workspace %zu < %zu (weight planes + activation planes + split-K partial slabs of %d + %d shares)",
                   ws_bytes, pl.ws_bytes(nb), pl.x6w_S, pl.b16w_S);
      return SG_EWORKSPACE;
    }
  }
  if (nb >= d->N) return conv2d_dgrad_launch(ctx, st, dtype, d, pl, fast, dy, w, bias, dx, flags, ws, prepared, res, dy_planes, bnb);
  for (int n0 = 0; n0 < d->N; n0 += nb) {
    sg_conv_desc sub = *d;
    sub.N = (d->N - n0 < nb) ? d->N - n0 : nb;
    const char* dys = (const char*)dy + (int64_t)n0 * d->Ho * d->Wo * yl * eby;
    char* dxs = (char*)dx + (int64_t)n0 * (down2 ? (d->H / 2) * (d->W / 2) : d->H * d->W) * xl * ebx;
    const char* ress = res ? (const char*)res + (int64_t)n0 * d->H * d->W * xl * ebx : nullptr;
    rc = conv2d_dgrad_launch(ctx, st, dtype, &sub, pl, fast, dys, w, bias, dxs, flags, ws, prepared, ress, nullptr, nullptr);
    if (rc) return rc;
  }
  return 0;
}

// The form of ONE launch of the plan (`d`: its images), for sg_conv2d_plan: the parameter fills of conv2d_fwd_launch /
// conv2d_dgrad_launch and run_x6, then the very rules the launchers ask (pick_bn, plan_common, igemm_ut_of, x6_var_of, x6_mf16_of,
// b16_ks, b16_pd_of, x6p_bn_of, native_vec_of).  a_class: the alignment class of the activation operand the kernel reads.
static sg_conv_launch conv_launch_form(int num_cus, int dtype, const sg_conv_desc* d, const ConvPlan& pl, bool fast, bool dgrad,
                                       int a_class, bool with_res) {
  sg_conv_launch f;
  memset(&f, 0, sizeof(f));
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  if (pl.family == CONV_THIN) {
    f.kernel = SG_CK_THIN;
    f.bn = d->Cout;
    f.vec = 1;
    return f;
  }
  IgemmParams p;
  if (!dgrad) fill_fwd_params(p, d, nullptr, nullptr, nullptr, nullptr, 0, dt_bytes(dtype));
  else fill_dgrad_params(p, d, nullptr, nullptr, nullptr, nullptr, 0, head32 ? 4 : dt_bytes(dtype));
  if (pl.family == CONV_HEAD || !fast) {
    const bool vec = native_vec_of(dtype, d, dgrad, a_class, true);
    f.kernel = SG_CK_NATIVE;
    f.vec = vec;
    if (b16) {
      f.bn = mixed_common(p, num_cus);
    } else {
      f.bn = native_common(p, vec, num_cus);
      f.ut = vec && igemm_ut_of(p);
    }
    f.skip_taps = p.skip_taps; f.group_m = p.group_m; f.cb = p.cb;
    return f;
  }
  if (dgrad && pl.perm2) p.perm2 = 1;
  if (pl.family == CONV_PATCH) {
    f.kernel = SG_CK_PATCH;
    f.bn = x6p_bn_of(p.Nout);
    f.pc = x6p_c_of(p.C);
    f.pmulti = x6p_multi_of(p.C);
    return f;
  }
  if (pl.family == CONV_WIDE) {
    f.kernel = SG_CK_WIDE;
    f.bn = pl.wbn;
    return f;
  }
  slab_fill(p, pl);
  const SlabKernel sk = slab_kernel_of(pl, b16, with_res);
  f.bn = slab_common(p, sk, b16 ? 2 : 4, num_cus);
  switch (sk) {
    case SLAB_X6W: f.kernel = SG_CK_X6W; f.bn = XW_N; break;
    case SLAB_B16W: f.kernel = SG_CK_B16W; f.bn = BW_N; break;
    case SLAB_B16:
      f.kernel = SG_CK_B16;
      f.ks = b16_ks(p.C, p.K == p.C);
      f.pd = b16_pd_of(p);
      break;
    default:
      f.kernel = SG_CK_X6;
      f.var = x6_var_of(sg_cdiv(p.M, BM) * sg_cdiv(p.Nout, f.bn), num_cus);
      f.mf16 = pl.npl == 3 && x6_mf16_of(p);
  }
  f.vec = 1;
  f.skip_taps = p.skip_taps; f.group_m = p.group_m; f.cb = p.cb;
  return f;
}

int sg_conv2d_plan(const sg_ctx* ctx, int dtype, const sg_conv_desc* d, int dgrad, int flags, int aligned, sg_conv_plan* out) {
  const char* who = dgrad ? "sg_conv2d_dgrad" : "sg_conv2d_fwd";
  SG_CHECK_ARG(out != nullptr, "sg_conv2d_plan: null out");
  memset(out, 0, sizeof(*out));
  SG_CHECK_ARG(aligned == 16 || aligned == 8 || aligned == 0, "sg_conv2d_plan: aligned %d (16, 8 or 0)", aligned);
  SG_CHECK_ARG((flags & ~(SG_EPI_BIAS | SG_EPI_RELU)) == 0, "sg_conv2d_plan: flags %d (SG_EPI_BIAS, SG_EPI_RELU; the fused up-sampling forms: `up2`)", flags);
  SG_CHECK_ARG(ctx != nullptr, "%s: null ctx", who);
  SG_CHECK_ARG(dt_ok(dtype) && !(dtype & SG_X_UP2), "%s: dtype %d", who, dtype);
  int rc = check_desc(d, who);
  if (rc) return rc;
  const bool dg = dgrad != 0, b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  SG_CHECK_ARG(!head32 || (b16 && d->Cout <= 4), "%s: SG_HEAD_F32 needs Cout <= 4 (a softmax head) on bf16 storage", who);
  if (dg && d->stride != 1 && d->stride != 2) {
    sg_set_error("sg_conv2d_dgrad: stride %d unsupported (the path uses strides 1 and 2 only)", d->stride);
    return SG_EUNSUPPORTED;
  }
  const int ebx = head32 ? 2 : dt_bytes(dtype);
  ConvPlan pl = plan_conv(ctx->num_cus, dtype, d, dg, flags);
  if (pl.family == CONV_THIN && !thin_operands_ok(pl, d, aligned == 16, ebx)) pl = plan_conv(ctx->num_cus, dtype, d, dg, flags | PLAN_NOT_THIN);
  if (pl.family == CONV_HEAD) SG_CHECK_ARG(pl.nb >= 1, "%s: one image of the softmax head beyond 2 GiB", who);
  const int nb = (pl.nb >= 1 && pl.nb < d->N) ? pl.nb : d->N;
  const bool fast = pl.family >= CONV_SLAB && pl.vec && aligned == 16;
  sg_conv_plan o;
  memset(&o, 0, sizeof(o));
  o.family = (int)pl.family;
  o.fast = fast;
  o.nb = nb;
  o.nsub = (int)sg_cdiv(d->N, nb);
  o.tail_n = d->N - (o.nsub - 1) * nb;
  o.vec = pl.vec; o.perm2 = pl.perm2; o.npl = pl.npl; o.kd = pl.kd; o.Ck = pl.Ck; o.Ckp = pl.Ckp; o.wbn = pl.wbn;
  o.x6w_S = pl.x6w_S; o.b16w_S = pl.b16w_S; o.deep = pl.deep;
  o.res = pl.res; o.bn_in = pl.bn_in; o.up2 = pl.up2; o.bnb = pl.bnb; o.planes_in = pl.planes_in;
  o.ws_bytes = pl.ws_bytes(nb);
  sg_conv_desc sub = *d;
  sub.N = nb;
  o.main = conv_launch_form(ctx->num_cus, dtype, &sub, pl, fast, dg, aligned, false);
  // (the entry point's own rule for opts->res: the thin kernels that are not the fp32 head, and fast launches of the slab family)
  if (dg && pl.res && !head32 && (pl.family == CONV_THIN || fast)) o.with_res = conv_launch_form(ctx->num_cus, dtype, &sub, pl, fast, dg, aligned, true);
  sub.N = o.tail_n;
  o.tail = conv_launch_form(ctx->num_cus, dtype, &sub, pl, fast, dg, aligned, false);
  *out = o;
  return 0;
}

// The checks that the two filter-gradient entry points and the plan query share, then the plan.  ax / ay: alignment class of x / dy.
static int wgrad_plan_checked(const sg_ctx* ctx, int dtype, const sg_conv_desc* d, int ax, int ay, bool planes, const char* who, WgradPlan* pl) {
  SG_CHECK_ARG(ctx != nullptr, "%s: null ctx", who);
  SG_CHECK_ARG(dt_ok(dtype), "%s: dtype %d", who, dtype);
  int rc = check_desc(d, who);
  if (rc) return rc;
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  SG_CHECK_ARG(!head32 || (b16 && d->Cout <= 4), "%s: SG_HEAD_F32 needs Cout <= 4 (a softmax head) on bf16 storage", who);
  SG_CHECK_ARG(!planes || (dtype == SG_F32 && ax == 16 && ay == 16), "%s: null / unaligned tensor", who);
  *pl = plan_wgrad(ctx->num_cus, dtype, d, ax, ay, planes);
  if (planes && !pl->main.family) {
    sg_set_error("%s: geometry outside the planes-in kernel (stride 1 SAME, W %% 32 = 0, channels %% 8 = 0, dense "
                 "planes below 2 GiB, not a wide pointwise / patch-form layer, x6 arithmetic)", who);
    return SG_EUNSUPPORTED;
  }
  SG_CHECK_ARG(!(head32 && pl->chunks > 1), "%s: softmax head beyond 2 GiB", who);
  return 0;
}

int sg_conv2d_wgrad_plan(const sg_ctx* ctx, int dtype, const sg_conv_desc* d, int aligned, int planes, sg_wgrad_plan* out) {
  SG_CHECK_ARG(out != nullptr, "sg_conv2d_wgrad_plan: null out");
  memset(out, 0, sizeof(*out));
  SG_CHECK_ARG(aligned == 16 || aligned == 8 || aligned == 0, "sg_conv2d_wgrad_plan: aligned %d (16, 8 or 0)", aligned);
  WgradPlan pl;
  const int rc = wgrad_plan_checked(ctx, dtype, d, aligned, aligned, planes != 0, planes ? "sg_conv2d_wgrad_planes" : "sg_conv2d_wgrad", &pl);
  if (!rc) *out = pl;
  return rc;
}

// The storage-blind query: the larger of the fp32 and the bf16 plan at full alignment.  No plan of another alignment class needs
// more: an unaligned thin layer writes dw directly (no partials), and the wide pointwise and patch fallbacks cut their slabs into
// at most the aligned plan's share count (plan_wgrad_launch: S <= S0), so their partial slabs fit the aligned plan's.
size_t sg_conv2d_wgrad_ws_bytes(const sg_ctx* ctx, const sg_conv_desc* d) {
  if (!ctx || !d) return 0;
  const size_t a = plan_wgrad(ctx->num_cus, SG_F32, d, 16, 16, false).ws_bytes, b = plan_wgrad(ctx->num_cus, SG_BF16, d, 16, 16, false).ws_bytes;
  return a > b ? a : b;
}

size_t sg_conv2d_wgrad_planes_ws_bytes(const sg_ctx* ctx, const sg_conv_desc* d) {
  if (!ctx || !d || check_desc(d, "sg_conv2d_wgrad_planes_ws_bytes")) return 0;
  const WgradPlan pl = plan_wgrad(ctx->num_cus, SG_F32, d, 16, 16, true);
  return pl.main.family ? pl.ws_bytes : 0;
}

// WgradParams of one launch of the plan: `dd` = its images, `out` = where its first partial slab (or dw itself) goes
static void fill_wgrad_params(WgradParams& p, int dtype, const sg_conv_desc& dd, const WgradLaunch& f, const void* xs, const void* dys,
                              float* out, const sg_bn_in* bn) {
  p.x = (const float*)xs;
  p.dy = (const float*)dys;
  p.out = out;
  p.H = dd.H; p.W = dd.W; p.Cin = dd.Cin; p.x_ld = dd.x_ld ? dd.x_ld : dd.Cin;
  p.OH = dd.Ho; p.OW = dd.Wo; p.Cout = dd.Cout; p.y_ld = dd.y_ld ? dd.y_ld : dd.Cout;
  p.stride = dd.stride; p.dil = dd.dilation; p.pad_t = dd.pad_t; p.pad_l = dd.pad_l;
  p.K = dd.KH * dd.KW * dd.Cin;
  p.KH_KW = dd.KH * dd.KW;
  p.P = dd.N * dd.Ho * dd.Wo;
  p.slabs_per_split = f.steps;
  p.skip_slabs = f.skip_slabs;
  p.tap_inner = f.tap_inner;
  p.stagger = f.stagger;
  p.up = (dtype & SG_X_UP2) ? 1 : 0;
  p.bn = bn_in_of(bn);
  p.fd_ohow = make_fastdiv((uint32_t)(dd.Ho * dd.Wo));
  p.fd_ow = make_fastdiv((uint32_t)dd.Wo);
  p.fd_c = make_fastdiv((uint32_t)dd.Cin);
  p.fd_kw = make_fastdiv((uint32_t)dd.KW);
  p.fd_oh = make_fastdiv((uint32_t)dd.Ho);
  if (f.family == SG_WG_PLANES) {   // x / dy = three dense bf16 planes each; the extents cover all three
    p.x_plane_bytes = (uint32_t)((int64_t)dd.N * dd.H * dd.W * dd.Cin * 2);
    p.dy_plane_bytes = (uint32_t)((int64_t)p.P * dd.Cout * 2);
    p.x_bytes = 3 * p.x_plane_bytes;
    p.dy_bytes = 3 * p.dy_plane_bytes;
  } else {
    p.x_plane_bytes = p.dy_plane_bytes = 0;
    wgrad_extents(dtype, &dd, p.x_bytes, p.dy_bytes);
  }
}

// the template instantiation the plan names, for the three tile widths
#define WG_TILE(FN, ...)                                                             \
  (f.bn == 128 ? FN<128, 2, 4, __VA_ARGS__>(p, f.S, st)                             \
               : f.bn == 64 ? FN<64, 4, 2, __VA_ARGS__>(p, f.S, st) : FN<32, 4, 1, __VA_ARGS__>(p, f.S, st))

static int launch_wgrad_plan(sg_ctx* ctx, hipStream_t st, int dtype, const sg_conv_desc& dd, const WgradLaunch& f, const WgradParams& p,
                             void* ws, const sg_bn_in* bn) {
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0;
  const sg_conv_desc* d = &dd;
  switch (f.family) {
    case SG_WG_THIN:   // (only the fp32 kernel applies a BatchNormalization)
      return launch_thin_wgrad(ctx->num_cus, d, b16, b16 && !head32, p.x, p.dy, p.out, (float*)ws, st, b16 ? bn_in_none() : p.bn);
    case SG_WG_WIDE:
      return b16 ? launch_wgrad_pw_wide_b16(p, f.S, st) : launch_wgrad_pw_wide(p, f.S, st);
    case SG_WG_PATCH:
      return launch_x6wp(p, f.S, b16, f.planes, st);
    case SG_WG_SLAB_X6:
      if (b16) return WG_TILE(launch_wgrad_x6, 1, 1, bf16_t);
      return f.planes == 1 ? WG_TILE(launch_wgrad_x6, 1, 1, float) : WG_TILE(launch_wgrad_x6, 1);
    case SG_WG_PLANES:
      // Single LDS buffer, two workgroups per CU, the fp32-operand kernel's structure.  Measured (scripts/wgrad_planes_bench.py, fourteen
      // long-K shapes): 7301 us against 8485 for the fp32-operand kernel; a double-buffered woven form took 7577 and four waves of 64 x 64
      // per tile changed nothing - the read + MFMA loop itself takes 640 of the 810 us of the ASPP launch either way.  Both are gone
      // (retired).
      return WG_TILE(launch_wgrad_x6, 1, 3, bf16_t, true);
    case SG_WG_HEAD32:
      return launch_wgrad_native(p, f.bn, f.S, true, false, f.vec != 0, 0, st);
    case SG_WG_SLAB_NATIVE:
      return launch_wgrad_native(p, f.bn, f.S, b16, b16, f.vec != 0, f.fast, st);
  }
  sg_set_error("filter gradient: plan without a family");
  return SG_EINVAL;
}
#undef WG_TILE

// Runs a checked plan: every sub-batch's launch, the fixed-order reduce of the partial slabs, the bias gradient.
static int run_wgrad(sg_ctx* ctx, hipStream_t st, int dtype, const sg_conv_desc* d, const WgradPlan& pl, const void* x, const void* dy,
                     void* dw, void* dbias, void* ws, const sg_bn_in* bn) {
  const bool b16 = dt_storage(dtype) == SG_BF16, head32 = (dtype & SG_HEAD_F32) != 0, up2 = (dtype & SG_X_UP2) != 0;
  const int eb = dt_bytes(dtype);
  const int64_t xl = d->x_ld ? d->x_ld : d->Cin, yl = d->y_ld ? d->y_ld : d->Cout;
  const int64_t slab = (int64_t)d->KH * d->KW * d->Cin * d->Cout;
  // sub-batches of whole images, each writing its partial slabs one after the other; one reduce over all of them.  (Where the plan
  // names a vector form, the pixel strides are multiples of that vector, so every sub-batch's operands keep the call's alignment.)
  int parts = 0;
  for (int c = 0; c < pl.chunks; ++c) {
    const WgradLaunch& f = c + 1 < pl.chunks ? pl.main : pl.tail;
    sg_conv_desc sub = *d;
    const int n0 = c * pl.nb;
    sub.N = c + 1 < pl.chunks ? pl.nb : pl.tail_n;
    WgradParams p;
    fill_wgrad_params(p, dtype, sub, f, (const char*)x + (int64_t)n0 * (up2 ? (d->H / 2) * (d->W / 2) : d->H * d->W) * xl * eb,
                      (const char*)dy + (int64_t)n0 * d->Ho * d->Wo * yl * eb,
                      pl.max_parts > 1 ? (float*)ws + (int64_t)parts * slab : (float*)dw, bn);
    const int rc = launch_wgrad_plan(ctx, st, dtype, sub, f, p, ws, bn);
    if (rc) return rc;
    parts += f.S;
  }
  if (parts > 1) {
    const bool v4 = (slab % 4 == 0) && aligned16(ws) && aligned16(dw);
    const int rc = launch_reduce_splits((const float*)ws, (float*)dw, slab, parts, v4, st);
    if (rc) return rc;
  }
  if (!dbias) return 0;
  const int64_t rows_y = (int64_t)d->N * d->Ho * d->Wo;
  float* bias_part = (float*)((char*)ws + pl.bias_off);
  return launch_colsum(ctx->num_cus, b16 && !head32, dy, rows_y, d->Cout, (int)yl, (float*)dbias, bias_part, st);
}

int sg_conv2d_wgrad(sg_ctx* ctx, void* stream, int dtype, const sg_conv_desc* d, const void* x, const void* dy,
                    void* dw, void* dbias, const sg_conv_opts* opts) {
  const sg_conv_opts& o = opts ? *opts : kNoOpts;
  const sg_bn_in* const bn = o.bn_in;
  SG_CHECK_ARG(!o.stats && !o.tiles_out && !o.a_planes && !o.res && !o.bnb,
               "sg_conv2d_wgrad: stats / tiles_out / a_planes / res / bnb are operands of the forward and the input gradient");
  SG_CHECK_ARG(!bn || (bn->mean && bn->invstd && bn->gamma && bn->beta), "sg_conv2d_wgrad: bn_in with null BatchNormalization parameters");
  WgradPlan pl;
  // (dy of the softmax head is fp32: its 4-channel loads need 16 bytes, which the plan asks of that class itself)
  int rc = wgrad_plan_checked(ctx, dtype, d, align_class(x), align_class(dy), false, "sg_conv2d_wgrad", &pl);
  if (rc) return rc;
  SG_CHECK_ARG(x && dy && dw, "sg_conv2d_wgrad: null tensor");
  if (bn && !pl.bn_in) {
    sg_set_error("sg_conv2d_wgrad: bn_in, but this launch takes neither the thin 1x1 nor the patch filter-gradient kernel (fp32 "
                 "storage, 16-byte aligned operands below 2 GiB)");
    return SG_EUNSUPPORTED;
  }
  if ((dtype & SG_X_UP2) && !pl.up2) {
    // x = the source of a 2x nearest up-sampling: only the patch kernel gathers that way (conv_x6wp.h)
    sg_set_error("sg_conv2d_wgrad: SG_X_UP2 on a launch the patch filter-gradient kernel does not cover");
    return SG_EUNSUPPORTED;
  }
  if (!o.ws || o.ws_bytes < pl.ws_bytes) {
    sg_set_error("sg_conv2d_wgrad: workspace %zu < %zu", o.ws_bytes, (size_t)pl.ws_bytes);
    return SG_EWORKSPACE;
  }
  SG_CHECK_ARG(aligned16(o.ws), "sg_conv2d_wgrad: workspace must be 16-byte aligned");
  return run_wgrad(ctx, (hipStream_t)stream, dtype, d, pl, x, dy, dw, dbias, o.ws, bn);
}

// ---- planes-in filter gradient (round 5; conv_x6.h: wgrad_x6_kernel<.., PIN>) -------------------------------------------
int sg_split_planes(sg_ctx* ctx, void* stream, const void* x, int64_t rows, int C, int ld, void* planes) {
  SG_CHECK_ARG(ctx && x && planes && rows > 0 && C > 0, "sg_split_planes: bad argument");
  const int xl = ld ? ld : C;
  SG_CHECK_ARG((C % 4 == 0) && (xl % 4 == 0) && xl >= C && aligned16(x) && aligned16(planes), "sg_split_planes: C and ld must be multiples of 4, pointers 16-byte aligned");
  int64_t blocks = sg_cdiv(rows * (C / 4), 256);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(x6w_split_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)x, (unsigned short*)planes, rows, C, xl);
  SG_LAUNCH_CHECK("x6w_split_kernel");
  return 0;
}

int sg_conv2d_wgrad_planes(sg_ctx* ctx, void* stream, const sg_conv_desc* d, const void* x_planes, const void* dy_planes, void* dw,
                           void* ws, size_t ws_bytes) {
  WgradPlan pl;
  const int ok = x_planes && dy_planes && dw;   // (a null tensor answers like an unaligned one)
  int rc = wgrad_plan_checked(ctx, SG_F32, d, ok ? align_class(x_planes) : 0, ok ? align_class(dy_planes) : 0, true, "sg_conv2d_wgrad_planes", &pl);
  if (rc) return rc;
  if (!ws || ws_bytes < pl.ws_bytes || !aligned16(ws)) {
    sg_set_error("sg_conv2d_wgrad_planes: workspace %zu < %zu", ws_bytes, (size_t)pl.ws_bytes);
    return SG_EWORKSPACE;
  }
  return run_wgrad(ctx, (hipStream_t)stream, SG_F32, d, pl, x_planes, dy_planes, dw, nullptr, ws, nullptr);
}

// what the launches of `d` can take: every answer from the plans they run by
int sg_conv2d_caps(const sg_ctx* ctx, int dtype, const sg_conv_desc* d, int dgrad, sg_conv_caps* out) {
  SG_CHECK_ARG(ctx && d && out && dt_ok(dtype), "sg_conv2d_caps: bad argument");
  memset(out, 0, sizeof(*out));
  if (check_desc(d, "sg_conv2d_caps")) return 0;   // a descriptor no launch takes: no option either (the launch says why)
  ConvPlan pl = plan_conv(ctx->num_cus, dtype, d, dgrad != 0, 0);
  // (aligned pointers assumed; a thin launch in sub-batches whose images are no multiple of 16 bytes leaves the family for any pointer)
  if (pl.family == CONV_THIN && !thin_operands_ok(pl, d, true, (dtype & SG_HEAD_F32) ? 2 : dt_bytes(dtype)))
    pl = plan_conv(ctx->num_cus, dtype, d, dgrad != 0, PLAN_NOT_THIN);
  out->thin = pl.family == CONV_THIN;
  out->planes_in = pl.planes_in;
  // (the filter gradient has no direction)
  out->wgrad_planes = dt_storage(dtype) == SG_F32 && plan_wgrad(ctx->num_cus, SG_F32, d, 16, 16, true).main.family != 0;
  if (dgrad) {
    out->bnb = pl.bnb;
  } else if (pl.bn_in || pl.up2) {   // forward AND filter gradient must both take the fused operand
    const WgradPlan wp = plan_wgrad(ctx->num_cus, dtype, d, 16, 16, false);
    out->bn_in = wp.bn_in;
    out->up2 = pl.up2 && wp.up2;
  }
  return 0;
}

size_t sg_bias_grad_ws_bytes(const sg_ctx* ctx, int64_t rows, int C) {
  if (!ctx) return 0;
  return colsum_ws_bytes(ctx->num_cus, rows, C) + 256;
}

int sg_bias_grad(sg_ctx* ctx, void* stream, int dtype, int64_t rows, int C, int ld, const void* dy, void* dbias,
                 void* ws, size_t ws_bytes) {
  SG_CHECK_ARG(ctx && (dtype == SG_F32 || dtype == SG_BF16) && dy && dbias && rows > 0 && C > 0, "sg_bias_grad: bad argument");
  if (ld == 0) ld = C;
  SG_CHECK_ARG(ld >= C, "sg_bias_grad: ld < C");
  const size_t need = colsum_ws_bytes(ctx->num_cus, rows, C);
  if (!ws || ws_bytes < need) {
    sg_set_error("sg_bias_grad: workspace %zu < %zu", ws_bytes, need);
    return SG_EWORKSPACE;
  }
  return launch_colsum(ctx->num_cus, dtype == SG_BF16, dy, rows, C, ld, (float*)dbias, (float*)ws, (hipStream_t)stream);
}

int sg_dense_fwd(sg_ctx* ctx, void* stream, int dtype, int rows, int in, int out, const void* x, const void* w,
                 const void* bias, void* y, int flags) {
  sg_conv_desc d = {};
  d.N = rows; d.H = 1; d.W = 1; d.Cin = in; d.Cout = out; d.KH = 1; d.KW = 1; d.stride = 1; d.dilation = 1;
  d.Ho = 1; d.Wo = 1;
  return sg_conv2d_fwd(ctx, stream, dtype, &d, x, w, bias, y, flags, nullptr);
}

}  // extern "C"
