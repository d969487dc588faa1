// What every convolution file shares: the tile constants, the kernels' parameter structs, the few device helpers more than one
// kernel family uses, the planning helpers every launch comes through, ConvPlan and the filter gradient's plan types.
//
// Types that cross a translation-unit boundary live in namespace sgconv; kernels and file-local helpers stay in an anonymous
// namespace inside their own unit.  A kernel family that is a unit of its own (today: native, thin and patch - conv_native.hip, conv_thin.hip, conv_x6p.hip) has
//   conv_<family>.h    its geometry constants, the host predicates the plan and the plan queries ask, and the declarations of its
//                      launch functions: plain host functions with run-time arguments (which template form a launch takes is
//                      decided behind them, in the family's unit)
//   conv_<family>.hip  its kernels, their launch templates and the switch that picks a form
// The other families' headers are still included by conv_igemm.hip inside its anonymous namespace.
#pragma once
#include "sg_common.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>

namespace sgconv {

constexpr int BM = 128;
constexpr int BK = 32;
constexpr int LDA = BK + 4;  // floats; 144-byte rows

template <int V>
using IC = std::integral_constant<int, V>;

// A BatchNormalization (+ReLU) applied to the convolution's INPUT while it is loaded (round 5: sg_conv_opts.bn_in of
// sg_conv2d_fwd / _wgrad; the patch kernels and the thin 1x1 kernels): y = [relu](fmaf((x - mean) * invstd, gamma, beta)), bn_apply's own
// expression, on every pixel inside the image (the zero padding stays zero).  mean == nullptr: none.
struct BnIn {
  const float* mean;
  const float* invstd;   // infer: the moving variance, invstd = rsqrtf(var + eps)
  const float* gamma;
  const float* beta;
  int relu, infer;
  float eps;
};
__device__ __forceinline__ f32x4 bn_in_inv(const BnIn& b, int c) {
  f32x4 is = *reinterpret_cast<const f32x4*>(b.invstd + c);
  if (b.infer) {
#pragma unroll
    for (int k = 0; k < 4; ++k) is[k] = rsqrtf(is[k] + b.eps);
  }
  return is;
}
__device__ __forceinline__ float bn_in_one(float x, float m, float is, float g, float bt, int relu) {
  const float t = fmaf((x - m) * is, g, bt);
  return relu ? fmaxf(t, 0.f) : t;
}

// pw_wide_kernel<3, float, BN, true> (conv_pw.h): the BatchNormalization backward apply evaluated in the dgrad's A path
struct BnBwdIn {
  const float* x;        // the BatchNormalization's raw input (= the pointwise convolution's forward output), same layout as dy
  const float* mean;
  const float* invstd;
  const float* gamma;
  const float* beta;     // null: no fused ReLU
  const float* dgamma;   // finished column sums
  const float* dbeta;
  float* dz;             // out: the applied gradient (for the filter gradient)
  int relu;
  float inv_n;
};

struct IgemmParams {
  const float* __restrict__ x;
  const float* __restrict__ w;
  const float* __restrict__ bias;
  float* __restrict__ y;
  int H, W, C, x_ld;
  int OH, OW;
  int Nout, y_ld;
  int a_mul, k_mul, off_h, off_w, div;
  int K, M;
  int flags;
  int stagger;  // waves in the upper half of the workgroup issue their gathers AFTER their MFMAs
  int ablate;   // timing-only diagnostics (results wrong): 1 = no global loads in the loop, 2 = no LDS store/barrier
  uint32_t x_bytes, w_bytes;  // extents for the buffer descriptors of the UT path (both < 2^31)
  int skip_taps;              // drop taps that are pure padding for the whole tile (dilated convs)
  int group_m;                // > 1: tiles are walked in groups of group_m row tiles, row tile fastest (L2 reuse of B)
  int cb;                     // > 0: K order = (channel block of cb slabs) x tap x slab, so the 9 taps of a
                              //      channel block re-read x from L2 instead of the fabric; 0: tap-major
  FastDiv fd_ohow, fd_ow, fd_c, fd_kw;
  // x6 path (conv_x6.h): the weights as three bf16 planes [3][Npad][Kpad]; w_bytes then is their extent
  const unsigned short* __restrict__ wq;
  int Kpad, Npad;
  int kd;  // k-block depth of the plane layout [npl][Kpad / kd][Npad][kd] (= the kernel's slab depth); 0: rows [npl][Npad][Kpad]
  float* __restrict__ stats;  // SG_EPI_BN_STATS: [tiles_m][2][Nout] per-tile (sum, centred sum of squares), else null
  // Stride-2 dgrad (and Conv2DTranspose forward) with rows in PARITY-CLASS order (conv_x6_kernel / conv_b16_kernel only):
  // GEMM row m = ((cls * N + n) * OH/2 + i) * OW/2 + j is output pixel (n, 2i + (cls >> 1), 2j + (cls & 1)).  Of the KH x KW
  // taps only those of matching parity reach a pixel of class cls; in raster order a 128-row tile mixes the column
  // parities, so every tap had a valid row and the tile multiplied all of them (3/4 of the products masked to zero).
  // Class-pure tiles let the existing padding-tap elimination drop the taps of the other parities: a 3x3 kernel runs 1 / 2 /
  // 2 / 4 taps instead of 9 four times, a 1x1 kernel one tap for a quarter of the tiles and none for the rest.
  int perm2;
  FastDiv fd_mc, fd_hcwc, fd_wc;
  // dgrad: a gradient already collected for the same tensor (y's layout, may be y itself), added in the epilogue
  // (sg_conv_opts.res; conv_x6_kernel / conv_b16_kernel only)
  const float* res;
  // the A operand already split into three bf16 planes [3][pixels][C] (sg_split_planes; sg_conv_opts.a_planes): the
  // planes-in kernel (conv_x6w.h) reads them instead of splitting x itself; ignored by every other kernel; null: none
  const unsigned short* a_planes;
  BnIn bn;   // conv_x6p_kernel only: the BatchNormalization applied in the patch loader (mean == nullptr: none)
  BnBwdIn bnb;   // pw_wide_kernel<.., BNB> only (x == nullptr: none)
};

__device__ __forceinline__ int spt_of(const IgemmParams& p) { return p.C / BK; }  // slabs per tap (UT)

// GEMM row -> output pixel coordinates (image, row, column); see IgemmParams::perm2
__device__ __forceinline__ void row_to_pixel(const IgemmParams& p, uint32_t m, uint32_t& n, uint32_t& oh, uint32_t& ow) {
  if (p.perm2) {
    uint32_t cls, r, rem, i, j;
    fd_divmod(m, p.fd_mc, cls, r);
    fd_divmod(r, p.fd_hcwc, n, rem);
    fd_divmod(rem, p.fd_wc, i, j);
    oh = 2 * i + (cls >> 1);
    ow = 2 * j + (cls & 1);
  } else {
    uint32_t rem;
    fd_divmod(m, p.fd_ohow, n, rem);
    fd_divmod(rem, p.fd_ow, oh, ow);
  }
}
// element offset of GEMM row `row` in y
__device__ __forceinline__ int64_t row_to_yoff(const IgemmParams& p, int row) {
  if (!p.perm2) return (int64_t)row * p.y_ld;
  uint32_t n, oh, ow;
  row_to_pixel(p, (uint32_t)row, n, oh, ow);
  return ((int64_t)(n * p.OH + oh) * p.OW + ow) * p.y_ld;
}

// ---- the filter gradient's kernels ----------------------------------------------------------------------
struct WgradParams {
  const float* __restrict__ x;
  const float* __restrict__ dy;
  float* __restrict__ out;  // [S][K][Cout] partials (or dw itself when S == 1)
  int H, W, Cin, x_ld;
  int OH, OW, Cout, y_ld;
  int stride, dil, pad_t, pad_l;
  int K, P;
  int slabs_per_split;
  int stagger;
  uint32_t x_bytes, dy_bytes;  // extents for the buffer descriptors of the FAST path (both < 2^31)
  int skip_slabs;              // drop 32-pixel slabs that are pure padding for every tap of the tile (dilated convs)
  int KH_KW;
  int tap_inner;               // tile order (channel block, tap, column tile) instead of (tap, channel block, column tile)
  uint32_t x_plane_bytes, dy_plane_bytes;   // planes-in filter gradient (wgrad_x6_kernel<.., PIN>): bytes from one bf16 plane of
                               //    x / dy to the next; x_bytes / dy_bytes then cover all three
  BnIn bn;                     // wgrad_x6wp_kernel only: the BatchNormalization applied to x in the patch loader (mean == nullptr: none)
  int up;                      // 1: x is the source of a nearest 2x up-sampling (SG_X_UP2; wgrad_x6wp_kernel only): pixel (h, w)
                               //    of the H x W tensor is x[n, h >> 1, w >> 1, :] of the (H / 2) x (W / 2) source
  FastDiv fd_ohow, fd_ow, fd_c, fd_kw, fd_oh;
};

// ---- device helpers that more than one kernel family uses ----------------------------------------------------------------------
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

// (x0, x1) -> three packed bf16 pairs (element 0 in the low half), x = h + m + l up to 2^-25 |x|
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  f32x2_t v = {x0, x1};
  h = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
  f32x2_t hf = {__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};
  f32x2_t r = v - hf;
  m = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2_t));
  f32x2_t mf = {__uint_as_float(m << 16), __uint_as_float(m & 0xffff0000u)};
  f32x2_t s = r - mf;
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(s, bf16x2_t));
}

typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr;

__device__ __forceinline__ bf16x8_t tr_frag(const char* lds_addr_a, const char* lds_addr_b) {
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lds_addr_a));
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lds_addr_b));
  typedef short s16x8_t __attribute__((ext_vector_type(8)));
  const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}

__device__ __forceinline__ void pw_lds_dma16(const __amdgpu_buffer_rsrc_t rsrc, char* lds_wave_base, unsigned voff, int soff) {
  // 64 lanes x 16 bytes -> lds_wave_base + 16 * lane (the LDS address is wave-uniform: M0); out-of-range lanes write zeros
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (void __attribute__((address_space(3)))*)lds_wave_base, 16, (int)voff, soff, 0, 0);
}

template <typename KernelT>
int set_dyn_lds(KernelT k, size_t bytes) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    sg_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize=%zu): %s", bytes, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// x6 == true: the switches as the x6 kernels use them.  Re-measured with those kernels (profiles/r01_ab_l2_orders.txt,
// second part): the grouped order takes the ASPP dgrad fetch from 1998 to 485 MiB and the tap-inner wgrad order from
// 795 to 279 MiB at 0-3 % of kernel time (the fp32 kernels paid 6-13 %), so both are on there: default 7.
inline int conv_l2(bool x6 = false) {
  if (sg_switch_set<SW_CONV_L2>()) return sg_switch<SW_CONV_L2>() & 7;
  if (x6) return 7;
  // the fp32 kernels, default 2: measured on the ASPP convs (scripts/ab_l2.sh, 30 iterations, two interleaved rounds):
  //   bit 1 (channel-block K order): forward fetch 1039 -> 451 MiB per launch, time unchanged      -> on
  //   bit 0 (grouped tile order):    dgrad fetch 1808 -> 461 MiB, but 6-13 % SLOWER               -> off
  //   bit 2 (wgrad tap-inner order): wgrad fetch 1018 -> 314 MiB, but 2-8 % SLOWER                 -> off
  // The re-reads are served by the 256 MiB Infinity Cache (operands total < 150 MiB), not by HBM, and the
  // orders that remove them make many CUs hit the same L2 lines at the same time.
  return 2;
}

// Tile width by wave quantisation: two workgroups fit a CU (LDS), so one "wave" of the grid is 2*CUs tiles; pick
// the BN in {128, 64} whose tile count wastes the least of its last wave and of its last column tile (e.g.
// M = 16384, N = 728: 128-wide = 768 tiles = 1.5 waves (75 %), 64-wide = 1536 tiles = 3.0 waves (100 %)).
inline int pick_bn(int64_t M, int N, int num_cus) {
  if (N <= 32) return 32;
  if (N <= 64) return 64;
  // quantum = one workgroup per CU: an 8-wave workgroup keeps a CU's matrix pipes fed on its own, and tiles
  // beyond the resident ones are dispatched as CUs free up, so the makespan is ceil(tiles / CUs) tile-times
  const int64_t slots = (int64_t)num_cus;
  double best = -1.0;
  int best_bn = 128;
  for (int bn : {128, 64}) {
    const int64_t tiles = sg_cdiv(M, BM) * sg_cdiv(N, bn);
    const double eff = (double)tiles / (double)(sg_cdiv(tiles, slots) * slots) * (double)N / (double)(sg_cdiv(N, bn) * bn) *
                       (bn == 128 ? 1.0 : 0.93);  // the wider tile re-reads A half as often
    if (eff > best) { best = eff; best_bn = bn; }
  }
  return best_bn;
}

// fields shared by the fp32 and the x6 kernel: padding-tap elimination, tile order, K order
inline void plan_common(IgemmParams& p, bool vec, int bn, bool x6 = false, int eb = 4) {
  const int noskip = sg_switch<SW_CONV_NOSKIP>();  // A/B switch for the padding-tap elimination
  const int ntaps = p.K / p.C, spt = p.C / BK;
  p.skip_taps = (!noskip && (p.k_mul > 1 || p.k_mul < -1) && ntaps > 1 && ntaps <= 64) ? 1 : 0;
  if (p.perm2) p.skip_taps = 1;  // parity-pure tiles: taps of the other parities have no valid row (also a lone 1x1 tap)
  // L2 locality (A/B switch SG_CONV_L2: bit 0 grouped tile order, bit 1 channel-block K order, bit 2 wgrad order).
  // An XCD owns 1/8 of the tiles and with them about 1/8 of the A operand's pixels.
  const int64_t ntn = sg_cdiv(p.Nout, bn);
  const int64_t a_per_xcd = p.x_bytes ? (int64_t)p.x_bytes / 8 : (1ll << 40);
  p.group_m = ((conv_l2(x6) & 1) && ntn >= 4) ? (a_per_xcd <= (2ll << 20) ? 16 : 8) : 1;
  const int gm_force = sg_switch<SW_CONV_GM>();   // experiment: row tiles per group
  if (gm_force > 0 && ntn >= 2) p.group_m = gm_force;
  const bool ut = vec && (p.C % BK == 0) && p.x_bytes != 0 && p.w_bytes != 0;
  // decided from ONE image's footprint, never from the batch: the K order fixes the rounding order, and
  // inference must not depend on how many tiles travel together (tests/test_fullsize_gpu.py)
  const int64_t img_bytes = (int64_t)p.H * p.W * p.x_ld * eb;
  const int cbv = sg_switch<SW_CONV_CB>();  // experiment switch: slabs per channel block of the K order (default 4)
  p.cb = ((conv_l2(x6) & 2) && ut && ntaps > 1 && spt > cbv && spt % cbv == 0 && img_bytes > (2ll << 20)) ? cbv : 0;
}

// The kernels of the slab family (plan_conv: CONV_SLAB) and what every one of their launches sets before it starts: the tile width
// (the two 256-wide forms plan with 128-wide column tiles, the others by wave quantisation) and plan_common's fields.  The
// dispatchers, run_x6 and the plan query (sg_conv2d_plan) all come through here; slab_kernel_of (behind ConvPlan) picks the kernel.
enum SlabKernel { SLAB_X6, SLAB_B16, SLAB_X6W, SLAB_B16W };
inline int slab_common(IgemmParams& p, SlabKernel sk, int eb, int num_cus) {
  const int bn = (sk == SLAB_X6W || sk == SLAB_B16W) ? 128 : pick_bn(p.M, p.Nout, num_cus);
  plan_common(p, true, bn, true, eb);
  return bn;
}
// the mixed-storage forms of the native kernel (bf16 storage, the softmax head): scalar-gather planning whatever the loads, no tap
// elimination, no K order, never the wave-uniform-tap form.  dispatch_igemm_mixed and the plan query both come through here.
inline int mixed_common(IgemmParams& p, int num_cus) {
  const int bn = pick_bn(p.M, p.Nout, num_cus);
  plan_common(p, false, bn);
  p.stagger = 0;
  p.ablate = 0;
  p.skip_taps = 0;
  p.cb = 0;
  return bn;
}
// the fp32 native kernel: planning by its channel runs; the UT form is launch_igemm's (igemm_ut_of)
inline int native_common(IgemmParams& p, bool vec, int num_cus) {
  const int bn = pick_bn(p.M, p.Nout, num_cus);
  plan_common(p, vec, bn);
  return bn;
}

// ---- the plan of a forward convolution or an input gradient (plan_conv, conv_igemm.hip) ----
enum ConvFamily {   // (from CONV_SLAB on: the kernels that read prepared weight planes, sg_planes_job.kind 1 / 2 / 3)
  CONV_NATIVE,   // the fp32-MFMA kernels: any shape, any alignment
  CONV_THIN,     // 1x1 with at most 4 output channels: the streaming kernels
  CONV_HEAD,     // the softmax head of a bf16 model that is not thin: the native kernel on mixed storage types
  CONV_SLAB,     // conv_x6 / conv_b16 and, on the same planes, their wide forms conv_x6w (planes-in) / conv_b16w
  CONV_PATCH,    // conv_x6p
  CONV_WIDE      // conv_pw
};
constexpr int PLAN_NOT_THIN = 1 << 30;   // plan_conv `flags` (no SG_EPI_* / SG_PRO_* bit): the operands of a thin launch missed its alignment

struct ConvPlan {
  ConvFamily family = CONV_NATIVE;
  int nb = 0;         // images per launch: >= N the whole batch; fewer: sub-batches of whole images (2 GiB buffer descriptors),
                      // none of which takes the wide pointwise kernel; 0: one image alone passes the limit (native, whole batch)
  bool vec = false;   // 16-byte channel runs as far as the descriptor says (the launch adds the pointers' alignment)
  int perm2 = 0;      // stride-2 dgrad: rows in parity-class order (IgemmParams::perm2; the slab kernels)
  // the weight planes (family >= CONV_SLAB): sg_planes_job's fields; Ckp = the tap depth after virtual channel padding
  int npl = 0, Ck = 0, Ckp = 0, K = 0, kd = 0, Kpad = 0, Npad = 0, nblocks = 0;
  int wbn = 0;        // CONV_WIDE: tile width, 384 or 256
  size_t w_bytes = 0;
  // CONV_SLAB: K shares of the planes-in kernel / of the 256-wide bf16 kernel (0: conv_x6_kernel / conv_b16_kernel); deep bf16 slabs
  int x6w_S = 0, b16w_S = 0;
  bool deep = false;
  size_t a_img_bytes = 0, part_img_bytes = 0;   // scratch behind the planes per image: activation planes, split-K partial slabs
  // what the family can do
  bool res = false;        // add a collected gradient (sg_conv_opts.res).  Of the plane kernels only the slab family: a launch
                           // with `res` whose plan names a wide slab form takes conv_x6_kernel / conv_b16_kernel on the same planes
  bool bn_in = false;      // apply a BatchNormalization in its loader (thin; patch with 32 / 64 reduction channels per tap)
  bool up2 = false;        // the fused up-sampling forms exist for this layer (SG_PRO_UP2; with CONV_PATCH: SG_EPI_DOWN2)
  bool bnb = false;        // evaluate the BatchNormalization backward in its A path (wide pointwise dgrad)
  bool planes_in = false;  // read the activation as bf16 planes the caller made (sg_split_planes)

  // scratch behind the weight planes of a launch of `images` images
  size_t scratch_bytes(int images) const {
    return (((size_t)images * a_img_bytes + 255) & ~(size_t)255) + (size_t)images * part_img_bytes;
  }
  // the weight planes and that scratch
  size_t ws_bytes(int images) const {
    const size_t sc = scratch_bytes(images);
    return sc ? ((w_bytes + 255) & ~(size_t)255) + sc : w_bytes;
  }
};

// Which kernel a launch of the slab family takes: the planes-in kernel / the 256-wide bf16 kernel where the plan names K shares and
// the launch adds no collected gradient (they have no such epilogue), conv_b16_kernel for deep bf16 slabs, else conv_x6_kernel.
inline SlabKernel slab_kernel_of(const ConvPlan& pl, bool b16, bool with_res) {
  if (pl.npl == 3 && !b16 && pl.x6w_S > 0 && !with_res) return SLAB_X6W;
  if (b16 && pl.deep) return (pl.b16w_S > 0 && !with_res) ? SLAB_B16W : SLAB_B16;
  return SLAB_X6;
}
// A slab launch's parameters from the plan: virtual channel padding, the planes' geometry and bytes
inline void slab_fill(IgemmParams& p, const ConvPlan& pl) {
  if (pl.Ckp != p.C) {   // virtual channel padding
    p.K = pl.K;
    p.C = pl.Ckp;
    p.fd_c = make_fastdiv((uint32_t)pl.Ckp);
  }
  p.kd = pl.kd;
  p.Kpad = pl.Kpad;
  p.Npad = pl.Npad;
  p.w_bytes = (uint32_t)pl.w_bytes;
}

// the filter gradient's plan and the launches it names (include/segengine.h: sg_conv2d_wgrad_plan hands them out); plan_wgrad: conv_igemm.hip
typedef sg_wgrad_launch WgradLaunch;
typedef sg_wgrad_plan WgradPlan;

inline int wgrad_bn(int cout) { return cout > 64 ? 128 : (cout > 32 ? 64 : 32); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int check_desc(const sg_conv_desc* d, const char* who) {
  SG_CHECK_ARG(d != nullptr, "%s: null desc", who);
  SG_CHECK_ARG(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "%s: non-positive dims", who);
  SG_CHECK_ARG(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->dilation > 0, "%s: bad kernel geometry", who);
  SG_CHECK_ARG(d->Ho > 0 && d->Wo > 0, "%s: bad output dims", who);
  SG_CHECK_ARG(d->pad_t >= 0 && d->pad_l >= 0, "%s: negative pad", who);
  // the gather packs a row's scaled (oh, ow) into signed 16-bit halves
  SG_CHECK_ARG(d->H < 8192 && d->W < 8192 && (int64_t)d->Ho * d->stride < 16384 && (int64_t)d->Wo * d->stride < 16384 &&
                   (int64_t)d->KH * d->dilation < 8192 && (int64_t)d->KW * d->dilation < 8192,
               "%s: map or kernel extent beyond the 16-bit coordinate range", who);
  const int xl = d->x_ld ? d->x_ld : d->Cin, yl = d->y_ld ? d->y_ld : d->Cout;
  SG_CHECK_ARG(xl >= d->Cin && yl >= d->Cout, "%s: pixel stride smaller than channel count", who);
  SG_CHECK_ARG((int64_t)d->N * d->H * d->W * xl < (1ll << 31) && (int64_t)d->N * d->Ho * d->Wo * yl < (1ll << 31),
               "%s: tensor exceeds 2^31 elements", who);
  return 0;
}

inline BnIn bn_in_none() {
  BnIn b;
  b.mean = b.invstd = b.gamma = b.beta = nullptr;
  b.relu = b.infer = 0;
  b.eps = 0.f;
  return b;
}
inline BnIn bn_in_of(const sg_bn_in* b) {
  BnIn o = bn_in_none();
  if (b && b->mean) {
    o.mean = (const float*)b->mean; o.invstd = (const float*)b->invstd; o.gamma = (const float*)b->gamma; o.beta = (const float*)b->beta;
    o.relu = b->relu; o.infer = b->infer; o.eps = b->eps;
  }
  return o;
}

// ---- storage-type plumbing of the entry points ---------------------------------------------------------------------
// dtype = SG_F32 or SG_BF16 (activation storage), optionally | SG_HEAD_F32: the few-channel side of a thin 1x1
// convolution (y of the forward, dy of dgrad / wgrad) is fp32 although the activations are bf16 - the softmax head,
// whose logits, probabilities and loss stay in fp32.
inline int dt_storage(int dtype) { return dtype & 0xff; }
inline bool dt_ok(int dtype) {
  const int st = dt_storage(dtype);
  return (st == SG_F32 || st == SG_BF16) && (dtype & ~(0xff | SG_HEAD_F32 | SG_X_UP2)) == 0;
}
inline int dt_bytes(int dtype) { return dt_storage(dtype) == SG_BF16 ? 2 : 4; }

}  // namespace sgconv
