// "Patch" form of the x6 convolution for 3x3, stride 1, dilation 1, "same" convolutions with 32 or 64 reduction channels per tap
// (and more, in chunks of 64), and the fused up-sampling forms on top of it: what the plan asks of the family, and its launch
// functions.  The kernels and their description: conv_x6p.hip.
#pragma once
#include "conv_common.h"

namespace sgconv {

inline bool x6p_enabled() {
  return !sg_switch<SW_X6_NOPATCH>();
}

// geometry the patch form covers; KH, KW are the filter's (IgemmParams carries only K).  Geometry fields only: plan_conv, the
// one caller, has the 16-byte channel runs from x6_ok's `vec` and keeps the launches of the planes-in kernel (K >= 2048 and >= 192
// output columns: conv_x6w.h) off this form
inline bool x6p_geom(const IgemmParams& p, int KH, int KW) {
  if (!x6p_enabled() || KH != 3 || KW != 3) return false;
  // 32 or 64 reduction channels per tap in one patch; 128 / 256 / ... in chunks of 64 (round 5)
  if (p.K != 9 * p.C) return false;
  if (!(p.C == 32 || p.C == 64)) {
    if (!sg_switch<SW_X6P_CHUNKS>() || p.C % 64 != 0 || p.C > 512) return false;
  }
  if (p.a_mul != 1 || p.div != 1) return false;
  const bool fwd = p.k_mul == 1 && p.off_h == -1 && p.off_w == -1, bwd = p.k_mul == -1 && p.off_h == 1 && p.off_w == 1;
  if (!fwd && !bwd) return false;
  if (p.OH != p.H || p.OW != p.W || (p.H % 8) || (p.W % 16)) return false;
  return p.Nout == 32 || p.Nout == 64 || p.Nout % 128 == 0;
}

// the patch kernel's tile width for N output columns (run_x6p and the plan query, sg_conv2d_plan); its <C, MULTI> follow from the
// tap depth alone: 32 -> <32>, 64 -> <64>, more -> <64, MULTI> (chunks of 64)
inline int x6p_bn_of(int N) { return N >= 128 ? 128 : N; }
inline int x6p_c_of(int C) { return C == 32 ? 32 : 64; }
inline bool x6p_multi_of(int C) { return C > 64; }

// ---- UpSampling2D(2) -> Conv2D 3x3: which launches take the fused kernels (sg_conv2d_fwd* with SG_PRO_UP2, sg_conv2d_dgrad with
// SG_EPI_DOWN2).  `d` describes the convolution on the UP-SAMPLED grid (H x W = twice the source's).
inline bool x6p_up2_geom(const sg_conv_desc* d) {
  if (!x6p_enabled() || d->KH != 3 || d->KW != 3 || d->stride != 1 || d->dilation != 1) return false;
  if (d->pad_t != 1 || d->pad_l != 1 || d->Ho != d->H || d->Wo != d->W) return false;
  if (d->Cin != 64 || d->Cout != 32) return false;
  if ((d->H % 16) || (d->W % 32)) return false;   // 8 x 16 SOURCE tiles (forward), 8 x 16 output tiles (dgrad)
  return true;
}

inline size_t x6p_up2_ws_bytes() { return (size_t)16 * 4 * 3 * 512 * 2; }   // 16 k-steps x 4 phases x 3 planes x 1 KB

// split the weights fragment-major (in `ws`, x6_planes_bytes() is enough; prepared: `ws` already holds them) and run the patch
// kernel in the form x6p_bn_of / x6p_c_of / x6p_multi_of name
int run_x6p(IgemmParams& p, const float* w, bool dgrad, int Cin, int Cout, void* ws, int num_cus, hipStream_t st, bool prepared = false);
// every weight of a model in one launch (sg_prepare_planes): planes of all three kinds, sg_planes_job by sg_planes_job
int launch_prepare_planes(const float* w_arena, char* planes_arena, const sg_planes_job* jobs_dev, int njobs, int total_blocks,
                          hipStream_t st);
// the sub-pixel forward: p describes the convolution on the SOURCE grid (H, W, OH, OW, M = source; Nout = 128 = 4 phases x 32)
int run_x6p_up2(IgemmParams& p, const float* w, void* ws, int num_cus, hipStream_t st);

}  // namespace sgconv
