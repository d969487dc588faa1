// "Patch" form of the filter gradient for 3x3, stride 1, dilation 1, "same" convolutions with 32 or 64 channels on both sides:
// what the plan asks of it, and its launch function.  The kernel and its description: conv_x6p.hip.
#pragma once
#include "conv_common.h"

namespace sgconv {

inline bool x6wp_enabled() {
  const bool on = !sg_switch<SW_X6_NOWPATCH>();
  return on;
}

// geometry the patch wgrad covers (descriptor level: the plan and the launch must agree)
inline bool x6wp_geom(const sg_conv_desc* d) {
  if (!x6wp_enabled() || d->KH != 3 || d->KW != 3 || d->stride != 1 || d->dilation != 1) return false;
  if (d->pad_t != 1 || d->pad_l != 1 || d->Ho != d->H || d->Wo != d->W) return false;
  if (!(d->Cin == 32 || d->Cin == 64) || !(d->Cout == 32 || d->Cout == 64)) return false;
  if ((d->H % 4) || (d->W % 16)) return false;
  return true;
}
inline int64_t x6wp_tiles(const sg_conv_desc* d) { return (int64_t)d->N * (d->H / 4) * (d->W / 16); }
// workgroups = partial slabs: two per CU, fewer when there are fewer tiles
inline int x6wp_grid(int num_cus, const sg_conv_desc* d) {
  const int64_t tiles = x6wp_tiles(d), slots = 2 * (int64_t)num_cus;
  return (int)(tiles < slots ? tiles : slots);
}


// `grid` workgroups (= partial slabs); b16: bf16 storage; planes: 3 = the six-pass arithmetic, 1 = bf16 products
int launch_x6wp(const WgradParams& p, int grid, bool b16, int planes, hipStream_t st);

}  // namespace sgconv
