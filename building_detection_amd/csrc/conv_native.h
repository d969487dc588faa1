// The native convolution kernels (fp32-in / fp32-acc MFMA; any shape, any alignment, fp32 or bf16 storage): what the plan queries
// ask of the family, and its launch functions.  The kernels and the description of their tiling: conv_native.hip.
#pragma once
#include "conv_common.h"

namespace sgconv {

// The vector form's wave-uniform tap (UT): a slab never straddles a tap, and both operands fit a 2 GiB buffer descriptor
// (the fp32 launch and the plan query, sg_conv2d_plan, both ask here)
inline bool igemm_ut_of(const IgemmParams& p) { return ((p.C % BK == 0) || (p.K == p.C)) && p.x_bytes != 0 && p.w_bytes != 0; }

// Forward or input gradient (p: fill_fwd_params / fill_dgrad_params).  x_b16 / y_b16: bf16 storage of the tensor the kernel reads / of
// the one it writes.  fp32 / fp32 plans by native_common, the other three by mixed_common: bf16 / bf16 is the any-shape fallback of
// bf16 storage, bf16 / fp32 the forward of a softmax head that is not a thin 1x1 convolution (Res34-UNet: Conv2D(2, 3,
// activation='softmax')), fp32 / bf16 its input gradient (fp32 dy in, bf16 dx out).  vec: 4-channel runs (native_vec_of).
int dispatch_igemm(const IgemmParams& p, bool x_b16, bool y_b16, bool vec, int num_cus, hipStream_t st);
// the input gradient's weights: w[tap][ci][co] -> wt[tap][co][ci]
int launch_transpose_taps(const float* w, float* wt, int Cin, int Cout, int taps, hipStream_t st);

// Filter gradient, S pixel shares of tiles bn wide (wgrad_bn).  Storage: fp32 / fp32, bf16 / bf16, or bf16 x with fp32 dy (the softmax
// head) - precondition: never fp32 x beside bf16 dy (with fp32 x, dy_b16 is not read); fast (fp32 with vec only): 0 / 1 / 2, see
// igemm_wgrad_kernel.
int launch_wgrad_native(const WgradParams& p, int bn, int S, bool x_b16, bool dy_b16, bool vec, int fast, hipStream_t st);
// out[i] = sum over the S partial slabs part[s][i], in fixed order (v4: n % 4 == 0 and 16-byte aligned pointers)
int launch_reduce_splits(const float* part, float* out, int64_t n, int S, bool v4, hipStream_t st);

}  // namespace sgconv
