// The streaming kernels of the convolutions: the "thin" 1x1 convolutions (at most 4 output channels: the sSE gate, the softmax head)
// and the segmented column reductions that belong to a convolution - the bias gradient and the BatchNormalization statistics from
// the per-tile sums of a convolution's epilogue.  What the plans ask of the family, and its launch functions; the kernels:
// conv_thin.hip, the one convolution unit that launches the segmented reducer (sg_reduce.h).
#pragma once
#include "conv_common.h"

namespace sgconv {

inline bool thin_ok(const sg_conv_desc* d) {
  const bool off = sg_switch<SW_CONV_NOTHIN>();  // A/B switch
  const int xl = d->x_ld ? d->x_ld : d->Cin;
  return !off && d->KH == 1 && d->KW == 1 && d->stride == 1 && d->Cout <= 4 && d->Ho == d->H && d->Wo == d->W &&
         d->Cin % 4 == 0 && xl % 4 == 0 && d->Cin >= 16;
}
// partial rows of the thin filter gradient's reduction
size_t thin_part_bytes(int num_cus, const sg_conv_desc* d);

// x_b16 / y_b16: bf16 storage of the tensor with Cin channels (x, dx) / of the few-channel side (y, dy).  The forms that exist:
// fp32 / fp32, bf16 / bf16, and bf16 / fp32 (SG_HEAD_F32, the softmax head of a bf16 model: no `bn`, no `res`).  Precondition: never
// fp32 x beside bf16 y (with fp32 x, y_b16 is not read).
int launch_thin_fwd(const sg_conv_desc* d, bool x_b16, bool y_b16, const void* x, const float* w, const float* bias, void* y, int flags,
                    hipStream_t st, const BnIn& bn);
int launch_thin_dgrad(const sg_conv_desc* d, bool x_b16, bool y_b16, const void* dy, const float* w, void* dx, hipStream_t st,
                      const void* res);
int launch_thin_wgrad(int num_cus, const sg_conv_desc* d, bool x_b16, bool y_b16, const void* x, const void* dy, float* dw, float* part,
                      hipStream_t st, const BnIn& bn);

// bias gradient = column sums of dy[rows][C] (pixel stride ld)
size_t colsum_ws_bytes(int num_cus, int64_t rows, int C);
int launch_colsum(int num_cus, bool b16, const void* dy, int64_t rows, int C, int ld, float* out, float* part, hipStream_t st);

// mean / variance over all rows from the per-tile (sum, centred sum of squares) pairs of a convolution's epilogue (SG_EPI_BN_STATS),
// then the BatchNormalization bookkeeping
size_t bn_tiles_ws_bytes(int num_cus, int tiles, int C);                           // enough for either alignment of `stats`
size_t bn_tiles_part_bytes(int num_cus, int tiles, int C, const void* stats);      // what a launch on `stats` needs
// stats: [tiles][2][C]; rows: pixels (not tiles); `part` holds bn_tiles_part_bytes
int launch_bn_tiles(int num_cus, const float* stats, int tiles, int C, int64_t rows, float* moving_mean, float* moving_var,
                    float* save_mean, float* save_invstd, float momentum, float eps, int unbiased, float* part, hipStream_t st);

}  // namespace sgconv
