// The softmax cross-entropy instantiations of the fused GCN head (gcn_tiles.h
// gcn_head_kernel<KP, HP, kGcnLossSoftmax>: the logits phase split around one barrier into
// per-tile row statistics and their merge in tile order), in a translation unit of their own:
// built without the packed fp32 instructions (_build.py NO_PACKED_FP32), while gcn.hip and
// with it the sigmoid head keep their build line and their code.  eh_gcn_head (gcn.hip)
// validates the argument block and hands the softmax launches here.
#include "hip/gcn_tiles.h"

namespace euler_hip {

#define GCN_HEAD_SOFTMAX(K, H, grid, lds, s, A) GCN_HEAD_LOSS(K, H, kGcnLossSoftmax, grid, lds, s, A)

hipError_t gcn_head_softmax_launch(const GcnHeadArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  if (a.loss != kGcnLossSoftmax || a.Cp > 16 * kGcnSmTiles || lds + kGcnSmLdsBytes > 160 * 1024)
    return hipErrorInvalidValue;
  GCN_DISPATCH(a.lin.inp, a.lin.outp, GCN_HEAD_SOFTMAX, grid, lds, s, a);
  return hipGetLastError();
}

}  // namespace euler_hip
