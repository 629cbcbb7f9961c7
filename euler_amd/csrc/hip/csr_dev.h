// Device helpers shared by the full-neighbourhood layer kernels over the graph's own CSR
// (sage_csr.hip: weight-normalised mean + [x_self | agg] GEMM; gcn_csr.hip: scaled sum + GEMM):
// the 16-byte table loads of the gather and the 4-column stores of the swapped-operand MFMA
// epilogue.  One copy: both kernels round and store through the same code.
#pragma once
#include "hip/tile.h"

namespace euler_hip {

constexpr int kCsrMaxD = 512;  // widest feature / hidden table row (Dp), a multiple of 16

// 8 consecutive features of a row as fp32 (+ the storage bits for a bf16 table)
__device__ __forceinline__ void csr_load8(const bf16_t* p, float* v) {
  const uint4_t u = *reinterpret_cast<const uint4_t*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(u[i] << 16);
    v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ void csr_load8(const float* p, float* v) {
  const float4_t a = *reinterpret_cast<const float4_t*>(p);
  const float4_t b = *reinterpret_cast<const float4_t*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = a[i];
    v[4 + i] = b[i];
  }
}

// four consecutive output columns of one row: one 8-byte (bf16, RNE) or 16-byte (fp32) store
__device__ __forceinline__ void csr_store4(bf16_t* p, float4_t v) {
  tl_uint2 o;
  o[0] = pack_bf16x2(v[0], v[1]);
  o[1] = pack_bf16x2(v[2], v[3]);
  *reinterpret_cast<tl_uint2*>(p) = o;
}

__device__ __forceinline__ void csr_store4(float* p, float4_t v) { *reinterpret_cast<float4_t*>(p) = v; }

}  // namespace euler_hip
