// Device helpers and limits shared by the k-nearest-neighbour kernels (knn.hip: fp32 tables,
// knn_bf16.hip: bf16 tables, knn_grouped.hip: the list-grouped IVF search over both): the sorted
// k-best list in LDS with its threshold, the unaligned bf16 load, and the launchers' grid cap.
// Ordering rule and partial format: see knn.hip.
#pragma once
#include "hip/common.h"

#include <limits.h>

namespace euler_hip {

constexpr int kKnnThreads = 256;
constexpr int kKnnMaxK = 128;
constexpr int kKnnMaxSplits = 64;

// Offer one candidate per lane (score s, offset off ascending with the lane, valid) to a
// sorted k-best list kept in LDS (ld / lo, c entries, threshold (td, to) = the k-th entry
// once full).  Whole-wave call; c, td, to are wave-uniform.
__device__ __forceinline__ void knn_wave_select(float s, int off, bool valid, volatile float* ld, volatile int* lo,
                                                int k, int& c, float& td, int& to) {
  const int lane = threadIdx.x & 63;
  uint64_t m = __ballot(valid && (s < td || (s == td && off < to)));
  while (m) {
    const int b = __ffsll(static_cast<unsigned long long>(m)) - 1;
    m &= m - 1;
    const float cs = __shfl(s, b);
    const int co = __shfl(off, b);
    if (!(cs < td || (cs == td && co < to))) continue;
    const int lim = c < k ? c + 1 : k;
    const int j0 = lane, j1 = lane + 64;
    const bool in0 = j0 < c, in1 = j1 < c;
    const float d0 = in0 ? ld[j0] : 0.f;
    const int e0 = in0 ? lo[j0] : 0;
    float d1 = 0.f;
    int e1 = 0;
    if (k > 64 && in1) {
      d1 = ld[j1];
      e1 = lo[j1];
    }
    const bool less0 = in0 && (d0 < cs || (d0 == cs && e0 < co));
    const bool less1 = in1 && (d1 < cs || (d1 == cs && e1 < co));
    const int pos = __popcll(__ballot(less0)) + __popcll(__ballot(less1));
    // entry j - 1 of the old list
    float p0 = __shfl_up(d0, 1);
    int q0 = __shfl_up(e0, 1);
    float p1 = __shfl_up(d1, 1);
    int q1 = __shfl_up(e1, 1);
    const float w0 = __shfl(d0, 63);
    const int w1 = __shfl(e0, 63);
    if (lane == 0) {
      p1 = w0;
      q1 = w1;
    }
    if (j0 >= pos && j0 < lim) {
      ld[j0] = j0 == pos ? cs : p0;
      lo[j0] = j0 == pos ? co : q0;
    }
    if (j1 >= pos && j1 < lim) {
      ld[j1] = j1 == pos ? cs : p1;
      lo[j1] = j1 == pos ? co : q1;
    }
    c = lim;
    if (c == k) {
      td = ld[k - 1];
      to = lo[k - 1];
    }
  }
}

// 8 bf16 starting at p, the first `valid` of them in range (the rest zero), by 2-byte loads
__device__ __forceinline__ uint4_t kb_load8_scalar(const bf16_t* __restrict__ p, int valid) {
  uint4_t v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t h = e < valid ? p[e] : 0u;
    v[e >> 1] |= h << (16 * (e & 1));
  }
  return v;
}

inline int knn_grid(int64_t blocks, int64_t cap) {
  if (blocks < 1) blocks = 1;
  return static_cast<int>(blocks < cap ? blocks : cap);
}

}  // namespace euler_hip
