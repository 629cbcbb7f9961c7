// Device helpers shared by the rank-count kernels: kg_rank.hip (queries and candidates given as
// rows) and kg_rank_proj.hip (candidates projected inside the kernel).  One copy of the score
// term, the filter lookup and the counting epilogue, so both files keep the same summation and
// counting rules (stated at the top of kg_rank.hip).
#pragma once

#include "hip/common.h"

namespace euler_hip {

// one term of the score, folded into the accumulator (the only place a score is computed)
template <int KIND>
__device__ __forceinline__ float kg_term(float acc, float q, float c) {
  if (KIND == 0) return __fadd_rn(acc, fabsf(__fsub_rn(q, c)));
  if (KIND == 1) {
    const float t = __fsub_rn(q, c);
    return fmaf(t, t, acc);
  }
  return fmaf(q, c, acc);
}

// is e in the ascending list idx[lo, hi)
__device__ __forceinline__ bool kg_filtered(const int32_t* __restrict__ idx, int64_t lo, int64_t hi, int32_t e) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int32_t v = idx[mid];
    if (v == e) return true;
    if (v < e) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return false;
}

// epilogue of one (query b, candidate e) pair that is inside the problem and not the true
// candidate: compare the score sv with the true score tsc, then (only for a pair that would
// count) look e up in b's filter list; nb / nt are the query's 32-bit counters
template <int KIND>
__device__ __forceinline__ void kg_rank_pair(float sv, float tsc, int64_t b, int64_t e,
                                             const int64_t* __restrict__ filt_ptr,
                                             const int32_t* __restrict__ filt_idx, int64_t nf, int& nb, int& nt) {
  const bool bt = KIND == 2 ? sv > tsc : sv < tsc;
  const bool tie = sv == tsc;
  if (!(bt || tie)) return;
  if (filt_ptr != nullptr) {
    int64_t lo = filt_ptr[b], hi = filt_ptr[b + 1];
    if (lo < 0) lo = 0;
    if (hi > nf) hi = nf;
    if (kg_filtered(filt_idx, lo, hi, static_cast<int32_t>(e))) return;
  }
  nb += bt ? 1 : 0;
  nt += tie ? 1 : 0;
}

}  // namespace euler_hip
