// One weighted neighbour draw of a (row, type)-segmented CSR with per-segment cumulative
// weights, shared by sample_neighbor_kernel (sampling.hip) and the fused GCN step's
// layer-wise draw (gcn.hip): the edge-type group proportionally to its weight sum (u01 of
// r[0]), then the first position whose cumulative weight exceeds u01(r[1]) * total.
// Returns the neighbour row or default_row; *w / *t: its weight and type (-1: none).
#pragma once
#include "hip/common.h"

namespace euler_hip {

__device__ __forceinline__ int32_t sample_one_neighbor(const int64_t* __restrict__ indptr,
                                                       const int32_t* __restrict__ nbr,
                                                       const float* __restrict__ cumw, int num_types,
                                                       uint32_t type_mask, int64_t row, const uint4_t& r,
                                                       int32_t default_row, float* w_out, int32_t* t_out) {
  const int64_t base = row * num_types;
  int64_t lo = 0, hi = 0;
  float total = 0.f;
  int32_t t = -1;
  if (num_types == 1) {
    lo = indptr[base];
    hi = indptr[base + 1];
    total = hi > lo ? cumw[hi - 1] : 0.f;
    t = 0;
  } else {
    float tot = 0.f;
    for (int k = 0; k < num_types; ++k) {
      if (!((type_mask >> k) & 1u)) continue;
      const int64_t a = indptr[base + k], b = indptr[base + k + 1];
      if (b > a) tot += cumw[b - 1];
    }
    if (tot > 0.f) {
      float u = u01(r[0]) * tot;
      for (int k = 0; k < num_types; ++k) {
        if (!((type_mask >> k) & 1u)) continue;
        const int64_t a = indptr[base + k], b = indptr[base + k + 1];
        if (b <= a) continue;
        const float g = cumw[b - 1];
        lo = a;
        hi = b;
        total = g;
        t = k;
        if (u < g) break;
        u -= g;
      }
    }
  }
  int32_t res = default_row;
  float w = 0.f;
  if (hi > lo && total > 0.f) {
    const float u = u01(r[1]) * total;
    int64_t a = lo, b = hi - 1;  // first position with cumw > u
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if (cumw[m] > u) b = m;
      else a = m + 1;
    }
    res = nbr[a];
    w = cumw[a] - (a > lo ? cumw[a - 1] : 0.f);
  } else {
    t = -1;
  }
  if (w_out) *w_out = w;
  if (t_out) *t_out = t;
  return res;
}

// One unbiased random-walk step (p = q = 1) from `row`, shared by random_walk_kernel
// (sampling.hip) and the sharded walk's owner kernel (walk_shard.hip) so a walker draws
// the same neighbour whichever of the two advances it: the edge-type group by its weight
// sum (u01 of r[0]), then the first position whose cumulative weight exceeds
// u01(r[1]) * the group's sum.  Returns default_row when no edge type of the mask has an
// edge.
__device__ __forceinline__ int32_t walk_draw_unbiased(const int64_t* __restrict__ indptr,
                                                      const int32_t* __restrict__ nbr,
                                                      const float* __restrict__ cumw, int num_types,
                                                      uint32_t mask, int64_t row, const uint4_t& r,
                                                      int32_t default_row) {
  const int64_t base = row * num_types;
  float tot = 0.f;
  for (int t = 0; t < num_types; ++t) {
    if (!((mask >> t) & 1u)) continue;
    const int64_t a = indptr[base + t], b = indptr[base + t + 1];
    if (b > a) tot += cumw[b - 1];
  }
  if (!(tot > 0.f)) return default_row;
  float u = u01(r[0]) * tot;
  int64_t lo = 0, hi = 0;
  float g = 0.f;
  for (int t = 0; t < num_types; ++t) {
    if (!((mask >> t) & 1u)) continue;
    const int64_t a = indptr[base + t], b = indptr[base + t + 1];
    if (b <= a) continue;
    g = cumw[b - 1];
    lo = a;
    hi = b;
    if (u < g) break;
    u -= g;
  }
  const float v = u01(r[1]) * g;
  int64_t a = lo, b = hi - 1;
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if (cumw[m] > v) b = m;
    else a = m + 1;
  }
  return nbr[a];
}

// The Philox words of walker `ticket` at hop `s` (walk_len <= 1024 hops per ticket).
__device__ __forceinline__ uint4_t walk_philox(const int64_t* __restrict__ rng, uint64_t stream_id,
                                               uint64_t ticket, int s) {
  return Philox::gen(static_cast<uint64_t>(rng[0]), (static_cast<uint64_t>(rng[1]) << 8) ^ stream_id,
                     ticket * 1024u + s);
}

}  // namespace euler_hip
