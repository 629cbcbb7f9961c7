// Row sets over the graph's rows as rank bitmaps, and the row -> table-position step of the
// full-neighbourhood layer (sage_csr.hip) that reads a table through one (frontier.hip builds
// the sets; ops/frontier_ops.py, models/sage_infer.py "frontier").
//
// A set of graph rows is an int32 [ceil(N / 32), 2] array: word w holds the bits of rows
// 32 w .. 32 w + 31 and, next to them, the number of set bits before the word.  The position
// of row j in the set's sorted row list (= in a compact table [count, D] of the set's rows) is
//   rank[j >> 5] + popcount(bits[j >> 5] & ((1 << (j & 31)) - 1)),
// one 8-byte load per lookup and N / 4 bytes per set.
#pragma once
#include "hip/common.h"

namespace euler_hip {

// more edges than this: the whole block takes the row (sage_csr.hip's gather, frontier.hip's marking)
constexpr int kCsrHubDeg = 256;

typedef uint32_t rs_uint2 __attribute__((ext_vector_type(2)));

// The row -> table-position step of sage_csr.hip: p = pos_of(j) for a graph row j in [0, N)
// (callers leave p = -1 for a j outside it), and found(in_graph, p): whether x has a row to
// read there; one that is not found is never read and counts as a zero row.
// x has one row per graph row
struct RowIdentity {
  __device__ __forceinline__ int64_t operator()(int64_t j) const { return j; }
  __device__ __forceinline__ static bool found(bool in_graph, int64_t) { return in_graph; }
};

// x [count, D] holds the set's rows in list order.  A row whose bit is clear is never read:
// -1 (the caller's zero row) and one more in *missing; the position stays below count
// whatever the rank words hold.
struct RowRank {
  const rs_uint2* __restrict__ words;
  int32_t count;
  uint32_t* missing;
  __device__ __forceinline__ int64_t operator()(int64_t j) const {
    const uint32_t r = static_cast<uint32_t>(j);  // N < 2^31
    const rs_uint2 v = words[r >> 5];
    const uint32_t bit = 1u << (r & 31u);
    if (!(v[0] & bit)) {
      atomicAdd(missing, 1u);
      return -1;
    }
    const int32_t p = static_cast<int32_t>(v[1] + __popc(v[0] & (bit - 1u)));
    return p < count ? p : count - 1;
  }
  __device__ __forceinline__ static bool found(bool, int64_t p) { return p >= 0; }
};

}  // namespace euler_hip
