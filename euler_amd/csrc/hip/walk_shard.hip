// One hop of a random walk over the row-sharded graph (graph/sharded_graph.py
// ShardedDeviceGraph.random_walk; reference tf_euler/kernels/random_walk_op.cc:172-291 over
// euler/core/kernels/remote_op.cc:60-146).  Row r lives on rank r % W at local row r / W.
// Per hop a walker's current row goes to its owner over a fixed-capacity all-to-all
// (route.hip), the owner draws the next row from its local CSR, a second all-to-all
// returns it.  The three kernels here are everything else a hop needs:
//   keys    : hop 0 only: column 0 of the walks and one int64 request per walker,
//             key = ticket * R + row (R = num_rows rounded up to a multiple of W, so
//             key % W == row % W and route_by_owner routes the key as it is), ticket =
//             rank * n + i; -1 for a walker with no row to step from (never routed)
//   owner   : per received request, the unbiased draw of random_walk_kernel
//             (sampling_math.h walk_draw_unbiased) with Philox counter ticket * 1024 + hop:
//             distinct (ticket, hop) never share a counter inside an owner, and with one
//             rank the walk is the whole-graph kernel's bit for bit
//   unroute : the returned answers back in walker order: column hop + 1 of the walks
//             (default where the walker had no slot, no row or no edge) and the next hop's
//             request keys
// Grid-stride, 256 threads, int64 indices (W * C * walk_len and E pass 2^31 at scale).
#include "hip/common.h"
#include "hip/launchers.h"
#include "hip/sampling_math.h"

namespace euler_hip {

__device__ __forceinline__ int64_t walk_key(int64_t row, int64_t num_rows, int64_t R, int64_t ticket) {
  return (row >= 0 && row < num_rows) ? ticket * R + row : -1;
}

__global__ __launch_bounds__(256) void walk_keys_kernel(const int32_t* __restrict__ starts, int64_t n,
                                                        int64_t num_rows, int64_t R, int64_t ticket0, int64_t cols,
                                                        int32_t* __restrict__ out, int64_t* __restrict__ keys) {
  grid_stride(n, [&](int64_t i) {
    const int32_t row = starts[i];
    out[i * cols] = row;
    keys[i] = walk_key(row, num_rows, R, ticket0 + i);
  });
}

__global__ __launch_bounds__(256) void walk_step_owner_kernel(
    const int64_t* __restrict__ req, int64_t m, int64_t R, int W, const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ nbr, const float* __restrict__ cumw, int64_t local_rows, int num_types,
    uint32_t mask, int hop, const int64_t* __restrict__ rng, uint64_t stream_id, int32_t* __restrict__ ans) {
  grid_stride(m, [&](int64_t j) {
    const int64_t key = req[j];
    int32_t nxt = -1;
    if (key >= 0) {
      const int64_t ticket = key / R, local = (key - ticket * R) / W;
      if (local < local_rows) {
        const uint4_t r = walk_philox(rng, stream_id, static_cast<uint64_t>(ticket), hop);
        nxt = walk_draw_unbiased(indptr, nbr, cumw, num_types, mask, local, r, -1);
      }
    }
    ans[j] = nxt;
  });
}

__global__ __launch_bounds__(256) void walk_unroute_kernel(const int32_t* __restrict__ back, int64_t m,
                                                           const int64_t* __restrict__ pos, int64_t n,
                                                           int32_t default_row, int64_t num_rows, int64_t R,
                                                           int64_t ticket0, int64_t cols, int64_t col,
                                                           int32_t* __restrict__ out, int64_t* __restrict__ keys) {
  grid_stride(n, [&](int64_t i) {
    const int64_t p = pos[i];  // m: the trash slot (ended walker, or no room at the owner)
    const int32_t v = (p >= 0 && p < m) ? back[p] : -1;
    const int32_t nxt = v >= 0 ? v : default_row;
    out[i * cols + col] = nxt;
    keys[i] = walk_key(nxt, num_rows, R, ticket0 + i);
  });
}

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

hipError_t eh_walk_keys(const int32_t* starts, int64_t n, int64_t num_rows, int64_t R, int64_t ticket0, int64_t cols,
                        int32_t* out, int64_t* keys, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (R < num_rows || R < 1 || cols < 1 || ticket0 < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(walk_keys_kernel, grid_for(n), dim3(256), 0, s, starts, n, num_rows, R, ticket0, cols, out,
                     keys);
  return hipGetLastError();
}

hipError_t eh_walk_step_owner(const int64_t* req, int64_t m, int64_t R, int W, const int64_t* indptr,
                              const int32_t* nbr, const float* cumw, int64_t local_rows, int num_types,
                              uint32_t mask, int hop, const int64_t* rng, uint64_t stream_id, int32_t* ans,
                              hipStream_t s) {
  if (m == 0) return hipSuccess;
  if (R < 1 || W < 1 || R % W != 0 || num_types < 1 || num_types > 32 || hop < 0 || hop >= 1024)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(walk_step_owner_kernel, grid_for(m), dim3(256), 0, s, req, m, R, W, indptr, nbr, cumw,
                     local_rows, num_types, mask, hop, rng, stream_id, ans);
  return hipGetLastError();
}

hipError_t eh_walk_unroute(const int32_t* back, int64_t m, const int64_t* pos, int64_t n, int32_t default_row,
                           int64_t num_rows, int64_t R, int64_t ticket0, int64_t cols, int64_t col, int32_t* out,
                           int64_t* keys, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (R < num_rows || R < 1 || col < 1 || col >= cols || ticket0 < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(walk_unroute_kernel, grid_for(n), dim3(256), 0, s, back, m, pos, n, default_row, num_rows, R,
                     ticket0, cols, col, out, keys);
  return hipGetLastError();
}

}  // extern "C"
