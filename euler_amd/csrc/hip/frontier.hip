// Row sets of frontier inference (models/sage_infer.py "frontier"): the rows a request reaches,
// as rank bitmaps (csr_rowset.h: int32 [ceil(N / 32), 2] = (bits, set bits before the word)).
//
//   mark            : sets the bits of a row list (entries outside [0, N) are ignored);
//   mark_neighbors  : sets the bits of the neighbours of a row list over the masked (row, type)
//                     segments (neighbours outside [0, N) are skipped, as sage_csr.hip skips
//                     them).  A block takes 32 listed rows at a time, 8 lanes per row; a row of
//                     more than kCsrHubDeg edges is left to the whole block, which then walks
//                     the chunk's hubs one after the other with all 256 threads;
//   rank            : exclusive scan of the words' popcounts: per-block totals of 1024 words,
//                     one block scans the totals (and writes the set's size), every block
//                     scans its own words on top of its total;
//   list            : every word writes its set bits at its rank: the sorted row list.
//
// Bits are set with atomicOr after a plain test of the bit, so a neighbour that many rows share
// is one atomic, not one per edge.  Block-stride loops, capped grids, int64 indices.
#include "hip/csr_rowset.h"
#include "hip/launchers.h"

namespace euler_hip {

constexpr int kFrThreads = 256;
constexpr int kFrLanes = 8;                           // lanes per listed row
constexpr int kFrRows = kFrThreads / kFrLanes;        // listed rows per block and step
constexpr int kFrPerThread = 4;                       // words per thread of the scan kernels
constexpr int kFrChunk = kFrThreads * kFrPerThread;   // words per block of the scan kernels

__device__ __forceinline__ void fr_set(uint32_t* __restrict__ words, int64_t N, int64_t j) {
  if (j < 0 || j >= N) return;
  uint32_t* w = words + 2 * (j >> 5);
  const uint32_t bit = 1u << (j & 31);
  if (!(*w & bit)) atomicOr(w, bit);
}

__global__ __launch_bounds__(kFrThreads) void fr_mark_kernel(uint32_t* __restrict__ words, int64_t N,
                                                             const int32_t* __restrict__ rows, int64_t n) {
  grid_stride(n, [&](int64_t i) { fr_set(words, N, rows[i]); });
}

__global__ __launch_bounds__(kFrThreads) void fr_mark_neighbors_kernel(uint32_t* __restrict__ words,
                                                                       const int64_t* __restrict__ indptr,
                                                                       const int32_t* __restrict__ nbr, int64_t N,
                                                                       int64_t E, int T, uint32_t mask,
                                                                       const int32_t* __restrict__ rows, int64_t n) {
  __shared__ int32_t hub[kFrRows];
  __shared__ int hub_n;
  const int tid = threadIdx.x, sub = tid % kFrLanes, slot = tid / kFrLanes;
  const int64_t chunks = ceil_div(n, kFrRows);
  // the masked segment t of row r, clamped to [0, E]
  auto bounds = [&](int64_t r, int t, int64_t& a, int64_t& b) {
    a = indptr[r * T + t];
    b = indptr[r * T + t + 1];
    a = a < 0 ? 0 : a;
    b = b > E ? E : b;
  };
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    if (tid == 0) hub_n = 0;
    __syncthreads();
    const int64_t i = chunk * kFrRows + slot;
    int64_t r = -1;
    if (i < n) r = rows[i];
    if (r >= N) r = -1;
    if (r >= 0) {
      int64_t deg = 0;
      for (int t = 0; t < T; ++t) {
        if (!((mask >> t) & 1u)) continue;
        int64_t a, b;
        bounds(r, t, a, b);
        if (b > a) deg += b - a;
      }
      if (deg > kCsrHubDeg) {
        if (sub == 0) hub[atomicAdd(&hub_n, 1)] = static_cast<int32_t>(r);
      } else if (deg > 0) {
        for (int t = 0; t < T; ++t) {
          if (!((mask >> t) & 1u)) continue;
          int64_t a, b;
          bounds(r, t, a, b);
          for (int64_t e = a + sub; e < b; e += kFrLanes) fr_set(words, N, nbr[e]);
        }
      }
    }
    __syncthreads();
    const int nh = hub_n;  // at most kFrRows: one entry per listed row of the chunk
    for (int h = 0; h < nh; ++h) {
      const int64_t r2 = hub[h];
      for (int t = 0; t < T; ++t) {
        if (!((mask >> t) & 1u)) continue;
        int64_t a, b;
        bounds(r2, t, a, b);
        for (int64_t e = a + tid; e < b; e += kFrThreads) fr_set(words, N, nbr[e]);
      }
    }
    __syncthreads();  // the next chunk resets the hub list
  }
}

// (exclusive prefix inside the block, block total) of one value per thread
__device__ __forceinline__ void fr_block_scan(int v, int* wave_tot, int& excl, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wave_tot[wv] = incl;
  __syncthreads();
  int pre = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < kFrThreads / 64; ++k) {
    if (k < wv) pre += wave_tot[k];
    total += wave_tot[k];
  }
  excl = pre + incl - v;
  __syncthreads();  // wave_tot is free again
}

// this thread's kFrPerThread words of the block's chunk: popcounts (0 past the end)
__device__ __forceinline__ int fr_counts(const uint32_t* __restrict__ words, int64_t W, int64_t w0, int* c) {
  int sum = 0;
#pragma unroll
  for (int q = 0; q < kFrPerThread; ++q) {
    c[q] = w0 + q < W ? __popc(words[2 * (w0 + q)]) : 0;
    sum += c[q];
  }
  return sum;
}

__global__ __launch_bounds__(kFrThreads) void fr_block_totals_kernel(const uint32_t* __restrict__ words, int64_t W,
                                                                     int32_t* __restrict__ totals) {
  __shared__ int wave_tot[kFrThreads / 64];
  const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kFrChunk + threadIdx.x * kFrPerThread;
  int c[kFrPerThread], excl, total;
  fr_block_scan(fr_counts(words, W, w0, c), wave_tot, excl, total);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// one block: totals [nb] -> their exclusive prefix sums in place, the grand total to *count
__global__ __launch_bounds__(kFrThreads) void fr_scan_totals_kernel(int32_t* __restrict__ totals, int64_t nb,
                                                                    int32_t* __restrict__ count) {
  __shared__ int wave_tot[kFrThreads / 64];
  int carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += kFrThreads) {
    const int64_t b = b0 + threadIdx.x;
    int excl, total;
    fr_block_scan(b < nb ? totals[b] : 0, wave_tot, excl, total);
    if (b < nb) totals[b] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(kFrThreads) void fr_rank_kernel(uint32_t* __restrict__ words, int64_t W,
                                                             const int32_t* __restrict__ totals) {
  __shared__ int wave_tot[kFrThreads / 64];
  const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kFrChunk + threadIdx.x * kFrPerThread;
  int c[kFrPerThread], excl, total;
  fr_block_scan(fr_counts(words, W, w0, c), wave_tot, excl, total);
  int r = totals[blockIdx.x] + excl;
#pragma unroll
  for (int q = 0; q < kFrPerThread; ++q) {
    if (w0 + q < W) words[2 * (w0 + q) + 1] = static_cast<uint32_t>(r);
    r += c[q];
  }
}

__global__ __launch_bounds__(kFrThreads) void fr_list_kernel(const rs_uint2* __restrict__ words, int64_t W,
                                                             int64_t count, int32_t* __restrict__ list) {
  grid_stride(W, [&](int64_t w) {
    const rs_uint2 v = words[w];
    uint32_t bits = v[0];
    int64_t p = v[1];
    while (bits) {
      const int b = __ffs(static_cast<int>(bits)) - 1;
      bits &= bits - 1;
      if (p >= 0 && p < count) list[p] = static_cast<int32_t>(w * 32 + b);  // in range whatever the ranks hold
      ++p;
    }
  });
}

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

int64_t eh_frontier_words(int64_t N) { return ceil_div(N, 32); }
int64_t eh_frontier_scan_blocks(int64_t N) { return ceil_div(ceil_div(N, 32), kFrChunk); }

static bool fr_rows_ok(int64_t N) { return N >= 1 && N < (int64_t{1} << 31); }

hipError_t eh_frontier_mark(int32_t* words, int64_t N, const int32_t* rows, int64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!fr_rows_ok(N) || n < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fr_mark_kernel, grid_for(n, kFrThreads), dim3(kFrThreads), 0, s,
                     reinterpret_cast<uint32_t*>(words), N, rows, n);
  return hipGetLastError();
}

hipError_t eh_frontier_mark_neighbors(int32_t* words, const int64_t* indptr, const int32_t* nbr, int64_t N, int64_t E,
                                      int T, uint32_t mask, const int32_t* rows, int64_t n, hipStream_t s) {
  if (n == 0 || E == 0) return hipSuccess;
  if (!fr_rows_ok(N) || n < 0 || E < 0 || T < 1 || T > 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fr_mark_neighbors_kernel, grid_for(n, kFrRows), dim3(kFrThreads), 0, s,
                     reinterpret_cast<uint32_t*>(words), indptr, nbr, N, E, T, mask, rows, n);
  return hipGetLastError();
}

hipError_t eh_frontier_rank(int32_t* words, int64_t N, int32_t* totals, int32_t* count, hipStream_t s) {
  if (!fr_rows_ok(N)) return hipErrorInvalidValue;
  const int64_t W = eh_frontier_words(N), nb = eh_frontier_scan_blocks(N);  // nb <= 2^16
  uint32_t* w = reinterpret_cast<uint32_t*>(words);
  hipLaunchKernelGGL(fr_block_totals_kernel, dim3(static_cast<uint32_t>(nb)), dim3(kFrThreads), 0, s, w, W, totals);
  EULER_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fr_scan_totals_kernel, dim3(1), dim3(kFrThreads), 0, s, totals, nb, count);
  EULER_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fr_rank_kernel, dim3(static_cast<uint32_t>(nb)), dim3(kFrThreads), 0, s, w, W, totals);
  return hipGetLastError();
}

hipError_t eh_frontier_list(const int32_t* words, int64_t N, int64_t count, int32_t* list, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (!fr_rows_ok(N) || count < 0 || count > N) return hipErrorInvalidValue;
  const int64_t W = eh_frontier_words(N);
  hipLaunchKernelGGL(fr_list_kernel, grid_for(W, kFrThreads), dim3(kFrThreads), 0, s,
                     reinterpret_cast<const rs_uint2*>(words), W, count, list);
  return hipGetLastError();
}

}  // extern "C"
