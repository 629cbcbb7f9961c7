// DeviceGraph.from_edges: an edge list in HBM -> the per-(row, edge type) CSR of
// graph/device_graph.py (indptr int64 [N*T+1], nbr int32, cumw fp32 inclusive prefix sums
// per segment, neighbours ascending inside a segment, equal neighbours in input order).
//
//   edge_pack   : validates ids / types / weights (failures are OR-ed into status[0], the
//                 number of ids out of range is added to status[1]; a failed edge is packed
//                 as row 0 -> row 0 so every later kernel stays in bounds), relabels ids by a
//                 binary search in the sorted id table when there is one, and writes the key
//                 ((row * T + type) << dst_bits) | dst_row with the edge index as payload;
//                 with `symmetric` the same launch writes the reverse edge at E + i
//   sort        : hipcub radix sort of (key, payload) over the bits the key uses; stable; the
//                 packed pairs and one more pair of buffers are its ping-pong buffers
//   edge_heads  : duplicates = "sum": head flag of every run of equal keys; an inclusive
//                 hipcub scan of the flags gives the output slots (no look-back, no flags
//                 between blocks of our own); edge_compact sums every run in input order in
//                 fp64 and writes the run's key, first payload and fp32 weight
//   csr_bounds  : indptr[s] = lower bound of s << dst_bits in the sorted keys
//   seg_prefix  : cumw and nbr of every segment.  A block takes 256 segments at a time and
//                 reads their lengths from indptr: a segment of <= 64 edges is summed serially
//                 by its own lane, one of 65 .. 256 edges by one wave (wave scan, carried
//                 total), a longer one (a hub) by the whole block (wave scans + LDS totals,
//                 carried total).  All sums are fp64 and are stored as fp32.
//
// Grid-stride, 256 threads, int64 indices.  Keys are unsigned 64-bit (at most 63 bits used).
#include "hip/common.h"
#include "hip/launchers.h"

#include <float.h>
#include <hipcub/hipcub.hpp>

namespace euler_hip {

constexpr int kGbShort = 64;   // longest segment summed by one lane
constexpr int kGbTile = 256;   // longest segment summed by one wave; longer ones take the block

typedef unsigned long long gb_u64;

__device__ __forceinline__ int64_t gb_load_id(const void* p, int is64, int64_t i) {
  return is64 ? static_cast<const int64_t*>(p)[i] : static_cast<int64_t>(static_cast<const int32_t*>(p)[i]);
}

// row of a raw id: the id itself without a table, else its position in the table (unique,
// ascending as unsigned 64-bit); -1 when out of range / absent
__device__ __forceinline__ int64_t gb_row_of(int64_t id, const int64_t* __restrict__ ids, int64_t N) {
  if (ids == nullptr) return (id >= 0 && id < N) ? id : -1;
  const uint64_t q = static_cast<uint64_t>(id);
  int64_t lo = 0, hi = N;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<uint64_t>(ids[mid]) < q) lo = mid + 1; else hi = mid;
  }
  return (lo < N && ids[lo] == id) ? lo : -1;
}

__global__ __launch_bounds__(256) void edge_pack_kernel(const void* __restrict__ src, int src64,
                                                        const void* __restrict__ dst, int dst64,
                                                        const float* __restrict__ w, const int32_t* __restrict__ et,
                                                        const int64_t* __restrict__ ids, int64_t N, int T,
                                                        int dst_bits, int64_t E, int symmetric,
                                                        uint64_t* __restrict__ keys, int32_t* __restrict__ idx,
                                                        gb_u64* __restrict__ status) {
  grid_stride(E, [&](int64_t i) {
    int64_t r = gb_row_of(gb_load_id(src, src64, i), ids, N);
    int64_t c = gb_row_of(gb_load_id(dst, dst64, i), ids, N);
    int t = et ? et[i] : 0;
    const int nbad = (r < 0) + (c < 0);
    unsigned bad = nbad ? 1u : 0u;
    if (t < 0 || t >= T) bad |= 2u;
    if (w) {
      const float x = w[i];
      if (!(x >= 0.f && x <= FLT_MAX)) bad |= 4u;  // negative, NaN or infinite
    }
    if (bad) {
      atomicOr(&status[0], static_cast<gb_u64>(bad));
      if (nbad) atomicAdd(&status[1], static_cast<gb_u64>(nbad));
      r = c = 0;
      t = 0;
    }
    keys[i] = (static_cast<uint64_t>(r * T + t) << dst_bits) | static_cast<uint64_t>(c);
    idx[i] = static_cast<int32_t>(i);
    if (symmetric) {
      keys[E + i] = (static_cast<uint64_t>(c * T + t) << dst_bits) | static_cast<uint64_t>(r);
      idx[E + i] = static_cast<int32_t>(E + i);
    }
  });
}

__global__ __launch_bounds__(256) void edge_heads_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                         int32_t* __restrict__ head) {
  grid_stride(n, [&](int64_t i) { head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0; });
}

__global__ void edge_runs_kernel(const int32_t* __restrict__ incl, int64_t n, gb_u64* __restrict__ status) {
  if (blockIdx.x == 0 && threadIdx.x == 0) status[2] = static_cast<gb_u64>(incl[n - 1]);
}

// the weight of the input edge behind payload p (reverse copies carry E + i)
__device__ __forceinline__ double gb_edge_weight(const float* __restrict__ w, int64_t p, int64_t E) {
  return w ? static_cast<double>(w[p >= E ? p - E : p]) : 1.0;
}

// one thread per run head: the run is walked in slot (= input) order
__global__ __launch_bounds__(256) void edge_compact_kernel(const uint64_t* __restrict__ keys,
                                                           const int32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ incl, int64_t n,
                                                           const float* __restrict__ w, int64_t E, int64_t nnz,
                                                           uint64_t* __restrict__ ckeys, int32_t* __restrict__ cidx,
                                                           float* __restrict__ cw) {
  grid_stride(n, [&](int64_t i) {
    const uint64_t k = keys[i];
    if (i != 0 && keys[i - 1] == k) return;
    const int64_t s = static_cast<int64_t>(incl[i]) - 1;
    if (s < 0 || s >= nnz) return;
    double acc = 0.0;
    int64_t j = i;
    do {
      acc += gb_edge_weight(w, idx[j], E);
      ++j;
    } while (j < n && keys[j] == k);
    ckeys[s] = k;
    cidx[s] = idx[i];
    cw[s] = static_cast<float>(acc);
  });
}

__global__ __launch_bounds__(256) void csr_bounds_kernel(const uint64_t* __restrict__ keys, int64_t nnz, int64_t S,
                                                         int dst_bits, int64_t* __restrict__ indptr) {
  grid_stride(S + 1, [&](int64_t s) {
    const uint64_t target = static_cast<uint64_t>(s) << dst_bits;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    indptr[s] = lo;
  });
}

__device__ __forceinline__ double gb_wave_scan(double v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// perm != nullptr: slot i holds input edge perm[i] (weight w[that edge], 1 without w);
// perm == nullptr: w [nnz] is the slot's weight itself (merged duplicates)
__global__ __launch_bounds__(256) void seg_prefix_kernel(const uint64_t* __restrict__ keys,
                                                         const int64_t* __restrict__ indptr, int64_t S,
                                                         int dst_bits, const float* __restrict__ w,
                                                         const int32_t* __restrict__ perm, int64_t E,
                                                         int32_t* __restrict__ nbr, float* __restrict__ cumw) {
  __shared__ int64_t hub[256];
  __shared__ double wave_tot[4];
  __shared__ int hub_n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t dmask = (uint64_t{1} << dst_bits) - 1;
  auto weight = [&](int64_t i) -> double {
    return perm ? gb_edge_weight(w, perm[i], E) : static_cast<double>(w[i]);
  };
  const int64_t step = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * 256; base < S; base += step) {
    if (tid == 0) hub_n = 0;
    __syncthreads();
    const int64_t s = base + tid;
    int64_t a = 0, len = 0;
    if (s < S) {
      a = indptr[s];
      len = indptr[s + 1] - a;
    }
    if (len > 0 && len <= kGbShort) {  // short: this lane, serially
      double acc = 0.0;
      for (int64_t i = a; i < a + len; ++i) {
        acc += weight(i);
        cumw[i] = static_cast<float>(acc);
        nbr[i] = static_cast<int32_t>(keys[i] & dmask);
      }
    } else if (len > kGbTile) {
      hub[atomicAdd(&hub_n, 1)] = s;
    }
    // medium: the wave takes its lanes' segments one after the other
    gb_u64 med = __ballot(len > kGbShort && len <= kGbTile);
    while (med) {
      const int l = __ffsll(static_cast<long long>(med)) - 1;
      med &= med - 1;
      const int64_t a2 = __shfl(a, l, 64), e2 = a2 + __shfl(len, l, 64);
      double carry = 0.0;
      for (int64_t t0 = a2; t0 < e2; t0 += 64) {
        const int64_t i = t0 + lane;
        const double incl = gb_wave_scan(i < e2 ? weight(i) : 0.0, lane);
        if (i < e2) {
          cumw[i] = static_cast<float>(carry + incl);
          nbr[i] = static_cast<int32_t>(keys[i] & dmask);
        }
        carry += __shfl(incl, 63, 64);
      }
    }
    __syncthreads();
    // hubs: the whole block, tile by tile with a carried total
    const int nh = hub_n;
    for (int h = 0; h < nh; ++h) {
      const int64_t s2 = hub[h];
      const int64_t a2 = indptr[s2], e2 = indptr[s2 + 1];
      double carry = 0.0;
      for (int64_t t0 = a2; t0 < e2; t0 += 256) {
        const int64_t i = t0 + tid;
        const double incl = gb_wave_scan(i < e2 ? weight(i) : 0.0, lane);
        if (lane == 63) wave_tot[wv] = incl;
        __syncthreads();
        double pre = carry, tot = carry;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < wv) pre += wave_tot[k];
          tot += wave_tot[k];
        }
        if (i < e2) {
          cumw[i] = static_cast<float>(pre + incl);
          nbr[i] = static_cast<int32_t>(keys[i] & dmask);
        }
        carry = tot;
        __syncthreads();
      }
    }
    __syncthreads();
  }
}

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

int eh_gb_short_len() { return kGbShort; }
int eh_gb_wave_len() { return kGbTile; }

static bool gb_bits_ok(int64_t N, int T, int dst_bits) {
  if (N < 1 || N >= (int64_t{1} << 31) || T < 1 || T > 32 || dst_bits < 1 || dst_bits > 31) return false;
  if (((N - 1) >> dst_bits) != 0) return false;          // a row does not fit its field
  const int64_t S = N * T;
  return dst_bits < 63 && (S >> (63 - dst_bits)) == 0;   // (S << dst_bits) stays below 2^63
}

hipError_t eh_gb_pack(const void* src, int src64, const void* dst, int dst64, const float* w, const int32_t* et,
                      const int64_t* ids, int64_t N, int T, int dst_bits, int64_t E, int symmetric, int64_t* keys,
                      int32_t* idx, int64_t* status, hipStream_t s) {
  if (E == 0) return hipSuccess;
  if (E < 0 || E * (symmetric ? 2 : 1) >= (int64_t{1} << 31) || !gb_bits_ok(N, T, dst_bits))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(edge_pack_kernel, grid_for(E), dim3(256), 0, s, src, src64, dst, dst64, w, et, ids, N, T,
                     dst_bits, E, symmetric, reinterpret_cast<uint64_t*>(keys), idx,
                     reinterpret_cast<gb_u64*>(status));
  return hipGetLastError();
}

// The two buffer pairs are the sort's ping-pong buffers (hipcub DoubleBuffer: no third copy
// of the pairs in the scratch); (keys_a, idx_a) hold the input, both pairs are overwritten and
// *result_in_b says which pair holds the sorted output.  temp null: *temp_bytes receives the
// scratch size and nothing runs
hipError_t eh_gb_sort(int64_t* keys_a, int64_t* keys_b, int32_t* idx_a, int32_t* idx_b, int64_t n, int end_bit,
                      void* temp, size_t* temp_bytes, int* result_in_b, hipStream_t s) {
  if (n < 1 || n >= (int64_t{1} << 31) || end_bit < 1 || end_bit > 63) return hipErrorInvalidValue;
  hipcub::DoubleBuffer<uint64_t> k(reinterpret_cast<uint64_t*>(keys_a), reinterpret_cast<uint64_t*>(keys_b));
  hipcub::DoubleBuffer<int32_t> v(idx_a, idx_b);
  const hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp, *temp_bytes, k, v, static_cast<int>(n), 0, end_bit, s);
  if (temp != nullptr && e == hipSuccess) {
    if ((k.Current() == reinterpret_cast<uint64_t*>(keys_b)) != (v.Current() == idx_b)) return hipErrorUnknown;
    *result_in_b = k.Current() == reinterpret_cast<uint64_t*>(keys_b) ? 1 : 0;
  }
  return e;
}

// head [n] / incl [n] int32 scratch; status[2] = number of runs.  temp null: size query
hipError_t eh_gb_heads(const int64_t* keys, int64_t n, int32_t* head, int32_t* incl, int64_t* status, void* temp,
                       size_t* temp_bytes, hipStream_t s) {
  if (n < 1 || n >= (int64_t{1} << 31)) return hipErrorInvalidValue;
  if (!temp) return hipcub::DeviceScan::InclusiveSum(nullptr, *temp_bytes, head, incl, static_cast<int>(n), s);
  hipLaunchKernelGGL(edge_heads_kernel, grid_for(n), dim3(256), 0, s, reinterpret_cast<const uint64_t*>(keys), n,
                     head);
  EULER_HIP_CHECK(hipGetLastError());
  EULER_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(temp, *temp_bytes, head, incl, static_cast<int>(n), s));
  hipLaunchKernelGGL(edge_runs_kernel, dim3(1), dim3(64), 0, s, incl, n, reinterpret_cast<gb_u64*>(status));
  return hipGetLastError();
}

hipError_t eh_gb_compact(const int64_t* keys, const int32_t* idx, const int32_t* incl, int64_t n, const float* w,
                         int64_t E, int64_t nnz, int64_t* ckeys, int32_t* cidx, float* cw, hipStream_t s) {
  if (n < 1 || nnz < 1 || nnz > n || E < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(edge_compact_kernel, grid_for(n), dim3(256), 0, s, reinterpret_cast<const uint64_t*>(keys), idx,
                     incl, n, w, E, nnz, reinterpret_cast<uint64_t*>(ckeys), cidx, cw);
  return hipGetLastError();
}

hipError_t eh_gb_csr(const int64_t* keys, int64_t nnz, int64_t N, int T, int dst_bits, const float* w,
                     const int32_t* perm, int64_t E, int64_t* indptr, int32_t* nbr, float* cumw, hipStream_t s) {
  if (nnz < 0 || !gb_bits_ok(N, T, dst_bits) || (perm == nullptr && w == nullptr && nnz > 0))
    return hipErrorInvalidValue;
  const int64_t S = N * T;
  hipLaunchKernelGGL(csr_bounds_kernel, grid_for(S + 1), dim3(256), 0, s, reinterpret_cast<const uint64_t*>(keys),
                     nnz, S, dst_bits, indptr);
  EULER_HIP_CHECK(hipGetLastError());
  if (nnz == 0) return hipSuccess;
  hipLaunchKernelGGL(seg_prefix_kernel, grid_for(S), dim3(256), 0, s, reinterpret_cast<const uint64_t*>(keys), indptr,
                     S, dst_bits, w, perm, E, nbr, cumw);
  return hipGetLastError();
}

}  // extern "C"
