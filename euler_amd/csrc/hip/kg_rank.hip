// Link-prediction rank counts (models/kg_eval.py): every query row against every candidate
// row, fused with the comparison against the true candidate's score, so no [B, N] score
// matrix ever exists.
//
// Score kinds      0 l1   sum_d |q - c|        lower is better
//                  1 l2   sum_d (q - c)^2      lower is better (squared: same order, no sqrt)
//                  2 dot  sum_d q * c          higher is better
// Summation rule   every score, in both kernels, is kg_term folded over d ascending into one
//                  fp32 accumulator that starts at +0.  A candidate row that is bitwise equal
//                  to the true row therefore ties exactly.  Columns past d are staged as zeros:
//                  their terms are +0 and leave the accumulator unchanged.
// Counting rule    candidate e counts for query b when e != true_idx[b], e is not in b's filter
//                  list, and its score is strictly better than (better) or equal to (ties) the
//                  true score.  NaN scores compare false and count nowhere.
//
//   kg_rank_true   one thread per query: ts[b] = score(Q[b], C[true_idx[b]]).
//   kg_rank_scan   one block (4 waves) per (64-query tile, candidate range).  Query and
//                  candidate tiles are staged through LDS in chunks of 32 columns of d, the next
//                  chunk's global loads in flight under the current chunk's VALU work.  The
//                  threads form a 16 x 16 grid; thread (ty, tx) owns the 4 x 4 pairs of queries
//                  ty * 4 + i and candidates tx + 16 j and reads its operands as 16-byte LDS
//                  vectors.  A ds_read_b128 lane group is 16 non-contiguous lanes (e.g. 0-3,
//                  12-15, 20-27): all 16 tx values under two ty values.  With the row stride of
//                  36 floats its 16 candidate rows start at 16 distinct 4-bank slots, and its
//                  two query rows, 4 rows = 144 floats apart, sit on different banks, each read
//                  as a broadcast.  The epilogue compares, binary-searches the filter list only
//                  for a pair that would count, and keeps 32-bit counters per owned query; the
//                  16 lanes of a query are reduced with shuffles and lane tx = 0 stores the
//                  (query, split) partial.  Every partial has exactly one writer, so the result
//                  is deterministic.
#include "hip/common.h"
#include "hip/launchers.h"

#include <limits.h>
#include <math.h>

namespace euler_hip {

namespace {

constexpr int kKgrThreads = 256;
constexpr int kKgrTQ = 64;          // queries per block
constexpr int kKgrTC = 64;          // candidates per tile
constexpr int kKgrKC = 32;          // columns of d per LDS chunk
constexpr int kKgrLd = kKgrKC + 4;  // staging row stride (floats): 16-byte aligned, conflict-free b128 reads
constexpr int kKgrMaxSplits = 4096;
constexpr int kKgrNLoad = (kKgrTQ + kKgrTC) * kKgrKC / kKgrThreads;  // staged floats per thread and chunk

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

template <int KIND>
__global__ __launch_bounds__(kKgrThreads) void kg_rank_true_kernel(const float* __restrict__ Q,
                                                                   const float* __restrict__ C,
                                                                   const int64_t* __restrict__ true_idx, int64_t B,
                                                                   int64_t N, int d, float* __restrict__ ts) {
  grid_stride(B, [&](int64_t b) {
    const int64_t t = true_idx[b];
    float acc = __builtin_nanf("");
    if (t >= 0 && t < N) {
      const float* q = Q + b * d;
      const float* c = C + t * d;
      acc = 0.f;
      for (int k = 0; k < d; ++k) acc = kg_term<KIND>(acc, q[k], c[k]);
    }
    ts[b] = acc;
  });
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

template <int KIND, bool VEC>
__global__ __launch_bounds__(kKgrThreads) void kg_rank_scan_kernel(
    const float* __restrict__ Q, const float* __restrict__ C, const int64_t* __restrict__ true_idx,
    const float* __restrict__ ts, const int64_t* __restrict__ filt_ptr, const int32_t* __restrict__ filt_idx,
    int64_t nf, int64_t B, int64_t N, int d, int S, int64_t tiles_per_split, int64_t items,
    int64_t* __restrict__ better, int64_t* __restrict__ ties) {
  __shared__ __align__(16) float smem[(kKgrTQ + kKgrTC) * kKgrLd];
  float* Qs = smem;                    // [kKgrTQ][kKgrLd]
  float* Cs = smem + kKgrTQ * kKgrLd;  // [kKgrTC][kKgrLd]

  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int nchunk = (d + kKgrKC - 1) / kKgrKC;
  const int64_t ntiles = (N + kKgrTC - 1) / kKgrTC;
  const int64_t nqt = (B + kKgrTQ - 1) / kKgrTQ;

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t qt = item % nqt;
    const int split = static_cast<int>(item / nqt);
    const int64_t q0 = qt * kKgrTQ;
    const int64_t t_begin = split * tiles_per_split;
    int64_t t_end = t_begin + tiles_per_split;
    if (t_end > ntiles) t_end = ntiles;

    // the owned queries: true candidate and its score
    int64_t tru[4];
    float tsc[4];
    int nb[4], nt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t b = q0 + ty * 4 + i;
      const bool ok = b < B;
      tru[i] = ok ? true_idx[b] : int64_t{-1};
      tsc[i] = ok ? ts[b] : __builtin_nanf("");
      nb[i] = 0;
      nt[i] = 0;
    }

    float stage[kKgrNLoad];
    auto load_stage = [&](int64_t tile, int chunk) {
      const int64_t c0 = tile * kKgrTC;
      const int k0 = chunk * kKgrKC;
      if (VEC) {
#pragma unroll
        for (int i = 0; i < kKgrNLoad / 4; ++i) {
          const int it = tid + kKgrThreads * i;
          const int row = it >> 3, c = (it & 7) * 4;
          const bool isq = row < kKgrTQ;
          const int64_t g = isq ? q0 + row : c0 + (row - kKgrTQ);
          const bool ok = (isq ? g < B : g < N) && k0 + c < d;  // d % 4 == 0: a vector is all in or all out
          float4_t v = {0.f, 0.f, 0.f, 0.f};
          if (ok) v = *reinterpret_cast<const float4_t*>((isq ? Q : C) + g * d + k0 + c);
          stage[4 * i] = v[0];
          stage[4 * i + 1] = v[1];
          stage[4 * i + 2] = v[2];
          stage[4 * i + 3] = v[3];
        }
      } else {
#pragma unroll
        for (int i = 0; i < kKgrNLoad; ++i) {
          const int it = tid + kKgrThreads * i;
          const int row = it >> 5, c = it & 31;
          const bool isq = row < kKgrTQ;
          const int64_t g = isq ? q0 + row : c0 + (row - kKgrTQ);
          const bool ok = (isq ? g < B : g < N) && k0 + c < d;
          stage[i] = ok ? (isq ? Q : C)[g * d + k0 + c] : 0.f;
        }
      }
    };
    auto store_stage = [&]() {
      if (VEC) {
#pragma unroll
        for (int i = 0; i < kKgrNLoad / 4; ++i) {
          const int it = tid + kKgrThreads * i;
          const int row = it >> 3, c = (it & 7) * 4;
          float4_t v = {stage[4 * i], stage[4 * i + 1], stage[4 * i + 2], stage[4 * i + 3]};
          *reinterpret_cast<float4_t*>(Qs + row * kKgrLd + c) = v;  // Cs follows Qs: rows kKgrTQ.. are candidates
        }
      } else {
#pragma unroll
        for (int i = 0; i < kKgrNLoad; ++i) {
          const int it = tid + kKgrThreads * i;
          Qs[(it >> 5) * kKgrLd + (it & 31)] = stage[i];
        }
      }
    };

    if (t_begin < t_end) load_stage(t_begin, 0);
    for (int64_t tile = t_begin; tile < t_end; ++tile) {
      const int64_t c0 = tile * kKgrTC;
      float acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

      for (int chunk = 0; chunk < nchunk; ++chunk) {
        __syncthreads();  // the previous chunk's operands are consumed
        store_stage();
        __syncthreads();
        if (chunk + 1 < nchunk) {
          load_stage(tile, chunk + 1);
        } else if (tile + 1 < t_end) {
          load_stage(tile + 1, 0);
        }
        int ngroup = (d - chunk * kKgrKC + 3) / 4;
        if (ngroup > kKgrKC / 4) ngroup = kKgrKC / 4;
        for (int kg = 0; kg < ngroup; ++kg) {
          float4_t qv[4], cv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            qv[i] = *reinterpret_cast<const float4_t*>(Qs + (ty * 4 + i) * kKgrLd + kg * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            cv[j] = *reinterpret_cast<const float4_t*>(Cs + (tx + 16 * j) * kKgrLd + kg * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e)  // d ascending for every pair
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[i][j] = kg_term<KIND>(acc[i][j], qv[i][e], cv[j][e]);
        }
      }

      // epilogue: skip the true candidate, compare, then (only for a pair that would count)
      // look the candidate up in the query's filter list
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t b = q0 + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t e = c0 + tx + 16 * j;
          if (b >= B || e >= N || e == tru[i]) continue;
          const float sv = acc[i][j];
          const bool bt = KIND == 2 ? sv > tsc[i] : sv < tsc[i];
          const bool tie = sv == tsc[i];
          if (!(bt || tie)) continue;
          if (filt_ptr != nullptr) {
            int64_t lo = filt_ptr[b], hi = filt_ptr[b + 1];
            if (lo < 0) lo = 0;
            if (hi > nf) hi = nf;
            if (kg_filtered(filt_idx, lo, hi, static_cast<int32_t>(e))) continue;
          }
          nb[i] += bt ? 1 : 0;
          nt[i] += tie ? 1 : 0;
        }
      }
    }

    // the 16 lanes tx = 0..15 of a query are consecutive lanes of one wave
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int vb = nb[i], vt = nt[i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        vb += __shfl_xor(vb, o);
        vt += __shfl_xor(vt, o);
      }
      const int64_t b = q0 + ty * 4 + i;
      if (tx == 0 && b < B) {
        better[b * S + split] = vb;
        ties[b * S + split] = vt;
      }
    }
  }
}

int kg_rank_grid(int64_t blocks, int64_t cap) {
  if (blocks < 1) blocks = 1;
  return static_cast<int>(blocks < cap ? blocks : cap);
}

}  // namespace

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

int eh_kg_rank_max_splits() { return kKgrMaxSplits; }

hipError_t eh_kg_rank_true(const float* Q, const float* C, const int64_t* true_idx, int64_t B, int64_t N, int d,
                           int kind, float* ts, hipStream_t s) {
  if (B <= 0 || N <= 0 || d < 1 || kind < 0 || kind > 2) return hipErrorInvalidValue;
  const dim3 grid = grid_for(B, kKgrThreads);
  if (kind == 0)
    hipLaunchKernelGGL(kg_rank_true_kernel<0>, grid, dim3(kKgrThreads), 0, s, Q, C, true_idx, B, N, d, ts);
  else if (kind == 1)
    hipLaunchKernelGGL(kg_rank_true_kernel<1>, grid, dim3(kKgrThreads), 0, s, Q, C, true_idx, B, N, d, ts);
  else
    hipLaunchKernelGGL(kg_rank_true_kernel<2>, grid, dim3(kKgrThreads), 0, s, Q, C, true_idx, B, N, d, ts);
  return hipGetLastError();
}

hipError_t eh_kg_rank_scan(const float* Q, const float* C, const int64_t* true_idx, const float* ts,
                           const int64_t* filt_ptr, const int32_t* filt_idx, int64_t nf, int64_t B, int64_t N, int d,
                           int kind, int S, int64_t* better, int64_t* ties, hipStream_t s) {
  if (B <= 0 || N <= 0 || N > INT_MAX || d < 1 || kind < 0 || kind > 2 || S < 1 || S > kKgrMaxSplits || nf < 0)
    return hipErrorInvalidValue;  // candidate positions are compared with the 32-bit filter entries
  if (filt_ptr != nullptr && filt_idx == nullptr && nf > 0) return hipErrorInvalidValue;
  const int64_t ntiles = ceil_div(N, kKgrTC);
  const int64_t tps = ceil_div(ntiles, S);
  const bool vec = d % 4 == 0 && reinterpret_cast<uintptr_t>(Q) % 16 == 0 && reinterpret_cast<uintptr_t>(C) % 16 == 0;
  const int64_t items = ceil_div(B, kKgrTQ) * S;
  const int grid = kg_rank_grid(items, 8192);
#define EH_KG_RANK(KIND, V)                                                                                     \
  hipLaunchKernelGGL((kg_rank_scan_kernel<KIND, V>), dim3(grid), dim3(kKgrThreads), 0, s, Q, C, true_idx, ts,  \
                     filt_ptr, filt_idx, nf, B, N, d, S, tps, items, better, ties)
  if (kind == 0) {
    if (vec) EH_KG_RANK(0, true); else EH_KG_RANK(0, false);
  } else if (kind == 1) {
    if (vec) EH_KG_RANK(1, true); else EH_KG_RANK(1, false);
  } else {
    if (vec) EH_KG_RANK(2, true); else EH_KG_RANK(2, false);
  }
#undef EH_KG_RANK
  return hipGetLastError();
}

}  // extern "C"
