// k-nearest-neighbour search (tools/knn.py): fused squared-distance + top-k kernels, so no
// [queries, rows] distance matrix ever exists.
//
// Ranking key      s = ||x||^2 - 2 q.x   (||q||^2 is constant per query; knn_merge adds it)
// Ordering rule    ascending (s, original row): equal scores go to the lower row, in every
//                  kernel and across the merge.
// Partial format   per (query, split) a sorted list  dist [nq, S, k] fp32 / row [nq, S, k]
//                  int64, missing entries +inf / -1.
//
//   knn_flat_scan  one block (4 waves) per (query tile, row range of X).  The dot products
//                  are fp32-input MFMAs (v_mfma_f32_32x32x2_f32: lane l supplies
//                  A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]; C/D column l & 31,
//                  row (r & 3) + 8 (r >> 2) + 4 (l >> 5)) over operands staged through LDS in
//                  chunks of 32 columns of d (zero-padded past d), the next chunk's global
//                  loads in flight under the current chunk's MFMAs.  The k order inside a
//                  group of 8 is permuted the same way for A and B (each lane half takes 4
//                  consecutive columns as one 16-byte LDS read).  A 64-row score tile goes to
//                  LDS; a query whose tile holds a score at or under its threshold is
//                  rescanned by its owner wave, which inserts into the query's sorted k-best
//                  list in LDS (one lane per list slot).
//   knn_ivf_scan   one wave per (query, probed list) over the CSR inverted lists; lanes split
//                  d, a butterfly reduction gives the score, 64 rows are ranked at a time by
//                  the same list insertion.  Inside a list the positions must be in ascending
//                  original-row order (a stable sort by list gives that).
//   knn_merge      one wave per query: S-way merge of the sorted partials, + ||q||^2, clamp.
#include "hip/common.h"
#include "hip/launchers.h"

#include <limits.h>
#include <math.h>

namespace euler_hip {

namespace {

constexpr int kKnnThreads = 256;
constexpr int kKnnTR = 64;        // rows of X per score tile
constexpr int kKnnKC = 32;        // columns of d per LDS chunk
constexpr int kKnnLd = kKnnKC + 4;  // staging row stride (floats): 16-byte aligned, conflict-free b128 reads
constexpr int kKnnScLd = 72;      // score tile row stride (floats)
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

// ---------------------------------------------------------------------------------- flat
// TQ queries per block: 128 (each wave 32 queries x 64 rows, two accumulators) or 64 (each
// wave 32 queries x 32 rows), picked by the launcher from k (the lists are TQ * k * 8 bytes).
template <int TQ, bool VEC>
__global__ __launch_bounds__(kKnnThreads) void knn_flat_scan_kernel(const float* __restrict__ Q,
                                                                    const float* __restrict__ X,
                                                                    const float* __restrict__ xn, int64_t nq,
                                                                    int64_t n, int d, int k, int S,
                                                                    int64_t tiles_per_split, int64_t items,
                                                                    float* __restrict__ pd,
                                                                    int64_t* __restrict__ pr) {
  constexpr int NWQ = TQ / 32;        // waves along the queries
  constexpr int NB = 2 / (4 / NWQ);   // 32-row column blocks per wave
  constexpr int QW = TQ / 4;          // queries owned per wave in the selection
  constexpr int NLOAD = (TQ + kKnnTR) * kKnnKC / kKnnThreads;  // staged floats per thread and chunk
  extern __shared__ __align__(16) float knn_smem[];
  float* As = knn_smem;                          // [TQ][kKnnLd]
  float* Bs = As + TQ * kKnnLd;                  // [64][kKnnLd]
  float* xns = Bs + kKnnTR * kKnnLd;             // [64]
  float* sc = xns + kKnnTR;                      // [TQ][kKnnScLd]
  float* st_td = sc + TQ * kKnnScLd;             // [TQ] threshold score
  int* st_to = reinterpret_cast<int*>(st_td + TQ);   // [TQ] threshold offset
  int* st_c = st_to + TQ;                        // [TQ] entries held
  int* qflag = st_c + TQ;                        // [TQ] tile has a candidate
  float* ld = reinterpret_cast<float*>(qflag + TQ);  // [TQ][k]
  int* lo = reinterpret_cast<int*>(ld + static_cast<size_t>(TQ) * k);  // [TQ][k]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int wq = w % NWQ, cb0 = (w / NWQ) * NB;
  const int nchunk = (d + kKnnKC - 1) / kKnnKC;
  const int64_t ntiles = (n + kKnnTR - 1) / kKnnTR;
  const int64_t nqt = (nq + TQ - 1) / TQ;
  const float inf = __builtin_inff();

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t qt = item % nqt;
    const int split = static_cast<int>(item / nqt);
    const int64_t q0 = qt * TQ;
    const int64_t t_begin = split * tiles_per_split;
    int64_t t_end = t_begin + tiles_per_split;
    if (t_end > ntiles) t_end = ntiles;
    const int64_t r_begin = t_begin * kKnnTR;

    __syncthreads();  // the previous item's lists and state are written out
    for (int i = tid; i < TQ; i += kKnnThreads) {
      st_td[i] = inf;
      st_to[i] = INT_MAX;
      st_c[i] = 0;
      qflag[i] = 0;
    }

    float stage[NLOAD];
    float stage_xn = 0.f;
    auto load_stage = [&](int64_t tile, int chunk) {
      const int64_t x0 = tile * kKnnTR;
      const int k0 = chunk * kKnnKC;
      if (VEC) {
#pragma unroll
        for (int i = 0; i < NLOAD / 4; ++i) {
          const int it = tid + kKnnThreads * i;
          const int row = it >> 3, c = (it & 7) * 4;
          const bool isq = row < TQ;
          const int64_t g = isq ? q0 + row : x0 + (row - TQ);
          const bool ok = (isq ? g < nq : g < n) && k0 + c < d;
          float4_t v = {0.f, 0.f, 0.f, 0.f};
          if (ok) v = *reinterpret_cast<const float4_t*>((isq ? Q : X) + g * d + k0 + c);
          stage[4 * i] = v[0];
          stage[4 * i + 1] = v[1];
          stage[4 * i + 2] = v[2];
          stage[4 * i + 3] = v[3];
        }
      } else {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
          const int it = tid + kKnnThreads * i;
          const int row = it >> 5, c = it & 31;
          const bool isq = row < TQ;
          const int64_t g = isq ? q0 + row : x0 + (row - TQ);
          const bool ok = (isq ? g < nq : g < n) && k0 + c < d;
          stage[i] = ok ? (isq ? Q : X)[g * d + k0 + c] : 0.f;
        }
      }
      if (chunk == 0 && tid < kKnnTR) stage_xn = x0 + tid < n ? xn[x0 + tid] : 0.f;
    };
    auto store_stage = [&](int chunk) {
      if (VEC) {
#pragma unroll
        for (int i = 0; i < NLOAD / 4; ++i) {
          const int it = tid + kKnnThreads * i;
          const int row = it >> 3, c = (it & 7) * 4;
          float4_t v = {stage[4 * i], stage[4 * i + 1], stage[4 * i + 2], stage[4 * i + 3]};
          *reinterpret_cast<float4_t*>(As + row * kKnnLd + c) = v;  // Bs follows As: rows TQ.. are X rows
        }
      } else {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
          const int it = tid + kKnnThreads * i;
          As[(it >> 5) * kKnnLd + (it & 31)] = stage[i];
        }
      }
      if (chunk == 0 && tid < kKnnTR) xns[tid] = stage_xn;
    };

    if (t_begin < t_end) load_stage(t_begin, 0);
    for (int64_t tile = t_begin; tile < t_end; ++tile) {
      const int64_t x0 = tile * kKnnTR;
      float16_t acc[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

      for (int chunk = 0; chunk < nchunk; ++chunk) {
        __syncthreads();  // the previous chunk's operands (and the previous tile's scores) are consumed
        store_stage(chunk);
        __syncthreads();
        if (chunk + 1 < nchunk) {
          load_stage(tile, chunk + 1);
        } else if (tile + 1 < t_end) {
          load_stage(tile + 1, 0);
        }
        int ngroup = (d - chunk * kKnnKC + 7) / 8;
        if (ngroup > kKnnKC / 8) ngroup = kKnnKC / 8;
        for (int kg = 0; kg < ngroup; ++kg) {
          const float4_t a = *reinterpret_cast<const float4_t*>(As + (wq * 32 + l31) * kKnnLd + kg * 8 + 4 * h);
          float4_t bf[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b)
            bf[b] = *reinterpret_cast<const float4_t*>(Bs + ((cb0 + b) * 32 + l31) * kKnnLd + kg * 8 + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int b = 0; b < NB; ++b)
              acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], bf[b][e], acc[b], 0, 0, 0);
        }
      }

      // scores to LDS; flag the queries with a score at or under their threshold
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int j = (cb0 + b) * 32 + l31;
        const bool rv = x0 + j < n;
        const float xv = xns[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = wq * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          const float s = rv ? fmaf(-2.f, acc[b][r], xv) : inf;
          sc[i * kKnnScLd + j] = s;
          if (rv && s <= st_td[i]) qflag[i] = 1;
        }
      }
      __syncthreads();

      // selection: wave w owns queries [w * QW, (w + 1) * QW)
      const int myq = w * QW + lane;
      const bool flagged = lane < QW && qflag[myq] != 0;
      if (flagged) qflag[myq] = 0;
      uint64_t qm = __ballot(flagged);
      const int toff = static_cast<int>(x0 - r_begin);
      while (qm) {
        const int qq = __ffsll(static_cast<unsigned long long>(qm)) - 1;
        qm &= qm - 1;
        const int ql = w * QW + qq;
        if (q0 + ql >= nq) break;
        int c = st_c[ql];
        float td = st_td[ql];
        int to = st_to[ql];
        const float s = sc[ql * kKnnScLd + lane];
        knn_wave_select(s, toff + lane, x0 + lane < n, ld + static_cast<size_t>(ql) * k,
                        lo + static_cast<size_t>(ql) * k, k, c, td, to);
        if (lane == 0) {
          st_c[ql] = c;
          st_td[ql] = td;
          st_to[ql] = to;
        }
      }
    }

    // write the partial lists of this (query tile, split): each wave its own queries
    __syncthreads();
    for (int qq = 0; qq < QW; ++qq) {
      const int ql = w * QW + qq;
      const int64_t qg = q0 + ql;
      if (qg >= nq) break;
      const int c = st_c[ql];
      const int64_t base = (qg * S + split) * k;
      for (int j = lane; j < k; j += 64) {
        const bool has = j < c;
        pd[base + j] = has ? ld[static_cast<size_t>(ql) * k + j] : inf;
        pr[base + j] = has ? r_begin + lo[static_cast<size_t>(ql) * k + j] : int64_t{-1};
      }
    }
  }
}

template <int TQ>
size_t knn_flat_lds(int k) {
  return sizeof(float) * (static_cast<size_t>(TQ) * kKnnLd + kKnnTR * kKnnLd + kKnnTR + TQ * kKnnScLd + 4 * TQ +
                          2 * static_cast<size_t>(TQ) * k);
}

// ---------------------------------------------------------------------------------- IVF
template <bool VEC>
__global__ __launch_bounds__(kKnnThreads) void knn_ivf_scan_kernel(const float* __restrict__ Q,
                                                                   const float* __restrict__ XS,
                                                                   const float* __restrict__ xn,
                                                                   const int64_t* __restrict__ list_ptr,
                                                                   const int64_t* __restrict__ row_of,
                                                                   const int64_t* __restrict__ probe, int64_t nq,
                                                                   int64_t n, int64_t ncent, int nprobe, int d, int k,
                                                                   float* __restrict__ pd, int64_t* __restrict__ pr) {
  extern __shared__ __align__(16) float knn_smem[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* ld = knn_smem + static_cast<size_t>(w) * 2 * k;
  int* lo = reinterpret_cast<int*>(ld + k);
  const float inf = __builtin_inff();
  const int64_t items = nq * nprobe;
  const int64_t step = static_cast<int64_t>(gridDim.x) * (kKnnThreads / 64);

  for (int64_t item = static_cast<int64_t>(blockIdx.x) * (kKnnThreads / 64) + w; item < items; item += step) {
    const int64_t qi = item / nprobe;
    const int64_t list = probe[item];
    int64_t b = 0, e = 0;
    if (list >= 0 && list < ncent) {
      b = list_ptr[list];
      e = list_ptr[list + 1];
      if (b < 0) b = 0;
      if (e > n) e = n;
      if (e - b > INT_MAX - 64) e = b + (INT_MAX - 64);  // offsets inside a list are 32-bit
    }
    const float* q = Q + qi * d;
    float4_t qv0 = {0.f, 0.f, 0.f, 0.f};
    float qs0 = 0.f;
    if (VEC) {
      if (4 * lane < d) qv0 = *reinterpret_cast<const float4_t*>(q + 4 * lane);
    } else {
      if (lane < d) qs0 = q[lane];
    }
    int c = 0, to = INT_MAX;
    float td = inf;
    for (int64_t base = b; base < e; base += 64) {
      const int cnt = e - base < 64 ? static_cast<int>(e - base) : 64;
      float mine = 0.f;
      for (int r0 = 0; r0 < cnt; r0 += 4) {
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
          for (int kk = 4 * lane; kk < d; kk += 256) {
            const float4_t qv = kk < 256 ? qv0 : *reinterpret_cast<const float4_t*>(q + kk);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              if (r0 + u < cnt) {
                const float4_t xv = *reinterpret_cast<const float4_t*>(XS + (base + r0 + u) * d + kk);
                part[u] = fmaf(qv[0], xv[0], fmaf(qv[1], xv[1], fmaf(qv[2], xv[2], fmaf(qv[3], xv[3], part[u]))));
              }
            }
          }
        } else {
          for (int kk = lane; kk < d; kk += 64) {
            const float qv = kk < 64 ? qs0 : q[kk];
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (r0 + u < cnt) part[u] = fmaf(qv, XS[(base + r0 + u) * d + kk], part[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float v = part[u];
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
          if (lane == r0 + u) mine = v;
        }
      }
      const bool valid = lane < cnt;
      const float s = valid ? fmaf(-2.f, mine, xn[base + lane]) : inf;
      knn_wave_select(s, static_cast<int>(base - b) + lane, valid, ld, lo, k, c, td, to);
    }
    const int64_t ob = item * k;
    for (int j = lane; j < k; j += 64) {
      const bool has = j < c;
      pd[ob + j] = has ? ld[j] : inf;
      pr[ob + j] = has ? row_of[b + lo[j]] : int64_t{-1};
    }
  }
}

// ---------------------------------------------------------------------------------- merge
// one wave per query; lane l walks the sorted partial of split l
__global__ __launch_bounds__(kKnnThreads) void knn_merge_kernel(const float* __restrict__ pd,
                                                                const int64_t* __restrict__ pr,
                                                                const float* __restrict__ qn, int64_t nq, int S,
                                                                int k, float* __restrict__ D,
                                                                int64_t* __restrict__ I) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float inf = __builtin_inff();
  const int64_t step = static_cast<int64_t>(gridDim.x) * (kKnnThreads / 64);
  for (int64_t qi = static_cast<int64_t>(blockIdx.x) * (kKnnThreads / 64) + w; qi < nq; qi += step) {
    const int64_t base = (qi * S + lane) * k;
    int ptr = 0;
    float hd = inf;
    int64_t hr = LLONG_MAX;
    auto fetch = [&]() {
      hd = inf;
      hr = LLONG_MAX;
      if (lane < S && ptr < k) {
        const int64_t r = pr[base + ptr];
        if (r >= 0) {
          hd = pd[base + ptr];
          hr = r;
        }
      }
    };
    fetch();
    const float qq = qn[qi];
    for (int j = 0; j < k; ++j) {
      float bd = hd;
      int64_t br = hr;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float od = __shfl_xor(bd, o);
        const int64_t orow = __shfl_xor(br, o);
        if (od < bd || (od == bd && orow < br)) {
          bd = od;
          br = orow;
        }
      }
      const bool none = br == LLONG_MAX;
      if (lane == 0) {
        D[qi * k + j] = none ? inf : fmaxf(bd + qq, 0.f);
        I[qi * k + j] = none ? int64_t{-1} : br;
      }
      // a row sits in one partial only, unless a list is probed twice: the lowest lane gives it up
      const uint64_t owners = __ballot(!none && hr == br && hd == bd);
      if (owners && lane == __ffsll(static_cast<unsigned long long>(owners)) - 1) {
        ++ptr;
        fetch();
      }
    }
  }
}

int knn_grid(int64_t blocks, int64_t cap) {
  if (blocks < 1) blocks = 1;
  return static_cast<int>(blocks < cap ? blocks : cap);
}

}  // namespace

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

hipError_t eh_knn_flat_scan(const float* Q, const float* X, const float* xn, int64_t nq, int64_t n, int d, int k,
                            int S, float* pd, int64_t* pr, hipStream_t s) {
  if (nq <= 0 || n <= 0 || d < 1 || k < 1 || k > kKnnMaxK || S < 1 || S > kKnnMaxSplits) return hipErrorInvalidValue;
  const int64_t ntiles = ceil_div(n, kKnnTR);
  const int64_t tps = ceil_div(ntiles, S);
  if (tps * kKnnTR > INT_MAX - kKnnTR) return hipErrorInvalidValue;  // offsets inside a split are 32-bit
  const bool vec = d % 4 == 0 && reinterpret_cast<uintptr_t>(Q) % 16 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0;
  const bool wide = k <= 32;  // 128-query tiles while the lists fit beside two resident blocks
  const int64_t nqt = ceil_div(nq, wide ? 128 : 64);
  const int64_t items = nqt * S;
  const int grid = knn_grid(items, 4096);
#define EH_KNN_FLAT(TQ, V)                                                                                     \
  do {                                                                                                         \
    const size_t lds = knn_flat_lds<TQ>(k);                                                                    \
    if (lds > 65536)                                                                                           \
      EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_flat_scan_kernel<TQ, V>),          \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds))); \
    hipLaunchKernelGGL((knn_flat_scan_kernel<TQ, V>), dim3(grid), dim3(kKnnThreads), lds, s, Q, X, xn, nq, n, d, k, \
                       S, tps, items, pd, pr);                                                                 \
  } while (0)
  if (wide) {
    if (vec) EH_KNN_FLAT(128, true); else EH_KNN_FLAT(128, false);
  } else {
    if (vec) EH_KNN_FLAT(64, true); else EH_KNN_FLAT(64, false);
  }
#undef EH_KNN_FLAT
  return hipGetLastError();
}

hipError_t eh_knn_ivf_scan(const float* Q, const float* XS, const float* xn, const int64_t* list_ptr,
                           const int64_t* row_of, const int64_t* probe, int64_t nq, int64_t n, int64_t ncent,
                           int nprobe, int d, int k, float* pd, int64_t* pr, hipStream_t s) {
  if (nq <= 0 || n < 0 || ncent < 1 || nprobe < 1 || nprobe > kKnnMaxSplits || d < 1 || k < 1 || k > kKnnMaxK)
    return hipErrorInvalidValue;
  const bool vec = d % 4 == 0 && reinterpret_cast<uintptr_t>(Q) % 16 == 0 && reinterpret_cast<uintptr_t>(XS) % 16 == 0;
  const int grid = knn_grid(ceil_div(nq * nprobe, kKnnThreads / 64), 1 << 16);
  const size_t lds = sizeof(float) * 2 * k * (kKnnThreads / 64);
  if (vec)
    hipLaunchKernelGGL(knn_ivf_scan_kernel<true>, dim3(grid), dim3(kKnnThreads), lds, s, Q, XS, xn, list_ptr, row_of,
                       probe, nq, n, ncent, nprobe, d, k, pd, pr);
  else
    hipLaunchKernelGGL(knn_ivf_scan_kernel<false>, dim3(grid), dim3(kKnnThreads), lds, s, Q, XS, xn, list_ptr, row_of,
                       probe, nq, n, ncent, nprobe, d, k, pd, pr);
  return hipGetLastError();
}

hipError_t eh_knn_merge(const float* pd, const int64_t* pr, const float* qn, int64_t nq, int S, int k, float* D,
                        int64_t* I, hipStream_t s) {
  if (nq <= 0 || S < 1 || S > kKnnMaxSplits || k < 1) return hipErrorInvalidValue;
  const int grid = knn_grid(ceil_div(nq, kKnnThreads / 64), 1 << 16);
  hipLaunchKernelGGL(knn_merge_kernel, dim3(grid), dim3(kKnnThreads), 0, s, pd, pr, qn, nq, S, k, D, I);
  return hipGetLastError();
}

int eh_knn_max_k() { return kKnnMaxK; }
int eh_knn_max_splits() { return kKnnMaxSplits; }

}  // extern "C"
