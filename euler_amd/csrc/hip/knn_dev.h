// Everything the k-nearest-neighbour kernels share (knn.hip: fp32 tables, knn_bf16.hip: bf16 tables,
// knn_grouped.hip: the list-grouped IVF search over both), so the ordering rule is enforced in one
// place: the sorted k-best list in LDS with its threshold (knn_wave_select), the per-block selection
// state around it (KnnSel: LDS layout and size, reset, register-tile threshold test and spill, the
// owner waves' insertion pass), the partial write-back, the inverted-list clamp, the bf16 MFMA and
// the unaligned bf16 load, and the launchers' host side (grid cap, alignment test, the flat scan's
// validation and dispatch, the per-wave IVF scan's plan).
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

// where a sorted list's offsets point: a row range starting at r0, or the rows row_of[b ..] of an
// inverted list
struct KnnRowBase {
  int64_t r0;
  __device__ __forceinline__ int64_t operator()(int off) const { return r0 + off; }
};
struct KnnRowOf {
  const int64_t* __restrict__ row_of;
  int64_t b;
  __device__ __forceinline__ int64_t operator()(int off) const { return row_of[b + off]; }
};

// One wave writes a sorted list of c entries as the partial pd / pr [base, base + k), +inf / -1 past c.
template <typename Row>
__device__ __forceinline__ void knn_write_partial(const float* ld, const int* lo, int c, int k,
                                                  float* __restrict__ pd, int64_t* __restrict__ pr, int64_t base,
                                                  Row row) {
  for (int j = (threadIdx.x & 63); j < k; j += 64) {
    const bool has = j < c;
    pd[base + j] = has ? ld[j] : __builtin_inff();
    pr[base + j] = has ? row(lo[j]) : int64_t{-1};
  }
}

// Rows [b, e) of an inverted list, inside [0, n) and short enough that an offset from b plus one tile
// (margin rows) stays 32-bit.
__device__ __forceinline__ void knn_list_range(const int64_t* __restrict__ list_ptr, int64_t list, int64_t n,
                                               int margin, int64_t& b, int64_t& e) {
  b = list_ptr[list];
  e = list_ptr[list + 1];
  if (b < 0) b = 0;
  if (e > n) e = n;
  if (e - b > INT_MAX - margin) e = b + (INT_MAX - margin);
}

// how many of `cap` consecutive items are inside their range when `left` remain from the first (<= 0: none)
__device__ __forceinline__ int knn_count(int64_t left, int cap) { return static_cast<int>(left < cap ? left : cap); }

// row of a 32x32 MFMA C/D tile that register r of a lane in half h = lane >> 5 holds (column lane & 31)
__device__ __forceinline__ int knn_c_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Selection state of a block-tile scan kernel, in LDS: the sorted k-best lists of the block's TQ
// queries and, per query, the threshold (td, to), the entries held, one flag per score half tile
// (NH of them) and NX words of the kernel's own.  knn_sel_bytes is what a launcher adds to its
// kernel's staging buffers; the constructor carves the same words in the same order.
constexpr int knn_sel_words(int tq, int nh, int nx) { return tq * (3 + nh + nx); }  // ahead of the lists
constexpr size_t knn_sel_bytes(int tq, int nh, int nx, int k) {
  return sizeof(float) * (knn_sel_words(tq, nh, nx) + 2 * static_cast<size_t>(tq) * k);
}

template <int TQ, int NH, int NX = 0>
struct KnnSel {
  static constexpr int QW = TQ / (kKnnThreads / 64);  // queries owned per wave in the selection
  float* td;   // [TQ] threshold score
  int* to;     // [TQ] threshold offset
  int* c;      // [TQ] entries held
  int* flag;   // [NH][TQ] (half) tile has a candidate
  int* extra;  // [NX][TQ]
  float* ld;   // [TQ][k]
  int* lo;     // [TQ][k]
  int k;

  __device__ __forceinline__ KnnSel(float* base, int k_) : k(k_) {
    constexpr int o_to = TQ, o_c = o_to + TQ, o_flag = o_c + TQ, o_extra = o_flag + NH * TQ, o_list = o_extra + NX * TQ;
    static_assert(o_list == knn_sel_words(TQ, NH, NX), "the carve and knn_sel_bytes must count the same words");
    td = base;
    to = reinterpret_cast<int*>(base + o_to);
    c = reinterpret_cast<int*>(base + o_c);
    flag = reinterpret_cast<int*>(base + o_flag);
    extra = reinterpret_cast<int*>(base + o_extra);
    ld = base + o_list;
    lo = reinterpret_cast<int*>(ld + static_cast<size_t>(TQ) * k);
  }

  // empty lists, no flags; whole-block call
  __device__ __forceinline__ void reset() const {
    for (int i = threadIdx.x; i < TQ; i += kKnnThreads) {
      td[i] = __builtin_inff();
      to[i] = INT_MAX;
      c[i] = 0;
#pragma unroll
      for (int hf = 0; hf < NH; ++hf) flag[hf * TQ + i] = 0;
    }
  }

  // Threshold test of a register tile.  The lane holds, in a0 / a1, the dot products of the rows
  // knn_c_row(r, h) of a 32-row block (norms xn32) against the queries ql and ql + 32: flag a query of
  // half hf if the least of its 16 scores is at or under its threshold.  At hf = 1 no barrier separates
  // this read of td from the owners' hf = 0 insertions, on purpose: a threshold only falls, so a stale
  // one only flags a query that knn_wave_select then turns away; the test must stay `<=` against a
  // value that is never below the current threshold.
  __device__ __forceinline__ void tile_flag(int hf, const float16_t& a0, const float16_t& a1, const float* xn32,
                                            int ql) const {
    const int h = (threadIdx.x & 63) >> 5;
    float xv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) xv[r] = xn32[knn_c_row(r, h)];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float m = __builtin_inff();
#pragma unroll
      for (int r = 0; r < 16; ++r) m = fminf(m, fmaf(-2.f, a ? a1[r] : a0[r], xv[r]));
      if (m <= td[ql + 32 * a]) flag[hf * TQ + ql + 32 * a] = 1;
    }
  }

  // After a barrier: the flagged queries' scores of that block go to the score half tile, sc32 being
  // the block's first column of sc [TQ][scld].
  __device__ __forceinline__ void tile_spill(int hf, const float16_t& a0, const float16_t& a1, const float* xn32,
                                             int ql, float* sc32, int scld) const {
    const int h = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      if (flag[hf * TQ + ql + 32 * a] == 0) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = knn_c_row(r, h);
        sc32[(ql + 32 * a) * scld + i] = fmaf(-2.f, a ? a1[r] : a0[r], xn32[i]);
      }
    }
  }

  // Insertion pass over one score (half) tile sc [TQ][scld] of 64 rows: row j is r0 + j, in range
  // under nr, at offset toff + j; query ql is q0 + ql and exists under nq.  Wave w owns queries
  // [w * QW, (w + 1) * QW) and rescans the flagged ones.  The bounds come in the width the kernel holds
  // them in (global 64-bit indices, or 0 and a count clamped to 32 bits): which of the two costs fewer
  // scalar registers differs by kernel (profiles/knn_refactor).  Whole-block call after a barrier
  // behind the scores.
  template <typename QI, typename RI>
  __device__ __forceinline__ void select(int hf, const float* sc, int scld, QI q0, QI nq, int toff, RI r0,
                                         RI nr) const {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int* fl = flag + hf * TQ;
    const int myq = w * QW + lane;
    const bool flagged = lane < QW && fl[myq] != 0;
    if (flagged) fl[myq] = 0;
    uint64_t qm = __ballot(flagged);
    while (qm) {
      const int qq = __ffsll(static_cast<unsigned long long>(qm)) - 1;
      qm &= qm - 1;
      const int ql = w * QW + qq;
      if (q0 + ql >= nq) break;
      int cq = c[ql];
      float tdq = td[ql];
      int toq = to[ql];
      const float s = sc[ql * scld + lane];
      knn_wave_select(s, toff + lane, r0 + lane < nr, ld + static_cast<size_t>(ql) * k,
                      lo + static_cast<size_t>(ql) * k, k, cq, tdq, toq);
      if (lane == 0) {
        c[ql] = cq;
        td[ql] = tdq;
        to[ql] = toq;
      }
    }
  }

  // Each wave writes the lists of its queries that exist (q0 + ql under nq, as in select): query ql to
  // the partial at dst(ql), offsets mapped to rows by row.  Whole-block call after a barrier behind the
  // last insertion.
  template <typename QI, typename Dst, typename Row>
  __device__ __forceinline__ void write_back(QI q0, QI nq, float* __restrict__ pd, int64_t* __restrict__ pr,
                                             Dst dst, Row row) const {
    const int w = threadIdx.x >> 6;
    for (int qq = 0; qq < QW; ++qq) {
      const int ql = w * QW + qq;
      if (q0 + ql >= nq) break;
      knn_write_partial(ld + static_cast<size_t>(ql) * k, lo + static_cast<size_t>(ql) * k, c[ql], k, pd, pr, dst(ql),
                        row);
    }
  }
};

typedef __bf16 knn_bf16x8 __attribute__((ext_vector_type(8)));

// v_mfma_f32_32x32x16_bf16 over operands held as 16-byte vectors of raw bf16
__device__ __forceinline__ float16_t knn_mfma_bf16(uint4_t a, uint4_t b, float16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(knn_bf16x8, a), __builtin_bit_cast(knn_bf16x8, b),
                                                 c, 0, 0, 0);
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

// ---------------------------------------------------------------------------------- host
inline int knn_grid(int64_t blocks, int64_t cap) {
  if (blocks < 1) blocks = 1;
  return static_cast<int>(blocks < cap ? blocks : cap);
}

inline bool knn_aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// The flat scan of either dtype: kern[wide][vec] over row tiles of tile_rows, vector loads for rows
// that are multiples of vec_width elements at 16-byte aligned bases, lds_of(TQ, k) dynamic LDS bytes.
template <typename T>
using knn_flat_kernel_t = void (*)(const T*, const T*, const float*, int64_t, int64_t, int, int, int, int64_t,
                                   int64_t, float*, int64_t*);

template <typename T>
hipError_t knn_flat_launch(const knn_flat_kernel_t<T> (&kern)[2][2], int tile_rows, int vec_width,
                           size_t (*lds_of)(int, int), const T* Q, const T* X, const float* xn, int64_t nq,
                           int64_t n, int d, int k, int S, float* pd, int64_t* pr, hipStream_t s) {
  if (nq <= 0 || n <= 0 || d < 1 || k < 1 || k > kKnnMaxK || S < 1 || S > kKnnMaxSplits) return hipErrorInvalidValue;
  const int64_t ntiles = ceil_div(n, tile_rows);
  const int64_t tps = ceil_div(ntiles, S);
  if (tps * tile_rows > INT_MAX - tile_rows) return hipErrorInvalidValue;  // offsets inside a split are 32-bit
  const bool vec = d % vec_width == 0 && knn_aligned16(Q) && knn_aligned16(X);
  const bool wide = k <= 32;  // 128-query tiles while the lists leave room for two resident blocks
  const int tq = wide ? 128 : 64;
  const int64_t items = ceil_div(nq, tq) * S;
  const int grid = knn_grid(items, 4096);
  const knn_flat_kernel_t<T> fn = kern[wide][vec];
  const size_t lds = lds_of(tq, k);
  if (lds > 65536)
    EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(lds)));
  hipLaunchKernelGGL(fn, dim3(grid), dim3(kKnnThreads), lds, s, Q, X, xn, nq, n, d, k, S, tps, items, pd, pr);
  return hipGetLastError();
}

// The per-wave IVF scan of either dtype: validation, the choice of vector loads, grid and LDS bytes
// (one list of k (score, offset) per wave).
struct KnnIvfPlan {
  bool vec;
  int grid;
  size_t lds;
};
inline hipError_t knn_ivf_plan(const void* Q, const void* XS, int vec_width, int64_t nq, int64_t n, int64_t ncent,
                               int nprobe, int d, int k, KnnIvfPlan& p) {
  if (nq <= 0 || n < 0 || ncent < 1 || nprobe < 1 || nprobe > kKnnMaxSplits || d < 1 || k < 1 || k > kKnnMaxK)
    return hipErrorInvalidValue;
  p.vec = d % vec_width == 0 && knn_aligned16(Q) && knn_aligned16(XS);
  p.grid = knn_grid(ceil_div(nq * nprobe, kKnnThreads / 64), 1 << 16);
  p.lds = sizeof(float) * 2 * k * (kKnnThreads / 64);
  return hipSuccess;
}

}  // namespace euler_hip
