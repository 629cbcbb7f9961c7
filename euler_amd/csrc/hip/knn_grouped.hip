// IVF search grouped by list (ivf_topk(..., schedule="list")): the queries that probe a list scan it
// together, as a [queries of the list] x [rows of the list] GEMM on the matrix units, instead of one
// wave per (query, list) streaming the rows once per query (knn_ivf_scan / knn_ivf_scan_bf16).
// Ranking key, ordering rule and partial format are those of knn.hip; the partials pd / pr
// [nq, nprobe, k] are addressed by (query, slot), so knn_merge follows unchanged and nothing here
// depends on the order in which atomics land.  A pair is the flat index query * nprobe + slot of a
// probe entry (32-bit: nq * nprobe < 2^31).  Nothing is read back to the host: every size is bounded
// from nq, nprobe and ncent.
//
//   invert   seg_count (flow.hip) histograms the probe entries per list (integer atomics: exact in
//            any order; -1 and out-of-range entries fall out).  knn_grouped_build, one block, scans
//            the counts twice at once: qptr = exclusive sum of the counts, and the first work item
//            of a list = exclusive sum of ceil(count / TQ); it writes the items (list, first pair)
//            and their number, and zeroes the counts, which knn_grouped_fill then uses as cursors
//            to place every entry's pair into its list's group.  An entry that names no list gets
//            its partial (+inf / -1) from the fill, so every element of pd / pr is written exactly
//            once by the pipeline.  Items are in list order (a list's tiles adjacent, so they meet
//            in L2); they are not sorted by list length.
//   scan     knn_grouped_scan: one block (4 waves) per work item, a capped grid striding over the
//            item table up to the device-side count.  The block gathers the rows of its TQ = 64
//            queries through the pair table and streams the list's rows in tiles of 128.  Both
//            operands are staged in 128-byte row chunks (64 bf16 or 32 fp32 columns, zero past d,
//            row stride 144 bytes: conflict-free 16-byte reads, as in knn_bf16.hip), the next
//            chunk's global loads in flight under the current MFMAs.  The query tile stays whole
//            in LDS when it fits beside the lists (QRES); otherwise its chunk is re-gathered (from
//            L2) with every row tile's chunk.  The table is the A operand and the queries are B,
//            for v_mfma_f32_32x32x16_bf16 and v_mfma_f32_32x32x2_f32 alike, so a lane holds 16 rows
//            against one query: wave w takes rows 32 w .. 32 w + 31 of the tile against all 64
//            queries (two accumulators).  A lane tests its 16 scores against the query's threshold
//            in registers; only flagged queries send a 64-row half tile of scores through LDS
//            (aliasing the row staging buffer), where the owner wave (16 queries each) inserts
//            into the sorted k-best list (knn_wave_select; key (score, position in the list), so
//            equal scores go to the lower position whatever lane or tile they arrive in).  A score
//            depends on its row and its query alone, so a query's result does not depend on which
//            queries share its tile.
// One block scans a whole list for its query tile: a single very long list is serial per tile.
// Offsets inside a list are 32-bit: of a list longer than INT_MAX - 128 rows only the first
// INT_MAX - 128 are scanned, as in knn_ivf_scan (no table that fits the device comes near it).
#include "hip/common.h"
#include "hip/knn_dev.h"
#include "hip/launchers.h"

#include <limits.h>
#include <math.h>

namespace euler_hip {

namespace {

constexpr int kGrTQ = 64;             // queries per work item
constexpr int kGrTR = 128;            // rows of the list per tile
constexpr int kGrHR = 64;             // rows per score half tile
constexpr int kGrCB = 128;            // bytes of a row per LDS chunk
constexpr int kGrLd = kGrCB + 16;     // staging row stride (bytes)
constexpr int kGrScLd = kGrHR + 1;    // score row stride (floats)
constexpr int kGrBuildThreads = 1024;
constexpr size_t kGrLdsMax = 160 * 1024;

static_assert(kGrTQ * kGrScLd * 4 <= kGrTR * kGrLd, "the score half tile must fit the row staging buffer");

// ---------------------------------------------------------------------------------- invert
// cnt[l] = probe entries of list l on entry, 0 on exit
__global__ __launch_bounds__(kGrBuildThreads) void knn_grouped_build_kernel(unsigned long long* __restrict__ cnt,
                                                                           int ncent, int* __restrict__ qptr,
                                                                           int2* __restrict__ items,
                                                                           int* __restrict__ n_items) {
  __shared__ int wsum[2][kGrBuildThreads / 64];
  __shared__ int carry[2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry[0] = carry[1] = 0;
  __syncthreads();
  for (int l0 = 0; l0 < ncent; l0 += kGrBuildThreads) {
    const int l = l0 + tid;
    const bool in = l < ncent && l >= 0;
    const int c = in ? static_cast<int>(cnt[l]) : 0;
    if (in) cnt[l] = 0ull;
    const int t = (c + kGrTQ - 1) / kGrTQ;
    int sc = c, st = t;  // inclusive sums over the wave
    for (int o = 1; o < 64; o <<= 1) {
      const int a = __shfl_up(sc, o), b = __shfl_up(st, o);
      if (lane >= o) {
        sc += a;
        st += b;
      }
    }
    if (lane == 63) {
      wsum[0][w] = sc;
      wsum[1][w] = st;
    }
    __syncthreads();
    int p0 = carry[0] + sc - c, i0 = carry[1] + st - t;
    for (int i = 0; i < w; ++i) {
      p0 += wsum[0][i];
      i0 += wsum[1][i];
    }
    if (in) {
      qptr[l] = p0;
      for (int j = 0; j < t; ++j) items[i0 + j] = make_int2(l, p0 + j * kGrTQ);
    }
    __syncthreads();
    if (tid == kGrBuildThreads - 1) {
      carry[0] = p0 + c;
      carry[1] = i0 + t;
    }
    __syncthreads();
    if (l0 > INT_MAX - kGrBuildThreads) break;
  }
  if (tid == 0) {
    qptr[ncent] = carry[0];
    *n_items = carry[1];
  }
}

__global__ __launch_bounds__(256) void knn_grouped_fill_kernel(const int64_t* __restrict__ probe, int64_t total,
                                                               int64_t ncent, int k, const int* __restrict__ qptr,
                                                               unsigned long long* __restrict__ cur,
                                                               int* __restrict__ pairs, float* __restrict__ pd,
                                                               int64_t* __restrict__ pr) {
  const float inf = __builtin_inff();
  grid_stride(total, [&](int64_t e) {
    const int64_t l = probe[e];
    if (l >= 0 && l < ncent) {
      pairs[qptr[l] + static_cast<int>(atomicAdd(cur + l, 1ull))] = static_cast<int>(e);
    } else {
      for (int j = 0; j < k; ++j) {
        pd[e * k + j] = inf;
        pr[e * k + j] = -1;
      }
    }
  });
}

// ---------------------------------------------------------------------------------- scan
// the 16 bytes at byte column cb of a row of rowbytes bytes, zero past the row's end
template <bool BF, bool VEC>
__device__ __forceinline__ uint4_t kg_load16(const unsigned char* __restrict__ row, int cb, int rowbytes) {
  uint4_t v = {0u, 0u, 0u, 0u};
  if (cb >= rowbytes) return v;
  if constexpr (VEC) {
    v = *reinterpret_cast<const uint4_t*>(row + cb);
  } else if constexpr (BF) {
    v = kb_load8_scalar(reinterpret_cast<const bf16_t*>(row + cb), (rowbytes - cb) >> 1);
  } else {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(row + cb);
    const int valid = (rowbytes - cb) >> 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < valid ? p[e] : 0u;
  }
  return v;
}

// c += x . q over one 32-byte column group: lane l holds the bytes [16 (l >> 5), + 16) of the group of
// table row / query l & 31.  bf16: one 32x32x16 MFMA (k = 8 (l >> 5) .. + 7).  fp32: four 32x32x2 MFMAs,
// step e over the columns {e, 4 + e} of the group (k = l >> 5), the same permutation on both operands.
template <bool BF>
__device__ __forceinline__ float16_t kg_mma(uint4_t x, uint4_t q, float16_t c) {
  if constexpr (BF) {
    return knn_mfma_bf16(x, q, c);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(x[e]), __uint_as_float(q[e]), c, 0, 0, 0);
    return c;
  }
}

// the second launch bound is waves per SIMD (= blocks per CU)
template <bool BF, bool VEC, bool QRES>
__global__ __launch_bounds__(kKnnThreads, 3) void knn_grouped_scan_kernel(
    const unsigned char* __restrict__ Q, const unsigned char* __restrict__ XS, const float* __restrict__ xn,
    const int64_t* __restrict__ list_ptr, const int64_t* __restrict__ row_of, const int* __restrict__ qptr,
    const int* __restrict__ pairs, const int2* __restrict__ items, const int* __restrict__ n_items, int64_t n,
    int nprobe, int rowbytes, int k, int qld, float* __restrict__ pd, int64_t* __restrict__ pr) {
  // staged 16-byte units per thread and chunk: the row tile, and the query chunk unless resident
  constexpr int NU = (kGrTR + (QRES ? 0 : kGrTQ)) * (kGrCB / 16) / kKnnThreads;
  extern __shared__ __align__(16) unsigned char kg_smem[];
  unsigned char* Xs = kg_smem;                              // [128][kGrLd]
  float* sc = reinterpret_cast<float*>(kg_smem);            // [TQ][kGrScLd], over the row staging buffer
  unsigned char* Qs = Xs + kGrTR * kGrLd;                   // [TQ][qld]; a chunk [TQ][kGrLd] unless QRES
  const int qs = QRES ? qld : kGrLd;
  float* xns = reinterpret_cast<float*>(Qs + kGrTQ * qs);   // [128], +inf past the list's end
  const KnnSel<kGrTQ, 2, 2> st(xns + kGrTR, k);             // a flag per query and score half tile
  int* tq_pair = st.extra;                                  // [TQ] pair of the tile's query, -1 past its end
  int* tq_q = tq_pair + kGrTQ;                              // [TQ] its query

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int nchunk = (rowbytes + kGrCB - 1) / kGrCB;
  const float inf = __builtin_inff();
  const int nit = *n_items;

  for (int item = xcd_remap(blockIdx.x, gridDim.x); item < nit; item += gridDim.x) {
    const int2 it2 = items[item];
    const int p_begin = it2.y;
    int np = qptr[it2.x + 1] - p_begin;
    if (np > kGrTQ) np = kGrTQ;
    int64_t b, e;
    knn_list_range(list_ptr, it2.x, n, kGrTR, b, e);

    __syncthreads();  // the previous item's lists and state are written out
    st.reset();
    for (int i = tid; i < kGrTQ; i += kKnnThreads) {
      const int p = i < np ? pairs[p_begin + i] : -1;
      tq_pair[i] = p;
      tq_q[i] = p >= 0 ? p / nprobe : 0;
    }
    __syncthreads();
    if (QRES) {
      const int upr = nchunk * (kGrCB / 16);  // units per query row
      for (int u = tid; u < kGrTQ * upr; u += kKnnThreads) {
        const int row = u / upr, cb = (u - row * upr) * 16;
        uint4_t v = {0u, 0u, 0u, 0u};
        if (row < np) v = kg_load16<BF, VEC>(Q + static_cast<int64_t>(tq_q[row]) * rowbytes, cb, rowbytes);
        *reinterpret_cast<uint4_t*>(Qs + row * qld + cb) = v;
      }
    }

    uint4_t stage[NU];
    float stage_xn = 0.f;
    auto load_stage = [&](int64_t x0, int chunk) {
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int u = tid + kKnnThreads * i;
        const int row = u >> 3, cb = chunk * kGrCB + (u & 7) * 16;
        uint4_t v = {0u, 0u, 0u, 0u};
        if (QRES || row < kGrTR) {
          if (x0 + row < e) v = kg_load16<BF, VEC>(XS + (x0 + row) * rowbytes, cb, rowbytes);
        } else if (row - kGrTR < np) {
          v = kg_load16<BF, VEC>(Q + static_cast<int64_t>(tq_q[row - kGrTR]) * rowbytes, cb, rowbytes);
        }
        stage[i] = v;
      }
      if (chunk == 0 && tid < kGrTR) stage_xn = x0 + tid < e ? xn[x0 + tid] : inf;
    };
    auto store_stage = [&](int chunk) {
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int u = tid + kKnnThreads * i;
        // the query chunk follows the row tile with the same stride: rows 128.. are query rows
        *reinterpret_cast<uint4_t*>(Xs + (u >> 3) * kGrLd + (u & 7) * 16) = stage[i];
      }
      if (chunk == 0 && tid < kGrTR) xns[tid] = stage_xn;
    };

    if (b < e) load_stage(b, 0);
    for (int64_t x0 = b; x0 < e; x0 += kGrTR) {
      float16_t acc[2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

      for (int chunk = 0; chunk < nchunk; ++chunk) {
        __syncthreads();  // the previous chunk's operands (and the previous tile's scores) are consumed
        store_stage(chunk);
        __syncthreads();
        if (chunk + 1 < nchunk) {
          load_stage(x0, chunk + 1);
        } else if (x0 + kGrTR < e) {
          load_stage(x0 + kGrTR, 0);
        }
        int ng = (rowbytes - chunk * kGrCB + 31) / 32;
        if (ng > kGrCB / 32) ng = kGrCB / 32;
        const unsigned char* qb = Qs + (QRES ? chunk * kGrCB : 0) + l31 * qs + 16 * h;
        const unsigned char* xb = Xs + (w * 32 + l31) * kGrLd + 16 * h;
        for (int g = 0; g < ng; ++g) {
          const uint4_t xf = *reinterpret_cast<const uint4_t*>(xb + g * 32);
#pragma unroll
          for (int a = 0; a < 2; ++a)
            acc[a] = kg_mma<BF>(xf, *reinterpret_cast<const uint4_t*>(qb + a * 32 * qs + g * 32), acc[a]);
        }
      }

      // selection, 64 rows at a time: wave w's rows belong to half w >> 1
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const bool mine = (w >> 1) == hf;
        // a lane's scores of one accumulator are 16 rows against one query (KnnSel::tile_flag)
        if (mine) st.tile_flag(hf, acc[0], acc[1], xns + w * 32, l31);
        __syncthreads();  // flags are set; at hf = 0 the tile's last fragment reads are done too
        if (mine) st.tile_spill(hf, acc[0], acc[1], xns + w * 32, l31, sc + (w & 1) * 32, kGrScLd);
        __syncthreads();
        const int64_t h0 = x0 + hf * kGrHR;
        st.select(hf, sc, kGrScLd, 0, np, static_cast<int>(h0 - b), 0, knn_count(e - h0, kGrHR));
      }
    }

    // write the partial list of every pair of the tile
    __syncthreads();
    st.write_back(0, np, pd, pr, [&](int ql) { return static_cast<int64_t>(tq_pair[ql]) * k; }, KnnRowOf{row_of, b});
  }
}

}  // namespace

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

int eh_knn_grouped_tq() { return kGrTQ; }

int64_t eh_knn_grouped_max_items(int64_t nq, int nprobe, int64_t ncent) {
  return nq * nprobe / kGrTQ + ncent;  // a list with c entries has ceil(c / TQ) <= c / TQ + 1 items
}

hipError_t eh_knn_grouped_invert(const int64_t* probe, int64_t nq, int nprobe, int64_t ncent, int k, int64_t* cnt,
                                 int32_t* qptr, int32_t* pairs, int32_t* items, int32_t* n_items, float* pd,
                                 int64_t* pr, hipStream_t s) {
  if (nq <= 0 || nprobe < 1 || nprobe > kKnnMaxSplits || ncent < 1 || ncent >= INT_MAX || k < 1 || k > kKnnMaxK ||
      nq > INT_MAX / nprobe)
    return hipErrorInvalidValue;
  const int64_t total = nq * nprobe;
  EULER_HIP_CHECK(eh_seg_count(probe, total, ncent, cnt, s));
  hipLaunchKernelGGL(knn_grouped_build_kernel, dim3(1), dim3(kGrBuildThreads), 0, s,
                     reinterpret_cast<unsigned long long*>(cnt), static_cast<int>(ncent), qptr,
                     reinterpret_cast<int2*>(items), n_items);
  EULER_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(knn_grouped_fill_kernel, grid_for(total), dim3(256), 0, s, probe, total, ncent, k, qptr,
                     reinterpret_cast<unsigned long long*>(cnt), pairs, pd, pr);
  return hipGetLastError();
}

hipError_t eh_knn_grouped_scan(const void* Q, const void* XS, int bf16, const float* xn, const int64_t* list_ptr,
                               const int64_t* row_of, const int32_t* qptr, const int32_t* pairs, const int32_t* items,
                               const int32_t* n_items, int64_t max_items, int64_t nq, int64_t n, int64_t ncent,
                               int nprobe, int d, int k, float* pd, int64_t* pr, hipStream_t s) {
  const int es = bf16 ? 2 : 4;
  if (nq <= 0 || n < 0 || ncent < 1 || ncent >= INT_MAX || nprobe < 1 || nprobe > kKnnMaxSplits || d < 1 ||
      d > (INT_MAX - kGrCB) / es || k < 1 || k > kKnnMaxK || nq > INT_MAX / nprobe || max_items < 1)
    return hipErrorInvalidValue;
  const int rowbytes = d * es;
  const bool vec = rowbytes % 16 == 0 && knn_aligned16(Q) && knn_aligned16(XS);
  const int64_t qld = ceil_div(rowbytes, kGrCB) * kGrCB + 16;
  // row staging, norms, the selection state with the two words (pair, query) of this kernel
  const size_t base = static_cast<size_t>(kGrTR) * kGrLd + sizeof(float) * kGrTR + knn_sel_bytes(kGrTQ, 2, 2, k);
  const bool qres = base + static_cast<size_t>(kGrTQ) * qld <= kGrLdsMax;
  const size_t lds = base + static_cast<size_t>(kGrTQ) * (qres ? qld : kGrLd);
  const int grid = knn_grid(max_items, 4096);
  const unsigned char* q8 = static_cast<const unsigned char*>(Q);
  const unsigned char* x8 = static_cast<const unsigned char*>(XS);
#define EH_KNN_GROUPED(B, V, R)                                                                                   \
  do {                                                                                                            \
    if (lds > 65536)                                                                                              \
      EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_grouped_scan_kernel<B, V, R>),        \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));    \
    hipLaunchKernelGGL((knn_grouped_scan_kernel<B, V, R>), dim3(grid), dim3(kKnnThreads), lds, s, q8, x8, xn,     \
                       list_ptr, row_of, qptr, pairs, reinterpret_cast<const int2*>(items), n_items, n, nprobe,   \
                       rowbytes, k, static_cast<int>(qld), pd, pr);                                               \
  } while (0)
#define EH_KNN_GROUPED_VR(B)                                                     \
  do {                                                                           \
    if (vec) {                                                                   \
      if (qres) EH_KNN_GROUPED(B, true, true); else EH_KNN_GROUPED(B, true, false);   \
    } else {                                                                     \
      if (qres) EH_KNN_GROUPED(B, false, true); else EH_KNN_GROUPED(B, false, false); \
    }                                                                            \
  } while (0)
  if (bf16) EH_KNN_GROUPED_VR(true); else EH_KNN_GROUPED_VR(false);
#undef EH_KNN_GROUPED_VR
#undef EH_KNN_GROUPED
  return hipGetLastError();
}

}  // extern "C"
