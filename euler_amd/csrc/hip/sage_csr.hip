// Full-neighbourhood GraphSAGE layer over the HBM graph's own CSR: the
// layer-wise inference kernel behind euler_amd.ops.sage_csr_ops / models.sage_infer.
//
//   agg[m] = sum_{t in mask} sum_{e in seg(row_m, t)} (w_e / sum w_e) * x[nbr_e]     (fp32; 0 without weight)
//   A[m]   = bf16([ x[row_m] | nbr_scale * agg[m] + self_scale * x[row_m] ])         ([64, 2 Dp], LDS only)
//   out[m] = act(A[m] @ W^T)                                                         (W [Hp, 2 Dp] bf16 row-major)
//
// w_e = cumw[e] - cumw[e - 1] inside its (row, type) segment: the graph stores per-segment
// prefix sums (the sampler's binary-search operand, tree_dev.h tr_neighbor), and agg is
// the expectation of the sampled mean aggregator.  The denominator is the segments' total
// weight, as the sampler's: an edge whose neighbour is outside [0, N) keeps its weight there
// and contributes a zero row (the sampler's -1 draw).
//
// One workgroup = 8 waves = 64 target rows, walked with a block-stride loop (8 waves, not 4: the
// gather is a chain of dependent loads per target, so the waves in flight set its rate, and
// the narrower per-wave GEMM tile keeps the registers at 4 waves per SIMD).
//   phase 0  one thread per target row: row id, edge count and total weight into LDS;
//   phase 1  gather: LPR = cpr rounded up to a power of two lanes cover one feature row with
//            16-byte loads (cpr = Dp / 8 chunks), so a wave holds NG = 64 / LPR lane groups and
//            each group takes every NG-th edge, kCsrUnroll edges in flight per lane.  The
//            groups' fp32 partial sums are added by an xor butterfly (every lane gets the same
//            sum in a fixed order).  A row with more than kCsrHubDeg edges is gathered by all
//            eight waves; their partial sums go through LDS and are added in wave order;
//   phase 2  MFMA GEMM out of the LDS A tile.  The operands are swapped (W fragment as A, tile
//            fragment as B), so a lane's four accumulators are four consecutive output columns
//            of one row: one 8-byte (bf16) or 16-byte (fp32) store.
// No atomics: two launches on the same inputs are bit-identical.
//
// The table x either has one row per graph row (RowIdentity) or holds the rows of a row set in
// list order and is addressed through the set's rank bitmap (RowRank, csr_rowset.h): the
// row -> table-position step is a template functor, everything else is the same code, so the
// two give the same bits for the same input rows.  A row the set lacks is never read: it counts
// as a zero row and is reported through a status word (the only atomic, on the error path).
#include "hip/csr_rowset.h"
#include "hip/tile.h"

namespace euler_hip {

constexpr int kCsrBM = 64;
constexpr int kCsrThreads = 512;
constexpr int kCsrWaves = kCsrThreads / 64;
constexpr int kCsrUnroll = 2;
constexpr int kCsrMaxD = 512;

struct CsrGraph {
  const int64_t* indptr;  // [N * T + 1]
  const int32_t* nbr;     // [E]
  const float* cumw;      // [E] prefix sums per (row, type) segment
  int64_t N, E;
  int T;
  uint32_t mask;
};

// 8 consecutive features of a row as fp32 (+ the storage bits for a bf16 table)
__device__ __forceinline__ void csr_load8(const bf16_t* p, float* v) {
  const uint4_t u = *reinterpret_cast<const uint4_t*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(u[i] << 16);
    v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ void csr_load8(const float* p, float* v) {
  const float4_t a = *reinterpret_cast<const float4_t*>(p);
  const float4_t b = *reinterpret_cast<const float4_t*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = a[i];
    v[4 + i] = b[i];
  }
}

// this lane group's share (edges slot, slot + nslots, ...) of row's masked segments:
// acc[8] += (w_e / tot) * x[nbr_e][8c .. 8c + 7] — the row of the row-normalised adjacency, edge
// by edge (tot > 0: rows without weight are not gathered)
template <typename XT, typename MAP>
__device__ __forceinline__ void csr_accum(const CsrGraph& g, const XT* __restrict__ x, const MAP& pos_of, int Dp,
                                          int64_t row, float tot, int slot, int nslots, int c, bool lane_on,
                                          float* acc) {
  const int64_t base = row * g.T;
  for (int t = 0; t < g.T; ++t) {
    if (!((g.mask >> t) & 1u)) continue;
    int64_t a = g.indptr[base + t], b = g.indptr[base + t + 1];
    a = a < 0 ? 0 : a;
    b = b > g.E ? g.E : b;
    for (int64_t e0 = a + slot; e0 < b; e0 += static_cast<int64_t>(nslots) * kCsrUnroll) {
      int32_t j[kCsrUnroll];
      float w[kCsrUnroll];
      float v[kCsrUnroll][8];
#pragma unroll
      for (int u = 0; u < kCsrUnroll; ++u) {
        const int64_t e = e0 + static_cast<int64_t>(u) * nslots;
        j[u] = -1;
        w[u] = 0.f;
        if (e < b) {
          j[u] = g.nbr[e];
          w[u] = (g.cumw[e] - (e > a ? g.cumw[e - 1] : 0.f)) / tot;
        }
      }
#pragma unroll
      for (int u = 0; u < kCsrUnroll; ++u) {
        // the neighbour's row of x: graph row j itself, or its position in a row set's table
        // (csr_rowset.h; -1: the set lacks the row, which then reads nothing)
        const bool ok = lane_on && j[u] >= 0 && static_cast<int64_t>(j[u]) < g.N;
        int64_t p = -1;
        if (ok) p = pos_of(static_cast<int64_t>(j[u]));
        if (MAP::found(ok, p)) {
          csr_load8(x + p * Dp + c * 8, v[u]);
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) v[u][i] = 0.f;
          w[u] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < kCsrUnroll; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += w[u] * v[u][i];
    }
  }
}

// the A-tile row of one target: [ x_self | nbr_scale * acc + self_scale * x_self ], every
// product and the sum rounded to fp32 on its own (no fma contraction: the documented order)
template <typename XT, typename MAP>
__device__ __forceinline__ void csr_finish(const XT* __restrict__ x, const MAP& pos_of, int Dp, int64_t row,
                                           const float* acc, float nbr_scale, float self_scale, bf16_t* arow, int c) {
  float xs[8], o[8];
  const int64_t p = pos_of(row);
  if (MAP::found(true, p)) {
    csr_load8(x + p * Dp + c * 8, xs);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) xs[i] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = __fadd_rn(__fmul_rn(nbr_scale, acc[i]), __fmul_rn(self_scale, xs[i]));
  *reinterpret_cast<uint4_t*>(arow + c * 8) = pack_bf16x8(xs);
  *reinterpret_cast<uint4_t*>(arow + Dp + c * 8) = pack_bf16x8(o);
}

template <typename XT, typename MAP>
__device__ __forceinline__ void csr_gather_tile(const CsrGraph& g, const XT* __restrict__ x, const MAP& pos_of, int Dp,
                                                const int32_t* __restrict__ rows, int64_t M, int64_t row0,
                                                float nbr_scale, float self_scale, bf16_t* lds, int ldsw, float* part,
                                                int32_t* m_row, int32_t* m_deg, float* m_tot) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cpr = Dp >> 3;
  int lpr = 1;
  while (lpr < cpr) lpr <<= 1;  // cpr <= 64
  const int ng = 64 / lpr;
  const int grp = lane / lpr, c = lane - grp * lpr;
  const bool lane_on = c < cpr;

  // phase 0: per-target metadata
  if (threadIdx.x < kCsrBM) {
    const int64_t m = row0 + threadIdx.x;
    int64_t r = -1;
    if (m < M) r = rows ? static_cast<int64_t>(rows[m]) : m;
    if (r < 0 || r >= g.N) r = -1;
    int64_t deg = 0;
    float tot = 0.f;
    if (r >= 0) {
      for (int t = 0; t < g.T; ++t) {
        if (!((g.mask >> t) & 1u)) continue;
        int64_t a = g.indptr[r * g.T + t], b = g.indptr[r * g.T + t + 1];
        a = a < 0 ? 0 : a;
        b = b > g.E ? g.E : b;
        if (b > a) {
          deg += b - a;
          tot += g.cumw[b - 1];
        }
      }
    }
    m_row[threadIdx.x] = static_cast<int32_t>(r);
    m_deg[threadIdx.x] = deg > INT32_MAX ? INT32_MAX : static_cast<int32_t>(deg);
    m_tot[threadIdx.x] = tot;
  }
  __syncthreads();

  // phase 1a: every wave gathers its own 16 targets (the hubs are left to 1b)
  for (int i = 0; i < kCsrBM / kCsrWaves; ++i) {
    const int p = wave * (kCsrBM / kCsrWaves) + i;
    const int64_t r = m_row[p];
    const int deg = m_deg[p];
    bf16_t* arow = lds + p * ldsw;
    if (r < 0) {  // no such row: a zero A row, a zero output row
      if (grp == 0 && lane_on) {
        *reinterpret_cast<uint4_t*>(arow + c * 8) = uint4_t{0u, 0u, 0u, 0u};
        *reinterpret_cast<uint4_t*>(arow + Dp + c * 8) = uint4_t{0u, 0u, 0u, 0u};
      }
      continue;
    }
    if (deg > kCsrHubDeg) continue;
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    const float tot = m_tot[p];
    if (deg > 0 && tot > 0.f) {
      csr_accum(g, x, pos_of, Dp, r, tot, grp, ng, c, lane_on, acc);
      for (int o = lpr; o < 64; o <<= 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += __shfl_xor(acc[q], o, 64);
      }
    }
    if (grp == 0 && lane_on) csr_finish(x, pos_of, Dp, r, acc, nbr_scale, self_scale, arow, c);
  }

  // phase 1b: hub targets, all waves on one row (block-uniform loop: m_deg is in LDS)
  for (int p = 0; p < kCsrBM; ++p) {
    if (m_row[p] < 0 || m_deg[p] <= kCsrHubDeg) continue;
    const int64_t r = m_row[p];
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    const float tot = m_tot[p];
    if (tot > 0.f) csr_accum(g, x, pos_of, Dp, r, tot, wave * ng + grp, kCsrWaves * ng, c, lane_on, acc);
    for (int o = lpr; o < 64; o <<= 1) {
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += __shfl_xor(acc[q], o, 64);
    }
    if (grp == 0 && lane_on) {
#pragma unroll
      for (int q = 0; q < 8; ++q) part[wave * Dp + c * 8 + q] = acc[q];
    }
    __syncthreads();
    if (wave == 0 && grp == 0 && lane_on) {
      float s[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        s[q] = part[c * 8 + q];
        for (int w = 1; w < kCsrWaves; ++w) s[q] += part[w * Dp + c * 8 + q];
      }
      csr_finish(x, pos_of, Dp, r, s, nbr_scale, self_scale, lds + p * ldsw, c);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void csr_store4(bf16_t* p, float4_t v) {
  tl_uint2 o;
  o[0] = pack_bf16x2(v[0], v[1]);
  o[1] = pack_bf16x2(v[2], v[3]);
  *reinterpret_cast<tl_uint2*>(p) = o;
}

__device__ __forceinline__ void csr_store4(float* p, float4_t v) { *reinterpret_cast<float4_t*>(p) = v; }

// out[row0 .., :] = act(A_lds @ W^T); D = Wfrag x Afrag: lane holds columns 4 (lane >> 4) + j of
// its 16-column slab for tile row lane & 15
template <int BN, typename OT>
__device__ __forceinline__ void csr_gemm_tile(const bf16_t* lds, int ldsw, int K2, const bf16_t* __restrict__ W,
                                              int H, int64_t M, int64_t row0, int relu, OT* __restrict__ out) {
  constexpr int WN = 2;                // waves along N
  constexpr int FN = BN / (16 * WN);   // 16-column fragments per wave: 4, 2 for BN 128, 64
  constexpr int WM = kCsrWaves / WN;   // waves along M
  constexpr int RW = kCsrBM / WM;      // rows per wave: 16
  constexpr int FM = RW / 16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  for (int cchunk = 0; cchunk < H; cchunk += BN) {
    const int cb = cchunk + wn * (16 * FN);
    if (cb >= H) continue;  // wave-uniform (H % 64 == 0)
    float4_t acc[FM][FN];
    tl_zero<FM, FN>(acc);
    const bf16_t* wrow[FN];
#pragma unroll
    for (int n = 0; n < FN; ++n) wrow[n] = W + static_cast<int64_t>(cb + n * 16 + lr) * K2 + lk;
    // no register double buffer for the W fragments: the waves in flight hide the L2 latency,
    // and the registers saved keep the kernel at 4 waves per SIMD
    for (int k0 = 0; k0 < K2; k0 += 32) {
      uint4_t b[FN], a[FM];
#pragma unroll
      for (int n = 0; n < FN; ++n) b[n] = *reinterpret_cast<const uint4_t*>(wrow[n] + k0);
#pragma unroll
      for (int m = 0; m < FM; ++m)
        a[m] = *reinterpret_cast<const uint4_t*>(lds + (wm * RW + m * 16 + lr) * ldsw + k0 + lk);
#pragma unroll
      for (int m = 0; m < FM; ++m)
#pragma unroll
        for (int n = 0; n < FN; ++n) acc[m][n] = mfma16(b[n], a[m], acc[m][n]);
    }
#pragma unroll
    for (int m = 0; m < FM; ++m) {
      const int64_t row = row0 + wm * RW + m * 16 + lr;
      if (row >= M) continue;
#pragma unroll
      for (int n = 0; n < FN; ++n) {
        float4_t v = acc[m][n];
        if (relu) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], 0.f);
        }
        csr_store4(out + row * H + cb + n * 16 + (lane >> 4) * 4, v);
      }
    }
  }
}

template <int BN, typename XT, typename OT, typename MAP>
__global__ __launch_bounds__(kCsrThreads) void sage_csr_fwd_kernel(CsrGraph g, const XT* __restrict__ x, MAP pos_of,
                                                                  int Dp, const int32_t* __restrict__ rows, int64_t M,
                                                                  const bf16_t* __restrict__ W, int H,
                                                                  float nbr_scale, float self_scale, int relu,
                                                                  OT* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  const int ldsw = 2 * Dp + 8;
  float* part = reinterpret_cast<float*>(lds + kCsrBM * ldsw);
  int32_t* m_row = reinterpret_cast<int32_t*>(part + kCsrWaves * Dp);
  int32_t* m_deg = m_row + kCsrBM;
  float* m_tot = reinterpret_cast<float*>(m_deg + kCsrBM);
  const int64_t tiles = ceil_div(M, kCsrBM);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kCsrBM;
    csr_gather_tile(g, x, pos_of, Dp, rows, M, row0, nbr_scale, self_scale, lds, ldsw, part, m_row, m_deg, m_tot);
    __syncthreads();
    csr_gemm_tile<BN>(lds, ldsw, 2 * Dp, W, H, M, row0, relu, out);
    __syncthreads();  // the next tile overwrites the A tile and the metadata
  }
}

}  // namespace euler_hip

using namespace euler_hip;

namespace {

size_t csr_lds_bytes(int Dp) {
  return static_cast<size_t>(kCsrBM) * (2 * Dp + 8) * sizeof(bf16_t) + static_cast<size_t>(kCsrWaves) * Dp * 4 +
         static_cast<size_t>(kCsrBM) * 12;
}

template <int BN, typename XT, typename OT, typename MAP>
hipError_t csr_launch(const CsrGraph& g, const void* x, const MAP& pos_of, int Dp, const int32_t* rows, int64_t M,
                      const void* W, int H, float nbr_scale, float self_scale, int relu, void* out, hipStream_t s) {
  const size_t lds = csr_lds_bytes(Dp);
  auto* k = sage_csr_fwd_kernel<BN, XT, OT, MAP>;
  if (lds > 65536)
    EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(lds)));
  const int64_t tiles = ceil_div(M, kCsrBM);
  const dim3 grid(static_cast<uint32_t>(tiles < kMaxGridBlocks ? tiles : kMaxGridBlocks));
  hipLaunchKernelGGL(k, grid, dim3(kCsrThreads), lds, s, g, static_cast<const XT*>(x), pos_of, Dp, rows, M,
                     static_cast<const bf16_t*>(W), H, nbr_scale, self_scale, relu, static_cast<OT*>(out));
  return hipGetLastError();
}

template <typename XT, typename OT, typename MAP>
hipError_t csr_pick_bn(const CsrGraph& g, const void* x, const MAP& pos_of, int Dp, const int32_t* rows, int64_t M,
                       const void* W, int H, float nbr_scale, float self_scale, int relu, void* out, hipStream_t s) {
  // 128 columns per pass (two passes at H = 256): a 256-column pass needs more than the 128
  // registers of 4 waves per SIMD, and the gather's rate is set by the waves in flight
  if (H > 64) return csr_launch<128, XT, OT>(g, x, pos_of, Dp, rows, M, W, H, nbr_scale, self_scale, relu, out, s);
  return csr_launch<64, XT, OT>(g, x, pos_of, Dp, rows, M, W, H, nbr_scale, self_scale, relu, out, s);
}

// pos_of: where x keeps a graph row (RowIdentity: x has every row; RowRank: a set's table)
template <typename MAP>
hipError_t csr_dispatch(const CsrGraph& g, const void* x, int x_fp32, const MAP& pos_of, int Dp, const int32_t* rows,
                        int64_t M, const void* W, int Hp, float nbr_scale, float self_scale, int relu, void* out,
                        int out_fp32, hipStream_t s) {
  if (M == 0) return hipSuccess;
  if (Dp <= 0 || Dp % 16 != 0 || Dp > kCsrMaxD || Hp <= 0 || Hp % 64 != 0 || g.T < 1 || g.T > 32 || g.N < 0 ||
      g.E < 0 || M < 0)
    return hipErrorInvalidValue;
  if (x_fp32) {
    if (out_fp32)
      return csr_pick_bn<float, float>(g, x, pos_of, Dp, rows, M, W, Hp, nbr_scale, self_scale, relu, out, s);
    return csr_pick_bn<float, bf16_t>(g, x, pos_of, Dp, rows, M, W, Hp, nbr_scale, self_scale, relu, out, s);
  }
  if (out_fp32)
    return csr_pick_bn<bf16_t, float>(g, x, pos_of, Dp, rows, M, W, Hp, nbr_scale, self_scale, relu, out, s);
  return csr_pick_bn<bf16_t, bf16_t>(g, x, pos_of, Dp, rows, M, W, Hp, nbr_scale, self_scale, relu, out, s);
}

}  // namespace

extern "C" {

int eh_sage_csr_hub_degree() { return kCsrHubDeg; }

hipError_t eh_sage_csr_fwd(const int64_t* indptr, const int32_t* nbr, const float* cumw, int64_t N, int64_t E, int T,
                           uint32_t mask, const void* x, int x_fp32, int Dp, const int32_t* rows, int64_t M,
                           const void* W, int Hp, float nbr_scale, float self_scale, int relu, void* out,
                           int out_fp32, hipStream_t s) {
  const CsrGraph g{indptr, nbr, cumw, N, E, T, mask};
  return csr_dispatch(g, x, x_fp32, RowIdentity{}, Dp, rows, M, W, Hp, nbr_scale, self_scale, relu, out, out_fp32, s);
}

hipError_t eh_sage_csr_fwd_mapped(const int64_t* indptr, const int32_t* nbr, const float* cumw, int64_t N, int64_t E,
                                  int T, uint32_t mask, const void* x, int x_fp32, int Dp, const int32_t* set_words,
                                  int64_t count, int32_t* missing, const int32_t* rows, int64_t M, const void* W,
                                  int Hp, float nbr_scale, float self_scale, int relu, void* out, int out_fp32,
                                  hipStream_t s) {
  if (count < 0 || count > N || set_words == nullptr || missing == nullptr) return hipErrorInvalidValue;
  const CsrGraph g{indptr, nbr, cumw, N, E, T, mask};
  const RowRank pos_of{reinterpret_cast<const rs_uint2*>(set_words), static_cast<int32_t>(count), reinterpret_cast<uint32_t*>(missing)};
  return csr_dispatch(g, x, x_fp32, pos_of, Dp, rows, M, W, Hp, nbr_scale, self_scale, relu, out, out_fp32, s);
}

}  // extern "C"
