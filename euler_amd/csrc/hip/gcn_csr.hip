// Full-neighbourhood GCN-family layer over the HBM graph's own CSR: the layer-wise inference
// kernel behind euler_amd.ops.gcn_csr_ops / models.gcn_infer.
//
//   s[m]   = sum_{t in mask} sum_{e in seg(row_m, t)} b[nbr_e] * x[nbr_e]  (+ b[row_m] * x[row_m] with self_loop)
//   A[m]   = bf16(a[row_m] * s[m])                                          ([128, Dp], LDS only)
//   out[m] = cast(c[row_m] * act(A[m] @ W^T))                               (W [Hp, Dp] bf16 row-major)
//
// a, b, c are the caller's fp32 per-row scale tables (b, c may be null: 1).  The kernel only
// multiplies: symmetric GCN normalisation is a = deg_t^-1/2, b = deg_s^-1/2 (or the source norm
// folded into the previous layer's output by its c, then b = null and an edge costs no scale
// load), an unnormalised sum is a = 1.  The sampler's prefix sums (cumw) are never read.
//
// What the narrower tile buys, against sage_csr.hip (A tile [64, 2 Dp], one cumw difference per
// edge), and what this kernel does with it:
//   * 128 target rows per workgroup, not 64.  The A tile is Dp wide, so twice the rows fit in
//     the LDS the SAGE tile takes (147 KB per workgroup at Dp = 512, 39 KB at Dp = 128, with the
//     hub partials and the row metadata).  Every W fragment a
//     wave reads from L2 now feeds two row fragments (FM = 2), which halves the W traffic per
//     output row, and a block amortises its two tile barriers over twice the gathers.
//   * three edges in flight per lane, not two.  An edge is one neighbour id, at most one scale
//     and one 16-byte row chunk: without the two cumw loads and the divide a third edge's loads
//     fit the 128 registers of 4 waves per SIMD (121-123 VGPRs; four edges take 137-149 and
//     drop the CU to one workgroup, profiles/gcn_infer/resource_usage.txt), and the gather is a
//     chain of dependent loads whose rate the loads in flight set.
// Overlapping the next tile's gather with this tile's MFMA phase was not chosen: the GEMM
// phase at H <= 128 is a few percent of a tile's time (K is Dp, not 2 Dp), and the second A
// tile would cost the LDS the 128 rows use.
//
//   phase 0  one thread per target row: row id and masked edge count into LDS;
//   phase 1  gather: LPR = Dp / 8 rounded up to a power of two lanes cover one table row with
//            16-byte loads, a wave holds NG = 64 / LPR lane groups, group g takes edges g,
//            g + NG, ... of the row, kGcnUnroll at a time.  The groups' fp32 partial sums are
//            added by an xor butterfly (a fixed order; every lane gets the same sum).  A row
//            with more than kCsrHubDeg edges is gathered by all eight waves; their partial
//            sums go through LDS and are added in wave order;
//   phase 2  MFMA GEMM out of the LDS tile, operands swapped (W fragment as A) so a lane holds
//            four consecutive output columns of one row: one 8- or 16-byte store after the
//            activation and the c scale.  Dp is a multiple of 16, the MFMA k step is 32: the
//            last step's upper half is fed zero fragments, never read.
// No atomics: two launches on the same inputs are bit-identical.  A neighbour outside [0, N)
// adds nothing; a target outside [0, N) is a zero output row (the binding refuses such a list).
//
// gcn_csr_degrees counts, for one edge-type mask, deg_t[r] = listed masked edges of row r and
// deg_s[j] = occurrences of row j in the masked neighbour lists (integer atomics: the result
// does not depend on their order).
#include "hip/csr_dev.h"
#include "hip/csr_rowset.h"

namespace euler_hip {

constexpr int kGcnBM = 128;
constexpr int kGcnThreads = 512;
constexpr int kGcnWaves = kGcnThreads / 64;
constexpr int kGcnUnroll = 3;
constexpr int kGcnBN = 64;  // output columns per GEMM pass (below)

struct GcnCsr {
  const int64_t* indptr;  // [N * T + 1]
  const int32_t* nbr;     // [E]
  int64_t N, E;
  int T;
  uint32_t mask;
};

// this lane group's share (edges slot, slot + nslots, ...) of row's masked segments:
// acc[8] += b[nbr_e] * x[nbr_e][8c .. 8c + 7]
template <typename XT>
__device__ __forceinline__ void gcn_accum(const GcnCsr& g, const XT* __restrict__ x, const float* __restrict__ bsc,
                                          int Dp, int64_t row, int slot, int nslots, int c, bool lane_on,
                                          float* acc) {
  const int64_t base = row * g.T;
  for (int t = 0; t < g.T; ++t) {
    if (!((g.mask >> t) & 1u)) continue;
    int64_t a = g.indptr[base + t], b = g.indptr[base + t + 1];
    a = a < 0 ? 0 : a;
    b = b > g.E ? g.E : b;
    for (int64_t e0 = a + slot; e0 < b; e0 += static_cast<int64_t>(nslots) * kGcnUnroll) {
      int32_t j[kGcnUnroll];
      float w[kGcnUnroll];
      float v[kGcnUnroll][8];
#pragma unroll
      for (int u = 0; u < kGcnUnroll; ++u) {
        const int64_t e = e0 + static_cast<int64_t>(u) * nslots;
        j[u] = e < b ? g.nbr[e] : -1;
      }
#pragma unroll
      for (int u = 0; u < kGcnUnroll; ++u) {
        if (lane_on && j[u] >= 0 && static_cast<int64_t>(j[u]) < g.N) {
          w[u] = bsc ? bsc[j[u]] : 1.f;
          csr_load8(x + static_cast<int64_t>(j[u]) * Dp + c * 8, v[u]);
        } else {
          w[u] = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) v[u][i] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < kGcnUnroll; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += w[u] * v[u][i];
    }
  }
}

// the A-tile row of one target: bf16(a[row] * (acc + b[row] * x[row])), the self term only with
// self_loop
template <typename XT>
__device__ __forceinline__ void gcn_finish(const XT* __restrict__ x, const float* __restrict__ asc,
                                           const float* __restrict__ bsc, int Dp, int64_t row, const float* acc,
                                           int self_loop, bf16_t* arow, int c) {
  float o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = acc[i];
  if (self_loop) {
    float xs[8];
    csr_load8(x + row * Dp + c * 8, xs);
    const float w = bsc ? bsc[row] : 1.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] += w * xs[i];
  }
  const float ar = asc[row];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] *= ar;
  *reinterpret_cast<uint4_t*>(arow + c * 8) = pack_bf16x8(o);
}

template <typename XT>
__device__ __forceinline__ void gcn_gather_tile(const GcnCsr& g, const XT* __restrict__ x,
                                                const float* __restrict__ asc, const float* __restrict__ bsc, int Dp,
                                                const int32_t* __restrict__ rows, int64_t row_start, int64_t M,
                                                int64_t row0, int self_loop, bf16_t* lds, int ldsw, float* part,
                                                int32_t* m_row, int32_t* m_deg) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cpr = Dp >> 3;
  int lpr = 1;
  while (lpr < cpr) lpr <<= 1;  // cpr <= 64
  const int ng = 64 / lpr;
  const int grp = lane / lpr, c = lane - grp * lpr;
  const bool lane_on = c < cpr;

  // phase 0: per-target metadata
  if (threadIdx.x < kGcnBM) {
    const int64_t m = row0 + threadIdx.x;
    int64_t r = -1;
    if (m < M) r = rows ? static_cast<int64_t>(rows[m]) : row_start + m;
    if (r < 0 || r >= g.N) r = -1;
    int64_t deg = 0;
    if (r >= 0) {
      for (int t = 0; t < g.T; ++t) {
        if (!((g.mask >> t) & 1u)) continue;
        int64_t a = g.indptr[r * g.T + t], b = g.indptr[r * g.T + t + 1];
        a = a < 0 ? 0 : a;
        b = b > g.E ? g.E : b;
        if (b > a) deg += b - a;
      }
    }
    m_row[threadIdx.x] = static_cast<int32_t>(r);
    m_deg[threadIdx.x] = deg > INT32_MAX ? INT32_MAX : static_cast<int32_t>(deg);
  }
  __syncthreads();

  // phase 1a: every wave gathers its own 16 targets (the hubs are left to 1b)
  for (int i = 0; i < kGcnBM / kGcnWaves; ++i) {
    const int p = wave * (kGcnBM / kGcnWaves) + i;
    const int64_t r = m_row[p];
    const int deg = m_deg[p];
    bf16_t* arow = lds + p * ldsw;
    if (r < 0) {  // no such row: a zero A row, a zero output row
      if (grp == 0 && lane_on) *reinterpret_cast<uint4_t*>(arow + c * 8) = uint4_t{0u, 0u, 0u, 0u};
      continue;
    }
    if (deg > kCsrHubDeg) continue;
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    if (deg > 0) {
      gcn_accum(g, x, bsc, Dp, r, grp, ng, c, lane_on, acc);
      for (int o = lpr; o < 64; o <<= 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += __shfl_xor(acc[q], o, 64);
      }
    }
    if (grp == 0 && lane_on) gcn_finish(x, asc, bsc, Dp, r, acc, self_loop, arow, c);
  }

  // phase 1b: hub targets, all waves on one row (block-uniform loop: m_deg is in LDS)
  for (int p = 0; p < kGcnBM; ++p) {
    if (m_row[p] < 0 || m_deg[p] <= kCsrHubDeg) continue;
    const int64_t r = m_row[p];
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    gcn_accum(g, x, bsc, Dp, r, wave * ng + grp, kGcnWaves * ng, c, lane_on, acc);
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
        for (int w = 1; w < kGcnWaves; ++w) s[q] += part[w * Dp + c * 8 + q];
      }
      gcn_finish(x, asc, bsc, Dp, r, s, self_loop, lds + p * ldsw, c);
    }
    __syncthreads();
  }
}

// out[row0 .., :] = c[row] * act(A_lds @ W^T); D = Wfrag x Afrag: a lane holds columns
// 4 (lane >> 4) + j of its 16-column slab for tile row lane & 15.  A wave owns 32 tile rows
// (two row fragments per W fragment) and BN / 2 of the pass's columns.  BN = kGcnBN = 64 (two
// passes at H = 128): with the two row fragments a 128-column pass holds 32 accumulators and
// six operand fragments, 141-149 VGPRs, which costs the gather its second workgroup per CU.
template <int BN, typename OT>
__device__ __forceinline__ void gcn_gemm_tile(const bf16_t* lds, int ldsw, int K, const bf16_t* __restrict__ W, int H,
                                              int64_t M, int64_t row0, int relu, const float* __restrict__ csc,
                                              const int32_t* m_row, OT* __restrict__ out) {
  constexpr int WN = 2;                // waves along N
  constexpr int FN = BN / (16 * WN);   // 16-column fragments per wave: 2
  constexpr int WM = kGcnWaves / WN;   // waves along M
  constexpr int RW = kGcnBM / WM;      // rows per wave: 32
  constexpr int FM = RW / 16;          // 2
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const uint4_t zero{0u, 0u, 0u, 0u};
  for (int cchunk = 0; cchunk < H; cchunk += BN) {
    const int cb = cchunk + wn * (16 * FN);
    if (cb >= H) continue;  // wave-uniform (H % 64 == 0)
    float4_t acc[FM][FN];
    tl_zero<FM, FN>(acc);
    const bf16_t* wrow[FN];
#pragma unroll
    for (int n = 0; n < FN; ++n) wrow[n] = W + static_cast<int64_t>(cb + n * 16 + lr) * K + lk;
    for (int k0 = 0; k0 < K; k0 += 32) {
      const bool in = k0 + lk < K;  // K % 16 == 0: a lane's 8 k values are all inside or all past K
      uint4_t b[FN], a[FM];
#pragma unroll
      for (int n = 0; n < FN; ++n) b[n] = in ? *reinterpret_cast<const uint4_t*>(wrow[n] + k0) : zero;
#pragma unroll
      for (int m = 0; m < FM; ++m)
        a[m] = in ? *reinterpret_cast<const uint4_t*>(lds + (wm * RW + m * 16 + lr) * ldsw + k0 + lk) : zero;
#pragma unroll
      for (int m = 0; m < FM; ++m)
#pragma unroll
        for (int n = 0; n < FN; ++n) acc[m][n] = mfma16(b[n], a[m], acc[m][n]);
    }
#pragma unroll
    for (int m = 0; m < FM; ++m) {
      const int p = wm * RW + m * 16 + lr;
      const int64_t row = row0 + p;
      if (row >= M) continue;
      const int32_t r = m_row[p];
      const float cs = (csc && r >= 0) ? csc[r] : 1.f;
#pragma unroll
      for (int n = 0; n < FN; ++n) {
        float4_t v = acc[m][n];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = cs * (relu ? fmaxf(v[q], 0.f) : v[q]);
        csr_store4(out + row * H + cb + n * 16 + (lane >> 4) * 4, v);
      }
    }
  }
}

template <int BN, typename XT, typename OT>
__global__ __launch_bounds__(kGcnThreads) void gcn_csr_fwd_kernel(GcnCsr g, const XT* __restrict__ x, int Dp,
                                                                 const float* __restrict__ asc,
                                                                 const float* __restrict__ bsc,
                                                                 const float* __restrict__ csc,
                                                                 const int32_t* __restrict__ rows, int64_t row_start,
                                                                 int64_t M, const bf16_t* __restrict__ W, int H,
                                                                 int self_loop, int relu, OT* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  const int ldsw = Dp + 8;
  float* part = reinterpret_cast<float*>(lds + kGcnBM * ldsw);
  int32_t* m_row = reinterpret_cast<int32_t*>(part + kGcnWaves * Dp);
  int32_t* m_deg = m_row + kGcnBM;
  const int64_t tiles = ceil_div(M, kGcnBM);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kGcnBM;
    gcn_gather_tile(g, x, asc, bsc, Dp, rows, row_start, M, row0, self_loop, lds, ldsw, part, m_row, m_deg);
    __syncthreads();
    gcn_gemm_tile<BN>(lds, ldsw, Dp, W, H, M, row0, relu, csc, m_row, out);
    __syncthreads();  // the next tile overwrites the A tile and the metadata
  }
}

// 8 lanes per row: deg_t from the offsets, one integer atomic per listed in-range neighbour
__global__ __launch_bounds__(256) void gcn_csr_degrees_kernel(GcnCsr g, int32_t* __restrict__ deg_t,
                                                             int32_t* __restrict__ deg_s) {
  grid_stride(g.N * 8, [&](int64_t t) {
    const int64_t row = t >> 3;
    const int sub = static_cast<int>(t & 7);
    int64_t cnt = 0;
    for (int ty = 0; ty < g.T; ++ty) {
      if (!((g.mask >> ty) & 1u)) continue;
      int64_t a = g.indptr[row * g.T + ty], b = g.indptr[row * g.T + ty + 1];
      a = a < 0 ? 0 : a;
      b = b > g.E ? g.E : b;
      if (b <= a) continue;
      cnt += b - a;
      for (int64_t e = a + sub; e < b; e += 8) {
        const int32_t j = g.nbr[e];
        if (j >= 0 && static_cast<int64_t>(j) < g.N) atomicAdd(deg_s + j, 1);
      }
    }
    if (sub == 0) deg_t[row] = cnt > INT32_MAX ? INT32_MAX : static_cast<int32_t>(cnt);
  });
}

}  // namespace euler_hip

using namespace euler_hip;

namespace {

size_t gcn_lds_bytes(int Dp) {
  return static_cast<size_t>(kGcnBM) * (Dp + 8) * sizeof(bf16_t) + static_cast<size_t>(kGcnWaves) * Dp * 4 +
         static_cast<size_t>(kGcnBM) * 8;
}

struct GcnCall {
  GcnCsr g;
  const void* x;
  int Dp;
  const float *a, *b, *c;
  const int32_t* rows;
  int64_t row_start, M;
  const void* W;
  int H, self_loop, relu;
  void* out;
};

template <int BN, typename XT, typename OT>
hipError_t gcn_launch(const GcnCall& k, hipStream_t s) {
  const size_t lds = gcn_lds_bytes(k.Dp);
  auto* fn = gcn_csr_fwd_kernel<BN, XT, OT>;
  if (lds > 65536)
    EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(lds)));
  const int64_t tiles = ceil_div(k.M, kGcnBM);
  const dim3 grid(static_cast<uint32_t>(tiles < kMaxGridBlocks ? tiles : kMaxGridBlocks));
  hipLaunchKernelGGL(fn, grid, dim3(kGcnThreads), lds, s, k.g, static_cast<const XT*>(k.x), k.Dp, k.a, k.b, k.c,
                     k.rows, k.row_start, k.M, static_cast<const bf16_t*>(k.W), k.H, k.self_loop, k.relu,
                     static_cast<OT*>(k.out));
  return hipGetLastError();
}

}  // namespace

extern "C" {

int eh_gcn_csr_tile_rows() { return kGcnBM; }

hipError_t eh_gcn_csr_fwd(const int64_t* indptr, const int32_t* nbr, int64_t N, int64_t E, int T, uint32_t mask,
                          const void* x, int x_fp32, int Dp, const float* tgt_scale, const float* src_scale,
                          const float* out_scale, const int32_t* rows, int64_t row_start, int64_t M, const void* W,
                          int Hp, int self_loop, int relu, void* out, int out_fp32, hipStream_t s) {
  if (M == 0) return hipSuccess;
  if (Dp <= 0 || Dp % 16 != 0 || Dp > kCsrMaxD || Hp <= 0 || Hp % 64 != 0 || T < 1 || T > 32 || N < 0 || E < 0 ||
      M < 0 || tgt_scale == nullptr || row_start < 0 || (rows == nullptr && row_start + M > N))
    return hipErrorInvalidValue;
  const GcnCall k{GcnCsr{indptr, nbr, N, E, T, mask}, x, Dp, tgt_scale, src_scale, out_scale, rows, row_start, M, W,
                  Hp, self_loop, relu, out};
  if (x_fp32) return out_fp32 ? gcn_launch<kGcnBN, float, float>(k, s) : gcn_launch<kGcnBN, float, bf16_t>(k, s);
  return out_fp32 ? gcn_launch<kGcnBN, bf16_t, float>(k, s) : gcn_launch<kGcnBN, bf16_t, bf16_t>(k, s);
}

hipError_t eh_gcn_csr_degrees(const int64_t* indptr, const int32_t* nbr, int64_t N, int64_t E, int T, uint32_t mask,
                              int32_t* deg_t, int32_t* deg_s, hipStream_t s) {
  if (N == 0) return hipSuccess;
  if (T < 1 || T > 32 || N < 0 || E < 0) return hipErrorInvalidValue;
  const GcnCsr g{indptr, nbr, N, E, T, mask};
  hipLaunchKernelGGL(gcn_csr_degrees_kernel, grid_for(N * 8), dim3(256), 0, s, g, deg_t, deg_s);
  return hipGetLastError();
}

}  // extern "C"
