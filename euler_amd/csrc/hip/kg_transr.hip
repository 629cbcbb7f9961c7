// TransR scores (reference examples/TransX/transR.py):
//
//   kgr_fwd / kgr_bwd   P(x) = y / max(|y|, 1e-12) with y = x M_r (x the raw entity row [E], M_r
//       the relation's row-major [E, R] matrix), rho = r / max(|r|, 1e-12),
//       score = -| P(a) + rho - P(b) | in L1 or L2; positive (h, t), front (n_k, t), tail (h, n_k).
//
// The projection is a dense product, so unlike kgp_fwd / kgp_bwd (one lane group per triple) a
// whole block of 4 waves works on one triple:
//   * the triple's K + 2 entity rows (h, t, the K negatives; K <= 14) are ONE 16-row MFMA tile X,
//     rows K + 2 .. 15 zero; every negative is projected once for its front and its tail score;
//   * M_r and X are read from global memory once per kernel and triple with 16-byte loads into
//     LDS, zero-padded to multiples of 16 in both dimensions (Ep, Rp).  Row strides are
//     n + 4 floats (n + 20 where n % 64 == 0), i.e. 4 * odd and never 4 mod 64: the transposed
//     fragment reads (lane l at row l & 15, column k + (l >> 4)) then fall on 64 distinct banks,
//     and the straight ones (row k + (l >> 4), column l & 15) on four 16-bank windows that
//     overlap in at most 12 banks;
//   * every product is v_mfma_f32_16x16x4_f32 (A[row l & 15][k l >> 4], B[k l >> 4][col l & 15],
//     D col l & 15, rows 4 (l >> 4) + reg): exact fp32 products.  Y[16, Rp] = X M_r, its 16-column
//     slabs dealt to the waves, goes to LDS, is normalised per row by 16-lane groups, and the
//     scores are reduced by 16-lane groups over R (kg_part / kg_finish of kg_dev.h);
//   * the backward recomputes Y (nothing but the scores is saved), sums each projected row's
//     gradient over every score the row takes part in, pushes it through the normalisation, and
//     runs dX[16, Ep] = dY M_r^T and dM_r[Ep, Rp] = X^T dY (reduction depth 16: at most 4 MFMA
//     steps per tile, accumulators in registers) on the LDS operands; it flushes by fp32
//     atomics K + 2 entity rows, the real E x R elements of dM_r, and one rel row.
// Padding rows and columns are zero in every operand, so they add exactly zero; every global
// store is guarded by the row's own id (kgp_row: inside its table) and by E / R.
#include "hip/common.h"
#include "hip/kg_dev.h"
#include "hip/launchers.h"

namespace euler_hip {

namespace {

constexpr int kKgrThreads = 256;
constexpr int kKgrMaxNeg = 14;   // K + 2 rows fill the 16-row tile
constexpr int kKgrMaxDim = 128;  // [128, 148] floats of M_r: 74 KB of the 160 KB LDS

// corrupt: 0 front, 1 tail, 2 both (front scores, then tail scores).  kind: 0 L1, 1 L2.
// ent [n_ent, E], rel [n_rel, R], mat [n_rel, E * R], all fp32; ids as kgp_fwd.
struct KgrArgs {
  const float* ent;
  const float* rel;
  const float* mat;
  const int64_t* src;
  const int64_t* dst;
  const int64_t* ridx;
  const int64_t* neg;
  int64_t n_ent, n_rel;
  int K, E, R, kind, corrupt;
};

__host__ __device__ inline int kgr_stride(int n) { return n + (n % 64 == 0 ? 20 : 4); }

// LDS layout in floats: the tile's 16 row ids (int64), 17 norms, the relation row rho [Rp] and
// (backward) its gradient, X [16, SX], Y [16, SY], (backward) G = dY [16, SY], M_r [Ep, SY]
struct KgrLds {
  int Ep, Rp, SX, SY, rho, drho, x, y, g, m, floats;
};
constexpr int kKgrNorms = 32;  // float offset of the norms: rows 0..15 of Y, then rho

__host__ __device__ inline KgrLds kgr_lds(int E, int R, bool bwd) {
  KgrLds L;
  L.Ep = (E + 15) & ~15;
  L.Rp = (R + 15) & ~15;
  L.SX = kgr_stride(L.Ep);
  L.SY = kgr_stride(L.Rp);
  L.rho = 64;
  L.drho = L.rho + L.Rp;
  L.x = L.drho + (bwd ? L.Rp : 0);
  L.y = L.x + 16 * L.SX;
  L.g = L.y + 16 * L.SY;
  L.m = L.g + (bwd ? 16 * L.SY : 0);
  L.floats = L.m + L.Ep * L.SY;
  return L;
}

__device__ __forceinline__ float4_t kgr_mfma(float a, float b, float4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float4_t kgr_ld4(const float* p) { return *reinterpret_cast<const float4_t*>(p); }
__device__ __forceinline__ void kgr_st4(float* p, float4_t v) { *reinterpret_cast<float4_t*>(p) = v; }

// rows (a, b) of the tile that score q compares: q = -1 the positive, else the q-th corrupted
__device__ __forceinline__ void kgr_pair(const KgrArgs& a, int q, int& ra, int& rb) {
  if (q < 0) {
    ra = 0;
    rb = 1;
    return;
  }
  const bool front = a.corrupt == 0 || (a.corrupt == 2 && q < a.K);
  const int k = a.corrupt == 2 && q >= a.K ? q - a.K : q;
  ra = front ? 2 + k : 0;
  rb = front ? 1 : 2 + k;
}

// row 0..15 of Y, or (16) rho
__device__ __forceinline__ float* kgr_rowp(const KgrLds& L, float* sm, int row) {
  return row < 16 ? sm + L.y + row * L.SY : sm + L.rho;
}

// Stage the triple and project it: on return the LDS holds the row ids (-1: padding row), X,
// M_r, the normalised Y rows and rho, and their norms.  Ends in a barrier.
__device__ __forceinline__ void kgr_project(const KgrArgs& a, const KgrLds& L, float* sm, int64_t b, int64_t rs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t* ids = reinterpret_cast<int64_t*>(sm);
  if (tid < 16) {
    int64_t id = -1;
    if (tid < a.K + 2)
      id = kgp_row(tid == 0 ? a.src[b] : (tid == 1 ? a.dst[b] : a.neg[b * a.K + tid - 2]), a.n_ent);
    ids[tid] = id;
  }
  __syncthreads();
  const float4_t zero = {0.f, 0.f, 0.f, 0.f};
  const int rc = L.Rp >> 2, ec = L.Ep >> 2;
  const float* mr = a.mat + rs * a.E * a.R;
  for (int i = tid; i < L.Ep * rc; i += kKgrThreads) {
    const int e = i / rc, c = (i - e * rc) * 4;
    kgr_st4(sm + L.m + e * L.SY + c, e < a.E && c < a.R ? kgr_ld4(mr + e * a.R + c) : zero);
  }
  for (int i = tid; i < 16 * ec; i += kKgrThreads) {
    const int j = i / ec, c = (i - j * ec) * 4;
    kgr_st4(sm + L.x + j * L.SX + c, ids[j] >= 0 && c < a.E ? kgr_ld4(a.ent + ids[j] * a.E + c) : zero);
  }
  for (int i = tid; i < rc; i += kKgrThreads)
    kgr_st4(sm + L.rho + 4 * i, 4 * i < a.R ? kgr_ld4(a.rel + rs * a.R + 4 * i) : zero);
  __syncthreads();
  // Y = X M_r: one 16-column slab per wave and turn, reduction over the real E (a multiple of 4)
  const int li = lane & 15, lk = lane >> 4;
  for (int s = wave; s < (L.Rp >> 4); s += kKgrThreads / 64) {
    const float* xa = sm + L.x + li * L.SX + lk;
    const float* mb = sm + L.m + lk * L.SY + s * 16 + li;
    float4_t acc = zero;
    for (int k0 = 0; k0 < a.E; k0 += 4) acc = kgr_mfma(xa[k0], mb[k0 * L.SY], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) sm[L.y + (4 * lk + r) * L.SY + s * 16 + li] = acc[r];
  }
  __syncthreads();
  // the 16 rows of Y and rho, each by a group of 16 lanes over 4-column chunks
  const int grp = tid >> 4, sub = tid & 15;
  for (int row = grp; row < 17; row += 16) {
    float* p = kgr_rowp(L, sm, row);
    float part = 0.f;
    for (int c = sub; c < rc; c += 16) {
      const float4_t v = kgr_ld4(p + 4 * c);
      part += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    const float n = fmaxf(sqrtf(emb_group_sum(part, 16)), 1e-12f);
    for (int c = sub; c < rc; c += 16) kgr_st4(p + 4 * c, kgr_ld4(p + 4 * c) / n);
    if (sub == 0) sm[kKgrNorms + row] = n;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kKgrThreads) void kgr_fwd_kernel(KgrArgs a, float* __restrict__ pos_score,
                                                              float* __restrict__ neg_score) {
  extern __shared__ __attribute__((aligned(16))) float kgr_smem[];
  float* sm = kgr_smem;
  const KgrLds L = kgr_lds(a.E, a.R, false);
  const int64_t b = blockIdx.x;
  kgr_project(a, L, sm, b, kgp_row(a.ridx[b], a.n_rel));
  const int grp = threadIdx.x >> 4, sub = threadIdx.x & 15, rc = L.Rp >> 2;
  const int nneg = a.corrupt == 2 ? 2 * a.K : a.K;
  for (int s = grp; s < 1 + nneg; s += 16) {
    int ra, rb;
    kgr_pair(a, s - 1, ra, rb);
    float part = 0.f;
    for (int c = sub; c < rc; c += 16) {
      float x[4], r[4], y[4];
      EV<float>::load(sm + L.y + ra * L.SY + 4 * c, x);
      EV<float>::load(sm + L.rho + 4 * c, r);
      EV<float>::load(sm + L.y + rb * L.SY + 4 * c, y);
      part += kg_part(a.kind, x, r, y);
    }
    const float sc = kg_finish(a.kind, emb_group_sum(part, 16));
    if (sub == 0) {
      if (s == 0)
        pos_score[b] = sc;
      else
        neg_score[b * nneg + s - 1] = sc;
    }
  }
}

__global__ __launch_bounds__(kKgrThreads) void kgr_bwd_kernel(KgrArgs a, const float* __restrict__ pos_score,
                                                              const float* __restrict__ neg_score,
                                                              const float* __restrict__ gpos,
                                                              const float* __restrict__ gneg, float* __restrict__ dent,
                                                              float* __restrict__ drel, float* __restrict__ dmat) {
  extern __shared__ __attribute__((aligned(16))) float kgr_smem[];
  float* sm = kgr_smem;
  const KgrLds L = kgr_lds(a.E, a.R, true);
  const int64_t b = blockIdx.x, rs = kgp_row(a.ridx[b], a.n_rel);
  kgr_project(a, L, sm, b, rs);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = tid >> 4, sub = tid & 15, rc = L.Rp >> 2;
  const int nneg = a.corrupt == 2 ? 2 * a.K : a.K;
  const int64_t* ids = reinterpret_cast<const int64_t*>(sm);
  // 1. G[row] = d loss / d (normalised row), summed over the row's scores (h and t: up to 1 + K,
  //    a negative: up to 2, rho: all); one 4-column chunk of one row per thread and turn.
  //    d score / d (a, rho, b) of -|a + rho - b| as kgp_grad: the L2 norm is the forward's score.
  for (int i = tid; i < 17 * rc; i += kKgrThreads) {
    const int row = i / rc, c = (i - row * rc) * 4;
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
    if (row == 16 || row < a.K + 2) {
      const float4_t rho = kgr_ld4(sm + L.rho + c);
      for (int q = -1; q < nneg; ++q) {
        int ra, rb;
        kgr_pair(a, q, ra, rb);
        if (row != 16 && row != ra && row != rb) continue;
        const float g = q < 0 ? gpos[b] : gneg[b * nneg + q];
        const float nrm = -(q < 0 ? pos_score[b] : neg_score[b * nneg + q]);
        const float coef = a.kind == 1 ? (nrm > 1e-12f ? 1.f / nrm : 0.f) : 1.f;
        const float4_t d = kgr_ld4(sm + L.y + ra * L.SY + c) + rho - kgr_ld4(sm + L.y + rb * L.SY + c);
        const float sgn = row == rb ? g : -g;  // a and rho take -g * dnorm, b takes +g * dnorm
#pragma unroll
        for (int v = 0; v < 4; ++v)
          acc[v] += sgn * (a.kind == 0 ? (d[v] > 0.f ? 1.f : (d[v] < 0.f ? -1.f : 0.f)) : d[v] * coef);
      }
    }
    kgr_st4(row < 16 ? sm + L.g + row * L.SY + c : sm + L.drho + c, acc);
  }
  __syncthreads();
  // 2. through the normalisations: dy = (g - yn (yn . g)) / |y|; rho's goes straight to drel
  for (int row = grp; row < 17; row += 16) {
    const float* yn = kgr_rowp(L, sm, row);
    float* gp = row < 16 ? sm + L.g + row * L.SY : sm + L.drho;
    float part = 0.f;
    for (int c = sub; c < rc; c += 16) {
      const float4_t y = kgr_ld4(yn + 4 * c), g = kgr_ld4(gp + 4 * c);
      part += y[0] * g[0] + y[1] * g[1] + y[2] * g[2] + y[3] * g[3];
    }
    const float dot = emb_group_sum(part, 16), n = sm[kKgrNorms + row];
    for (int c = sub; c < rc; c += 16) {
      const float4_t dy = (kgr_ld4(gp + 4 * c) - kgr_ld4(yn + 4 * c) * dot) / n;
      if (row < 16) {
        kgr_st4(gp + 4 * c, dy);
      } else if (4 * c < a.R) {
#pragma unroll
        for (int v = 0; v < 4; ++v) atomicAdd(drel + rs * a.R + 4 * c + v, dy[v]);
      }
    }
  }
  __syncthreads();
  // 3. dX = dY M_r^T (Ep / 16 tiles, reduction over the real R) and dM_r = X^T dY
  //    ((Ep / 16) (Rp / 16) tiles, reduction over the tile's K + 2 rows), dealt to the waves
  const int li = lane & 15, lk = lane >> 4, ne = L.Ep >> 4, nr = L.Rp >> 4;
  float* dm = dmat + rs * a.E * a.R;
  for (int t = wave; t < ne + ne * nr; t += kKgrThreads / 64) {
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
    if (t < ne) {
      const float* ga = sm + L.g + li * L.SY + lk;
      const float* mb = sm + L.m + (t * 16 + li) * L.SY + lk;
      for (int k0 = 0; k0 < a.R; k0 += 4) acc = kgr_mfma(ga[k0], mb[k0], acc);
      const int col = t * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t id = ids[4 * lk + r];
        if (id >= 0 && col < a.E) atomicAdd(dent + id * a.E + col, acc[r]);
      }
    } else {
      const int e0 = (t - ne) / nr * 16, r0 = (t - ne) % nr * 16;
      const float* xa = sm + L.x + lk * L.SX + e0 + li;
      const float* gb = sm + L.g + lk * L.SY + r0 + li;
      for (int j0 = 0; j0 < a.K + 2; j0 += 4) acc = kgr_mfma(xa[j0 * L.SX], gb[j0 * L.SY], acc);
      const int col = r0 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = e0 + 4 * lk + r;
        if (e < a.E && col < a.R) atomicAdd(dm + e * a.R + col, acc[r]);
      }
    }
  }
}

bool kgr_args(const float* ent, const float* rel, const float* mat, int64_t n_ent, int64_t n_rel, const int64_t* src,
              const int64_t* dst, const int64_t* ridx, const int64_t* neg, int64_t B, int K, int E, int R, int kind,
              int corrupt, KgrArgs* a) {
  if (E % 4 != 0 || E < 4 || E > kKgrMaxDim || R % 4 != 0 || R < 4 || R > kKgrMaxDim || K < 0 || K > kKgrMaxNeg ||
      kind < 0 || kind > 1 || corrupt < 0 || corrupt > 2 || n_ent < 1 || n_rel < 1 || B < 0 || B > INT32_MAX)
    return false;
  if (!ent || !rel || !mat || !src || !dst || !ridx || (K > 0 && !neg)) return false;
  *a = KgrArgs{ent, rel, mat, src, dst, ridx, neg, n_ent, n_rel, K, E, R, kind, corrupt};
  return true;
}

// dynamic LDS of kernel `k` for these dimensions, raised past the default limit where needed
template <typename F>
hipError_t kgr_lds_bytes(F k, const KgrArgs& a, bool bwd, size_t* bytes) {
  *bytes = sizeof(float) * static_cast<size_t>(kgr_lds(a.E, a.R, bwd).floats);
  if (*bytes > 65536)
    EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(*bytes)));
  return hipSuccess;
}

}  // namespace

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

hipError_t eh_kgr_fwd(const float* ent, const float* rel, const float* mat, int64_t n_ent, int64_t n_rel,
                      const int64_t* src, const int64_t* dst, const int64_t* ridx, const int64_t* neg, int64_t B, int K,
                      int E, int R, int kind, int corrupt, float* pos_score, float* neg_score, hipStream_t s) {
  if (B == 0) return hipSuccess;
  KgrArgs a;
  if (!kgr_args(ent, rel, mat, n_ent, n_rel, src, dst, ridx, neg, B, K, E, R, kind, corrupt, &a) || !pos_score ||
      (K > 0 && !neg_score))
    return hipErrorInvalidValue;
  size_t lds;
  EULER_HIP_CHECK(kgr_lds_bytes(kgr_fwd_kernel, a, false, &lds));
  hipLaunchKernelGGL(kgr_fwd_kernel, dim3(static_cast<uint32_t>(B)), dim3(kKgrThreads), lds, s, a, pos_score,
                     neg_score);
  return hipGetLastError();
}

hipError_t eh_kgr_bwd(const float* ent, const float* rel, const float* mat, int64_t n_ent, int64_t n_rel,
                      const int64_t* src, const int64_t* dst, const int64_t* ridx, const int64_t* neg, int64_t B, int K,
                      int E, int R, int kind, int corrupt, const float* pos_score, const float* neg_score,
                      const float* gpos, const float* gneg, float* dent, float* drel, float* dmat, hipStream_t s) {
  if (B == 0) return hipSuccess;
  KgrArgs a;
  if (!kgr_args(ent, rel, mat, n_ent, n_rel, src, dst, ridx, neg, B, K, E, R, kind, corrupt, &a) || !pos_score ||
      !gpos || (K > 0 && (!neg_score || !gneg)) || !dent || !drel || !dmat)
    return hipErrorInvalidValue;
  size_t lds;
  EULER_HIP_CHECK(kgr_lds_bytes(kgr_bwd_kernel, a, true, &lds));
  hipLaunchKernelGGL(kgr_bwd_kernel, dim3(static_cast<uint32_t>(B)), dim3(kKgrThreads), lds, s, a, pos_score,
                     neg_score, gpos, gneg, dent, drel, dmat);
  return hipGetLastError();
}

}  // extern "C"
