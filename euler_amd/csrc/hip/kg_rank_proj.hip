// Link-prediction rank counts for the projected translation models (ops/kg_rank_ops.py
// rank_counts_proj): every query against every entity, with the entity rows projected under the
// query's relation INSIDE the kernel, so neither a projected [N, D'] table nor a [B, N] score
// matrix ever reaches global memory.
//
//   model 0  TransH   w = hyper[r] / max(|hyper[r]|, 1e-12)     P(x) = x - (x . w) w
//   model 1  TransD   P(x) = y / max(|y|, 1e-12),  y = x + (x . ent_t[x]) rel_t[r]
//   model 2  TransR   P(x) = y / max(|y|, 1e-12),  y = x M_r   (M_r row-major [E, R])
//   rho = rel[r] / max(|rel[r]|, 1e-12);  query = P(given) + rho (tail side) or - rho (head side);
//   score = sum_d |query - P(e)| (kind 0) or sum_d (query - P(e))^2 (kind 1), lower is better.
// Counting rule, summation rule (kg_term folded over d ascending into one fp32 accumulator) and
// the epilogue are those of kg_rank.hip (kg_rank_dev.h).
//
// Work split.  The host orders the queries by relation (`order`: sorted position -> query) and
// cuts every relation segment into tiles of at most 64 queries of ONE relation (`tiles`:
// relation row, first sorted position, count).  A work item is (tile, candidate range); blocks of
// 4 waves take items grid-stride.
//
// Per item, once: the relation's operands go to LDS (w normalised by one wave, rho by another,
// TransD's r_p raw, TransR's M_r zero-padded to 16 columns), then the tile's `given` rows are
// gathered (with their entity_transfer rows for TransD), projected by kgrp_project — the function
// the candidates go through — and shifted by +-rho.  The projected queries stay in LDS.
//
// Per candidate tile of 64 rows: the raw rows are staged WHOLE (the projection needs the full-row
// dot product before any score term exists).  Thread t stages row t >> 2, its 16-byte chunks
// sub + 4 i (sub = t & 3), in registers, one tile ahead: the next tile's global loads are in
// flight under the current tile's projection and scan.  kgrp_project:
//   TransH / TransD   the thread that staged a chunk projects it, so the raw rows (and TransD's
//                     transfer rows) never touch LDS: the dot product and the norm are 4-lane xor
//                     butterflies over the row's 4 threads, and only the projected row is stored;
//   TransR            the raw tile goes to LDS; wave w owns rows 16 w .. 16 w + 15 and computes
//                     Y = X M_r for ALL of its (up to 8) 16-column slabs with
//                     v_mfma_f32_16x16x4_f32, one A fragment per step shared by the slabs,
//                     accumulators in registers; only then does it write Y over X (this is why
//                     the tile fits: M_r + queries + ONE 64-row buffer is 146 KB at E = R = 128,
//                     a separate Y would need 181 KB), and normalises its rows with the 4-lane
//                     groups.
// Then kg_rank.hip's 16 x 16 thread grid: thread (ty, tx) folds the 4 x 4 pairs of queries
// ty * 4 + i and candidates tx + 16 j over all of d, and runs the epilogue.
//
// True scores.  The SAME kernel runs first with pass = 0: its only candidate tile is the tile's
// own true rows, and the thread that owns pair (query i, candidate i) stores ts.  Both passes are
// one binary, every projection step is an explicit fma / add / div / sqrt (nothing for the compiler
// to contract differently), and a row's projection depends on nothing but its own table rows and
// the relation operands, so a candidate whose rows equal the true entity's rows bitwise ties.
//
// Row strides are 4 * odd floats (kgrp_stride): 16 rows then start at 16 distinct 4-bank slots, as
// with kg_rank.hip's 36, for the b128 reads of the scan and the A fragment reads of the MFMA;
// M_r keeps kg_transr.hip's stride.  Every LDS word that is read was written by this item: rows
// past the tile or past N are staged as zeros (their projections are zeros, never NaN) and are
// skipped by the epilogue.
#include "hip/common.h"
#include "hip/kg_rank_dev.h"
#include "hip/launchers.h"

#include <limits.h>
#include <math.h>

namespace euler_hip {

namespace {

constexpr int kKgrpThreads = 256;
constexpr int kKgrpTile = 64;     // queries per tile = candidates per tile
constexpr int kKgrpMaxDim = 128;  // E, R
constexpr int kKgrpNV = kKgrpMaxDim / 16;  // 16-byte chunks per thread of a staged 64-row tile
constexpr int kKgrpMaxSplits = 4096;

struct KgrpArgs {
  const float* ent;   // [N, E]
  const float* rel;   // [n_rel, R]
  const float* pe;    // TransD entity_transfer [N, E]
  const float* pr;    // hyper [n_rel, E] / relation_transfer [n_rel, E] / mat [n_rel, E * R]
  const int64_t* given;
  const int64_t* true_idx;
  const int64_t* order;  // [B] sorted position -> query
  const int32_t* tiles;  // [T, 3] relation row, first sorted position, count (1..64)
  const int64_t* filt_ptr;
  const int32_t* filt_idx;
  int64_t nf, B, N, tiles_per_split, items;
  float* ts;        // [B]
  int64_t* better;  // [B, S]
  int64_t* ties;
  int T, S, E, R, pass;
  float sign;  // +1 tail side, -1 head side
};

__host__ __device__ inline int kgrp_stride(int n) { return n + (((n >> 2) & 1) ? 8 : 4); }  // 4 * odd
__host__ __device__ inline int kgrp_mstride(int n) { return n + (n % 64 == 0 ? 20 : 4); }

// LDS layout in floats: 3 x 64 int64 ids (given, true, query), w / r_p [128], rho [128], the
// projected queries [64, S], the candidate tile [64, S], TransR's M_r [E, SM]
struct KgrpLds {
  int S, SM, Rp, w, rho, q, x, m, floats;
};

__host__ __device__ inline KgrpLds kgrp_lds(int model, int E, int R) {
  KgrpLds L;
  L.Rp = (R + 15) & ~15;
  L.S = kgrp_stride(model == 2 ? (E > L.Rp ? E : L.Rp) : E);
  L.SM = kgrp_mstride(L.Rp);
  L.w = 3 * kKgrpTile * 2;
  L.rho = L.w + kKgrpMaxDim;
  L.q = L.rho + kKgrpMaxDim;
  L.x = L.q + kKgrpTile * L.S;
  L.m = L.x + kKgrpTile * L.S;
  L.floats = L.m + (model == 2 ? E * L.SM : 0);
  return L;
}

__device__ __forceinline__ float4_t kgrp_ld4(const float* p) { return *reinterpret_cast<const float4_t*>(p); }
__device__ __forceinline__ void kgrp_st4(float* p, float4_t v) { *reinterpret_cast<float4_t*>(p) = v; }

__device__ __forceinline__ float kgrp_dot4(float4_t a, float4_t b, float acc) {
#pragma unroll
  for (int v = 0; v < 4; ++v) acc = fmaf(a[v], b[v], acc);
  return acc;
}

// sum over aligned groups of G lanes; every lane of a group gets the same bits
template <int G>
__device__ __forceinline__ float kgrp_group_sum(float v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

// x / max(|x|, 1e-12) from the row's sum of squares: IEEE sqrt and division (kg_dev.h's formula)
__device__ __forceinline__ float kgrp_norm(float sumsq) { return fmaxf(__fsqrt_rn(sumsq), 1e-12f); }
__device__ __forceinline__ float4_t kgrp_div4(float4_t x, float n) {
  return float4_t{__fdiv_rn(x[0], n), __fdiv_rn(x[1], n), __fdiv_rn(x[2], n), __fdiv_rn(x[3], n)};
}

// one wave: n floats (n <= 128) of src -> dst in LDS, l2-normalised on the way when asked
__device__ __forceinline__ void kgrp_load_vec(const float* __restrict__ src, int n, bool normalize, float* dst) {
  const int lane = threadIdx.x & 63;
  const bool in = 4 * lane < n;
  float4_t v = {0.f, 0.f, 0.f, 0.f};
  if (in) v = kgrp_ld4(src + 4 * lane);
  if (normalize) v = kgrp_div4(v, kgrp_norm(kgrp_group_sum<32>(kgrp_dot4(v, v, 0.f))));
  if (in) kgrp_st4(dst + 4 * lane, v);
}

// rows of a [64, S] LDS tile, 4 lanes each, divided by their l2 norm over nch 16-byte chunks
__device__ __forceinline__ void kgrp_normalize_rows(float* buf, int S, int nch) {
  float* p = buf + (threadIdx.x >> 2) * S;
  const int sub = threadIdx.x & 3;
  float4_t y[kKgrpNV];
  float part = 0.f;
#pragma unroll
  for (int i = 0; i < kKgrpNV; ++i) {
    const int c = sub + 4 * i;
    if (c < nch) {
      y[i] = kgrp_ld4(p + 4 * c);
      part = kgrp_dot4(y[i], y[i], part);
    }
  }
  const float n = kgrp_norm(kgrp_group_sum<4>(part));
#pragma unroll
  for (int i = 0; i < kKgrpNV; ++i) {
    const int c = sub + 4 * i;
    if (c < nch) kgrp_st4(p + 4 * c, kgrp_div4(y[i], n));
  }
}

// A 64-row tile is dealt to the threads the same way everywhere: thread t has row t >> 2 and its
// 16-byte chunks sub + 4 i (sub = t & 3).  This thread's chunks of entity row `id` (TransD: and
// of its transfer row), zeros for id < 0 or past the row.
template <int MODEL>
__device__ __forceinline__ void kgrp_load_row(const KgrpArgs& a, int64_t id, float4_t* x, float4_t* xp) {
  const int sub = threadIdx.x & 3, nch = a.E >> 2;
  const int64_t o = (id < 0 ? 0 : id) * a.E;
#pragma unroll
  for (int i = 0; i < kKgrpNV; ++i) {
    const int c = sub + 4 * i;
    const bool ok = id >= 0 && c < nch;
    x[i] = ok ? kgrp_ld4(a.ent + o + 4 * c) : float4_t{0.f, 0.f, 0.f, 0.f};
    if (MODEL == 1) xp[i] = ok ? kgrp_ld4(a.pe + o + 4 * c) : float4_t{0.f, 0.f, 0.f, 0.f};
  }
}

// Project a tile of raw rows (this thread's chunks x, TransD: xp) under the relation operands in
// LDS and leave the projected rows in buf [64, S].  The caller puts a barrier before (buf is
// free) and after.  The queries and the candidates both come through here.
template <int MODEL>
__device__ __forceinline__ void kgrp_project(const KgrpLds& L, float* sm, float* buf, float4_t* x,
                                             const float4_t* xp, int E, int R) {
  const int tid = threadIdx.x;
  const int sub = tid & 3, nch = E >> 2;
  float* p = buf + (tid >> 2) * L.S;
  if (MODEL == 2) {
#pragma unroll
    for (int i = 0; i < kKgrpNV; ++i)
      if (sub + 4 * i < nch) kgrp_st4(p + 4 * (sub + 4 * i), x[i]);
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4, ns = L.Rp >> 4;
    const float* xa = buf + (16 * wave + li) * L.S + lk;
    const float* mb = sm + L.m + lk * L.SM + li;
    float4_t acc[kKgrpNV];
#pragma unroll
    for (int s = 0; s < kKgrpNV; ++s) acc[s] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < E; k0 += 4) {  // reduction over the real E (a multiple of 4)
      const float av = xa[k0];
#pragma unroll
      for (int s = 0; s < kKgrpNV; ++s)
        if (s < ns) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, mb[k0 * L.SM + 16 * s], acc[s], 0, 0, 0);
    }
    __syncthreads();  // every fragment of X is read before Y goes over it
#pragma unroll
    for (int s = 0; s < kKgrpNV; ++s)
      if (s < ns) {
#pragma unroll
        for (int r = 0; r < 4; ++r) buf[(16 * wave + 4 * lk + r) * L.S + 16 * s + li] = acc[s][r];
      }
    __syncthreads();
    kgrp_normalize_rows(buf, L.S, R >> 2);
  } else {
    const float* w = sm + L.w;  // w (TransH) or r_p (TransD)
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < kKgrpNV; ++i)
      if (sub + 4 * i < nch) part = kgrp_dot4(x[i], MODEL == 0 ? kgrp_ld4(w + 4 * (sub + 4 * i)) : xp[i], part);
    const float s = kgrp_group_sum<4>(part);
    float n2 = 0.f;
#pragma unroll
    for (int i = 0; i < kKgrpNV; ++i)
      if (sub + 4 * i < nch) {
        const float4_t wv = kgrp_ld4(w + 4 * (sub + 4 * i));
#pragma unroll
        for (int v = 0; v < 4; ++v) x[i][v] = fmaf(MODEL == 0 ? -s : s, wv[v], x[i][v]);
        if (MODEL == 1) n2 = kgrp_dot4(x[i], x[i], n2);
      }
    float n = 1.f;
    if (MODEL == 1) n = kgrp_norm(kgrp_group_sum<4>(n2));
#pragma unroll
    for (int i = 0; i < kKgrpNV; ++i)
      if (sub + 4 * i < nch) kgrp_st4(p + 4 * (sub + 4 * i), MODEL == 1 ? kgrp_div4(x[i], n) : x[i]);
  }
}

template <int MODEL, int KIND>
__global__ __launch_bounds__(kKgrpThreads) void kg_rank_proj_kernel(KgrpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kgrp_smem[];
  float* sm = kgrp_smem;
  const KgrpLds L = kgrp_lds(MODEL, a.E, a.R);
  int64_t* giv = reinterpret_cast<int64_t*>(sm);  // [64] given entity of the tile's queries, -1 past the tile
  int64_t* tru_s = giv + kKgrpTile;               // [64] their true entity
  int64_t* qb_s = giv + 2 * kKgrpTile;            // [64] the query (row of the outputs)
  float* Qs = sm + L.q;
  float* Xs = sm + L.x;

  const int tid = threadIdx.x, wave = tid >> 6;
  const int tx = tid & 15, ty = tid >> 4;
  const int srow = tid >> 2;              // the tile row this thread stages
  const int DP = MODEL == 2 ? a.R : a.E;  // width of the projected rows
  const int64_t ntiles = (a.N + kKgrpTile - 1) / kKgrpTile;

  for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int t = static_cast<int>(item % a.T);
    const int split = static_cast<int>(item / a.T);
    const int64_t rs = a.tiles[3 * t];
    const int64_t first = a.tiles[3 * t + 1];
    const int cnt = a.tiles[3 * t + 2];
    int64_t t_begin = 0, t_end = 1;  // pass 0: the one tile of true rows
    if (a.pass != 0) {
      t_begin = split * a.tiles_per_split;
      t_end = t_begin + a.tiles_per_split;
      if (t_end > ntiles) t_end = ntiles;
      if (t_begin >= t_end) {  // more ranges than candidate tiles: this partial is zero
        if (tid < cnt) {
          const int64_t b = a.order[first + tid];
          a.better[b * a.S + split] = 0;
          a.ties[b * a.S + split] = 0;
        }
        continue;
      }
    }

    __syncthreads();  // the previous item's LDS is consumed
    if (tid < kKgrpTile) {
      const int64_t b = tid < cnt ? a.order[first + tid] : int64_t{-1};
      qb_s[tid] = b;
      giv[tid] = b >= 0 ? a.given[b] : int64_t{-1};
      tru_s[tid] = b >= 0 ? a.true_idx[b] : int64_t{-1};
    }
    if (wave == 0 && MODEL != 2) kgrp_load_vec(a.pr + rs * a.E, a.E, MODEL == 0, sm + L.w);
    if (wave == 1) kgrp_load_vec(a.rel + rs * a.R, DP, true, sm + L.rho);
    if (MODEL == 2) {
      const int rc = L.Rp >> 2;
      const float* mr = a.pr + rs * a.E * a.R;
      for (int i = tid; i < a.E * rc; i += kKgrpThreads) {
        const int e = i / rc, c = (i - e * rc) * 4;
        kgrp_st4(sm + L.m + e * L.SM + c, c < a.R ? kgrp_ld4(mr + e * a.R + c) : float4_t{0.f, 0.f, 0.f, 0.f});
      }
    }
    __syncthreads();

    // the candidate row of tile slot srow: pass 0 the slot's true row, else row c0 + srow
    auto cand_id = [&](int64_t c0) {
      if (a.pass == 0) return tru_s[srow];
      return c0 + srow < a.N ? c0 + srow : int64_t{-1};
    };

    // the queries: P(given) + sign * rho, resident for the whole item
    float4_t st[kKgrpNV], stp[MODEL == 1 ? kKgrpNV : 1];  // the staged raw row, one tile ahead
    float4_t x[kKgrpNV], xp[MODEL == 1 ? kKgrpNV : 1];
    kgrp_load_row<MODEL>(a, giv[srow], x, xp);
    kgrp_load_row<MODEL>(a, cand_id(t_begin * kKgrpTile), st, stp);  // in flight under the query projection
    kgrp_project<MODEL>(L, sm, Qs, x, xp, a.E, a.R);
    __syncthreads();
    for (int i = tid; i < kKgrpTile * (DP >> 2); i += kKgrpThreads) {
      const int row = i / (DP >> 2), c = (i - row * (DP >> 2)) * 4;
      float4_t q = kgrp_ld4(Qs + row * L.S + c);
      const float4_t r = kgrp_ld4(sm + L.rho + c);
#pragma unroll
      for (int v = 0; v < 4; ++v) q[v] = __fadd_rn(q[v], a.sign * r[v]);
      kgrp_st4(Qs + row * L.S + c, q);
    }

    // the owned queries
    int64_t qb[4], tru[4];
    float tsc[4];
    int nb[4], nt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      qb[i] = qb_s[ty * 4 + i];
      tru[i] = tru_s[ty * 4 + i];
      tsc[i] = a.pass != 0 && qb[i] >= 0 ? a.ts[qb[i]] : __builtin_nanf("");
      nb[i] = 0;
      nt[i] = 0;
    }

    for (int64_t tile = t_begin; tile < t_end; ++tile) {
      const int64_t c0 = tile * kKgrpTile;
#pragma unroll
      for (int i = 0; i < kKgrpNV; ++i) {
        x[i] = st[i];
        if (MODEL == 1) xp[i] = stp[i];
      }
      // the next tile's global loads stay in flight under this tile's projection and scan
      if (tile + 1 < t_end) kgrp_load_row<MODEL>(a, cand_id(c0 + kKgrpTile), st, stp);
      __syncthreads();  // the previous tile's rows are consumed (first turn: the queries are written)
      kgrp_project<MODEL>(L, sm, Xs, x, xp, a.E, a.R);
      __syncthreads();

      float acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
      for (int kg = 0; kg < (DP >> 2); ++kg) {
        float4_t qv[4], cv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) qv[i] = kgrp_ld4(Qs + (ty * 4 + i) * L.S + kg * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[j] = kgrp_ld4(Xs + (tx + 16 * j) * L.S + kg * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e)  // d ascending for every pair
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = kg_term<KIND>(acc[i][j], qv[i][e], cv[j][e]);
      }

      if (a.pass == 0) {
        // candidate slot s holds the true row of query slot s: pair (s, s) is the true score
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (tx + 16 * j == ty * 4 + i && qb[i] >= 0) a.ts[qb[i]] = acc[i][j];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int64_t e = c0 + tx + 16 * j;
            if (qb[i] < 0 || e >= a.N || e == tru[i]) continue;
            kg_rank_pair<KIND>(acc[i][j], tsc[i], qb[i], e, a.filt_ptr, a.filt_idx, a.nf, nb[i], nt[i]);
          }
      }
    }

    if (a.pass != 0) {
      // the 16 lanes tx = 0..15 of a query are consecutive lanes of one wave
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int vb = nb[i], vt = nt[i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          vb += __shfl_xor(vb, o);
          vt += __shfl_xor(vt, o);
        }
        if (tx == 0 && qb[i] >= 0) {
          a.better[qb[i] * a.S + split] = vb;
          a.ties[qb[i] * a.S + split] = vt;
        }
      }
    }
  }
}

template <int MODEL, int KIND>
hipError_t kgrp_launch(KgrpArgs a, hipStream_t s) {
  const size_t lds = sizeof(float) * static_cast<size_t>(kgrp_lds(MODEL, a.E, a.R).floats);
  auto k = kg_rank_proj_kernel<MODEL, KIND>;
  if (lds > 65536)
    EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(lds)));
  for (int pass = 0; pass < 2; ++pass) {  // true scores, then the scan that compares against them
    a.pass = pass;
    a.items = pass == 0 ? a.T : static_cast<int64_t>(a.T) * a.S;
    const int grid = static_cast<int>(a.items < 8192 ? a.items : 8192);
    hipLaunchKernelGGL(k, dim3(grid), dim3(kKgrpThreads), lds, s, a);
    EULER_HIP_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

}  // namespace

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

int eh_kg_rank_proj_max_dim() { return kKgrpMaxDim; }

hipError_t eh_kg_rank_proj(int model, const float* ent, const float* rel, const float* pe, const float* pr, int64_t N,
                           int E, int R, const int64_t* given, const int64_t* true_idx, const int64_t* order,
                           const int32_t* tiles, int64_t T, int64_t B, int side, int kind, const int64_t* filt_ptr,
                           const int32_t* filt_idx, int64_t nf, int S, float* ts, int64_t* better, int64_t* ties,
                           hipStream_t s) {
  if (model < 0 || model > 2 || kind < 0 || kind > 1 || side < 0 || side > 1) return hipErrorInvalidValue;
  if (E % 4 != 0 || E < 4 || E > kKgrpMaxDim || R % 4 != 0 || R < 4 || R > kKgrpMaxDim || (model != 2 && E != R))
    return hipErrorInvalidValue;
  // candidate positions are compared with the 32-bit filter entries; a tile holds at least one query
  if (B <= 0 || N <= 0 || N > INT_MAX || B > INT_MAX || T < 1 || T > B || S < 1 || S > kKgrpMaxSplits || nf < 0)
    return hipErrorInvalidValue;
  if (!ent || !rel || !pr || (model == 1 && !pe) || !given || !true_idx || !order || !tiles || !ts || !better || !ties)
    return hipErrorInvalidValue;
  if (filt_ptr != nullptr && filt_idx == nullptr && nf > 0) return hipErrorInvalidValue;
  KgrpArgs a;
  a.ent = ent;
  a.rel = rel;
  a.pe = pe;
  a.pr = pr;
  a.given = given;
  a.true_idx = true_idx;
  a.order = order;
  a.tiles = tiles;
  a.filt_ptr = filt_ptr;
  a.filt_idx = filt_idx;
  a.nf = nf;
  a.B = B;
  a.N = N;
  a.tiles_per_split = ceil_div(ceil_div(N, kKgrpTile), S);
  a.items = 0;
  a.ts = ts;
  a.better = better;
  a.ties = ties;
  a.T = static_cast<int>(T);
  a.S = S;
  a.E = E;
  a.R = R;
  a.pass = 0;
  a.sign = side == 1 ? 1.f : -1.f;
#define EH_KGRP(M)                                                              \
  return kind == 0 ? kgrp_launch<M, 0>(a, s) : kgrp_launch<M, 1>(a, s)
  if (model == 0) EH_KGRP(0);
  if (model == 1) EH_KGRP(1);
  EH_KGRP(2);
#undef EH_KGRP
}

}  // extern "C"
