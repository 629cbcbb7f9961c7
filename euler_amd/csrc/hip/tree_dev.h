// Device code of the fused GraphSAGE tree step that more than one of its translation units
// (tree_fwd.hip, tree_head.hip, tree_dw.hip) uses, each piece defined once:
//   * the mini-batch sampler: Philox streams, root / neighbour draws, the slot chain of
//     tree_args.h and one sampler block (its own launch, extra blocks of the head launch and of
//     the optimizer launch);
//   * feature rows: Feat8;
//   * the swizzled layer-0 A tile: f2_gather / f2_kt (tr_fwd2_kernel) and the 32-row gather
//     tile of the pipelined step (extra blocks of the optimizer launch);
//   * per-block phase stamps.
#pragma once
#include "hip/tile.h"
#include "hip/tree_args.h"

namespace euler_hip {

constexpr uint64_t kTrStreamRoot = 1, kTrStreamPos = 2, kTrStreamNeg = 3, kTrStreamHop = 16;

// per-block phase stamp k (0..7) of the optional diagnostics buffer prof [blocks][8].  A macro:
// as an inline function the kernels with a signed block id come out with other registers
// (profiles/tree_split/README.md), and the split keeps every kernel's code as it was.
#define TR_STAMP(prof, blk, k) \
  if ((prof) && threadIdx.x == 0) (prof)[(blk) * 8 + (k)] = static_cast<long long>(wall_clock64())

__device__ __forceinline__ uint4_t tr_rand(const int64_t* rng, uint64_t stream, uint64_t idx) {
  return Philox::gen(static_cast<uint64_t>(rng[0]), (static_cast<uint64_t>(rng[1]) << 8) ^ stream, idx);
}

// Walker alias draw of root t (reference sample_node: weighted, per node type)
__device__ __forceinline__ int32_t tr_root(const TrGraph& g, const int64_t* rng, int64_t t,
                                           uint64_t stream = kTrStreamRoot) {
  const uint4_t r = tr_rand(rng, stream, static_cast<uint64_t>(t));
  const uint64_t x = (static_cast<uint64_t>(r[0]) << 32) | r[1];
  int64_t k = static_cast<int64_t>(__umul64hi(x, static_cast<uint64_t>(g.pop)));
  if (k >= g.pop) k = g.pop - 1;
  const int64_t pick = (u01(r[2]) < g.prob[k]) ? k : static_cast<int64_t>(g.alias[k]);
  return g.root_rows ? g.root_rows[pick] : static_cast<int32_t>(pick);
}

// one weighted with-replacement neighbour draw (reference node.cc:98-161: pick an edge
// type group by its weight sum, then binary-search the group); -1 when there is none
__device__ int32_t tr_neighbor(const TrGraph& g, int32_t row, uint32_t mask, uint4_t r) {
  if (row < 0 || row >= g.num_rows) return -1;
  const int64_t base = static_cast<int64_t>(row) * g.num_types;
  int64_t lo = 0, hi = 0;
  float total = 0.f;
  if (g.num_types == 1) {
    if (!(mask & 1u)) return -1;
    lo = g.indptr[base];
    hi = g.indptr[base + 1];
    total = hi > lo ? g.cumw[hi - 1] : 0.f;
  } else {
    float tot = 0.f;
    for (int t = 0; t < g.num_types; ++t) {
      if (!((mask >> t) & 1u)) continue;
      const int64_t a = g.indptr[base + t], b = g.indptr[base + t + 1];
      if (b > a) tot += g.cumw[b - 1];
    }
    if (!(tot > 0.f)) return -1;
    float u = u01(r[0]) * tot;
    for (int t = 0; t < g.num_types; ++t) {
      if (!((mask >> t) & 1u)) continue;
      const int64_t a = g.indptr[base + t], b = g.indptr[base + t + 1];
      if (b <= a) continue;
      const float gw = g.cumw[b - 1];
      lo = a;
      hi = b;
      total = gw;
      if (u < gw) break;
      u -= gw;
    }
  }
  if (hi <= lo || !(total > 0.f)) return -1;
  const float u = u01(r[1]) * total;
  int64_t a = lo, b = hi - 1;
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if (g.cumw[m] > u) b = m;
    else a = m + 1;
  }
  return g.nbr[a];
}

// slot j of the group of `parent` (whose own slot index is parent_slot) at hop `hop`
__device__ __forceinline__ int32_t tr_hop(const TrGraph& g, const int64_t* rng, int32_t parent, int j, int F,
                                          uint32_t mask, int hop, int64_t parent_slot, int stream_off = 0) {
  if (j < F)
    return parent >= 0 ? tr_neighbor(g, parent, mask,
                                     tr_rand(rng, kTrStreamHop + hop + stream_off,
                                             static_cast<uint64_t>(parent_slot * F + j)))
                       : -1;
  return j == F ? parent : -1;
}

// root t of a tree (see TrTree::root_mode): given, an alias draw, or a pair model's context
// root (the source root's positive neighbour, or a negative draw)
__device__ __forceinline__ int32_t tr_tree_root(const TrGraph& g, const TrTree& tr, int64_t t) {
  if (tr.root_in) return tr.root_in[t];
  if (tr.root_mode == 0) return tr_root(g, tr.rng, t);
  if (t < tr.pair_B) {
    const int32_t src = tr_root(g, tr.rng, t);
    return src >= 0 ? tr_neighbor(g, src, tr.pair_mask, tr_rand(tr.rng, kTrStreamPos, static_cast<uint64_t>(t)))
                    : -1;
  }
  return tr_root(g, tr.rng, t, kTrStreamNeg);
}

// node of slot s at level lv (0..2); *root = index of its root, *self_chain = the slot is
// the root itself (every digit is the self slot)
__device__ int32_t tr_slot_node(const TrGraph& g, const TrTree& tr, int64_t s, int lv, int64_t* root,
                                bool* self_chain) {
  int64_t i0 = s, i1 = 0, i2 = 0;
  if (lv == 1) {
    i1 = s;
    i0 = s >> tr.logP1;
  } else if (lv == 2) {
    i2 = s;
    i1 = s >> tr.logP2;
    i0 = i1 >> tr.logP1;
  }
  int32_t node = tr_tree_root(g, tr, i0);
  bool sc = true;
  if (lv >= 1) {
    const int j = static_cast<int>(i1 & ((int64_t(1) << tr.logP1) - 1));
    sc = j == tr.F1;
    node = tr_hop(g, tr.rng, node, j, tr.F1, tr.m1, 1, i0, tr.stream_off);
  }
  if (lv >= 2) {
    const int j = static_cast<int>(i2 & ((int64_t(1) << tr.logP2) - 1));
    sc = sc && j == tr.F2;
    node = tr_hop(g, tr.rng, node, j, tr.F2, tr.m2, 2, i1, tr.stream_off);
  }
  *root = i0;
  *self_chain = sc;
  return node;
}

__device__ __forceinline__ float bf_lo(uint32_t v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float bf_hi(uint32_t v) { return __uint_as_float(v & 0xffff0000u); }

// 8 consecutive feature columns of one row, bf16 or fp32 storage
template <typename FT>
struct Feat8;
template <>
struct Feat8<bf16_t> {
  static constexpr int kInFlight = 10;  // rows in flight per thread and item
  uint4_t v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const uint4_t*>(p); }
  __device__ __forceinline__ void zero() { v = uint4_t{0u, 0u, 0u, 0u}; }
  __device__ __forceinline__ void add_to(float* acc) const { acc_bf16x8(acc, v); }
  __device__ __forceinline__ void add_scaled_to(float* acc, float w) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[2 * i] += w * bf_lo(v[i]);
      acc[2 * i + 1] += w * bf_hi(v[i]);
    }
  }
  // keep = false: the row was a padding id (-1) loaded from row 0; contributes zero
  __device__ __forceinline__ void keep(bool k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = k ? v[i] : 0u;
  }
  __device__ __forceinline__ uint4_t bf16() const { return v; }
};
template <>
struct Feat8<float> {
  static constexpr int kInFlight = 5;
  float4_t a, b;
  __device__ __forceinline__ void load(const float* p) {
    a = *reinterpret_cast<const float4_t*>(p);
    b = *reinterpret_cast<const float4_t*>(p + 4);
  }
  __device__ __forceinline__ void zero() { a = b = float4_t{0.f, 0.f, 0.f, 0.f}; }
  __device__ __forceinline__ void add_to(float* acc) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] += a[i];
      acc[4 + i] += b[i];
    }
  }
  __device__ __forceinline__ void add_scaled_to(float* acc, float w) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] += w * a[i];
      acc[4 + i] += w * b[i];
    }
  }
  __device__ __forceinline__ void keep(bool k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = k ? a[i] : 0.f;
      b[i] = k ? b[i] : 0.f;
    }
  }
  __device__ __forceinline__ uint4_t bf16() const {
    float t[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return pack_bf16x8(t);
  }
};

// ----------------------------------------------------------------------------
// tr_sample: target-row nodes (root -> hop chain) and their leaf draws, NT / 4 rows per block
// ----------------------------------------------------------------------------
constexpr int kTrSampleRows = 64;  // of tr_sample_kernel and the optimizer launch's sampler blocks (256 threads)

// one sampler block of NT threads: NT / 4 target rows (root -> hop chain by the first
// NT / 4 threads, then every thread draws leaves)
template <int NT>
__device__ __forceinline__ void tr_sample_block(const TrSampleArgs& a, int blk, int32_t* node_s) {
  constexpr int R = NT / 4;
  const int64_t row0 = static_cast<int64_t>(blk) * R;
  if (threadIdx.x < R) {
    const int64_t s = row0 + threadIdx.x;
    int32_t node = -1;
    if (s < a.M) {
      int64_t root;
      bool sc;
      node = tr_slot_node(a.g, a.tr, s, a.lv, &root, &sc);
      if (sc) a.roots[root] = node;
      a.nodes[s] = node;
    }
    node_s[threadIdx.x] = node;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < R * a.FL; it += NT) {
    const int r = it / a.FL, k = it - r * a.FL;
    const int64_t s = row0 + r;
    if (s >= a.M) break;
    const int32_t node = node_s[r];
    a.leaf[s * a.FL + k] =
        node >= 0 ? tr_neighbor(a.g, node, a.mL,
                                tr_rand(a.tr.rng, kTrStreamHop + a.hopL + a.tr.stream_off,
                                        static_cast<uint64_t>(s * a.FL + k)))
                  : -1;
  }
}

// ----------------------------------------------------------------------------
// the swizzled, unpadded layer-0 A tile [BM][2D] of tr_fwd2_kernel (tree_fwd.hip) and of the
// gather tiles: 16-B chunk c of row r lives at chunk c ^ (r & 15)
// ----------------------------------------------------------------------------
#ifndef F2_SKIP_PAD
#define F2_SKIP_PAD 1
#endif

__device__ __forceinline__ int f2_chunk(int r, int c) { return c ^ (r & 15); }

// gather + mean of BM target rows into the swizzled LDS tile At [BM][2D] (see tr_fwd2):
// item = (used row, 8-column chunk), two items per thread, every leaf load of both in
// flight; padding ids (-1) read row 0 and are zeroed at use; only the Fg + 1 used slots of
// each sibling group are gathered (F2_SKIP_PAD), the unused slots' rows are zero-filled.
template <typename FT, int BM, int NT>
__device__ __forceinline__ void f2_gather(const TrFwdArgs& a, bf16_t* At, const int32_t* node_s,
                                          const int32_t* leaf_s, int tid) {
  const int D = a.D, K2 = 2 * D;
  const FT* x = static_cast<const FT*>(a.x);
  const int cpr = D >> 3;
  const int P = 1 << a.logPg, U = F2_SKIP_PAD ? a.Fg + 1 : P;
  const int nitems = (BM >> a.logPg) * U * cpr;
  constexpr int G = Feat8<FT>::kInFlight;
  if (F2_SKIP_PAD && U < P) {
    const int pad = P - U, nch = K2 >> 3;
    for (int it = tid; it < (BM >> a.logPg) * pad * nch; it += NT) {
      const int q = it / nch, c = it - q * nch;
      const int r = (q / pad) * P + U + q % pad;
      *reinterpret_cast<uint4_t*>(At + r * K2 + f2_chunk(r, c) * 8) = uint4_t{0u, 0u, 0u, 0u};
    }
  }
  for (int it = tid; it < nitems; it += 2 * NT) {
    const int itb = it + NT;
    const bool hb = itb < nitems;
    const int qa = it / cpr, ca = it - qa * cpr;
    const int qb = hb ? itb / cpr : qa, cb = hb ? itb - qb * cpr : ca;
    const int ra = (qa / U) * P + qa % U, rb = (qb / U) * P + qb % U;
    const int32_t na = node_s[ra], nb = hb ? node_s[rb] : -1;
    Feat8<FT> sa, sb;
    float acc_a[8], acc_b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc_a[i] = acc_b[i] = 0.f;
    sa.load(x + static_cast<int64_t>(na > 0 ? na : 0) * D + ca * 8);
    sb.load(x + static_cast<int64_t>(nb > 0 ? nb : 0) * D + cb * 8);
    for (int k = 0; k < a.FL; k += G) {
      int32_t ja[G], jb[G];
      Feat8<FT> va[G], vb[G];
#pragma unroll
      for (int u = 0; u < G; ++u) {
        ja[u] = (k + u < a.FL) ? leaf_s[ra * a.FL + k + u] : -1;
        jb[u] = (hb && k + u < a.FL) ? leaf_s[rb * a.FL + k + u] : -1;
      }
#pragma unroll
      for (int u = 0; u < G; ++u) {
        va[u].load(x + static_cast<int64_t>(ja[u] > 0 ? ja[u] : 0) * D + ca * 8);
        vb[u].load(x + static_cast<int64_t>(jb[u] > 0 ? jb[u] : 0) * D + cb * 8);
      }
#pragma unroll
      for (int u = 0; u < G; ++u) {
        va[u].keep(ja[u] >= 0);
        vb[u].keep(jb[u] >= 0);
        va[u].add_to(acc_a);
        vb[u].add_to(acc_b);
      }
    }
    sa.keep(na >= 0);
    sb.keep(nb >= 0);
    if (a.include_self) {
      sa.add_to(acc_a);
      sb.add_to(acc_b);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      acc_a[i] *= a.inv_leaf;
      acc_b[i] *= a.inv_leaf;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h == 1 && !hb) break;
      const int r = h ? rb : ra, c = h ? cb : ca;
      *reinterpret_cast<uint4_t*>(At + r * K2 + f2_chunk(r, c) * 8) = h ? sb.bf16() : sa.bf16();
      *reinterpret_cast<uint4_t*>(At + r * K2 + f2_chunk(r, cpr + c) * 8) = pack_bf16x8(h ? acc_b : acc_a);
    }
  }
}

// the A tile -> kt layout (dW operand): item = (column pair, 8-row chunk), column pairs
// fastest: a half-wave's 4-byte reads cover 128 contiguous (permuted) bytes of a row
template <int BM, int NT>
__device__ __forceinline__ void f2_kt(const TrFwdArgs& a, int64_t row0, const bf16_t* At, int tid) {
  const int K2 = 2 * a.D;
  const int np = K2 >> 1;
  for (int it = tid; it < np * (BM / 8); it += NT) {
    const int q = it / np;
    const int n = (it - q * np) * 2;
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = q * 8 + i;
      w[i] = *reinterpret_cast<const uint32_t*>(At + r * K2 + f2_chunk(r, n >> 3) * 8 + (n & 7));
    }
    uint4_t lo, hi;
    kt_pack8(w, lo, hi);
    *reinterpret_cast<uint4_t*>(a.a_kt + kt_off(row0 + q * 8, n, K2)) = lo;
    *reinterpret_cast<uint4_t*>(a.a_kt + kt_off(row0 + q * 8, n + 1, K2)) = hi;
  }
}

// one 32-row gather tile of the pipelined step (extra blocks of the optimizer launch, 256
// threads): ids -> gather + mean -> LDS -> kt copy (dW operand) + row-major A rows (the
// GEMM-only forward's input).  LDS: A tile [32][2D] + ids (eh_tr_gather32_lds).
constexpr int kG32Rows = 32, kG32Threads = 256;

template <typename FT>
__device__ __forceinline__ void tr_gather32_tile(const TrFwdArgs& a, int tile, bf16_t* lds) {
  constexpr int BM = kG32Rows, NT = kG32Threads;
  const int K2 = 2 * a.D, tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(tile) * BM;
  bf16_t* At = lds;
  int32_t* node_s = reinterpret_cast<int32_t*>(lds + BM * K2);
  int32_t* leaf_s = node_s + BM;
  if (tid < BM) node_s[tid] = a.nodes[row0 + tid];
  for (int it = tid; it < BM * a.FL; it += NT) leaf_s[it] = a.leaf[row0 * a.FL + it];
  __syncthreads();
  f2_gather<FT, BM, NT>(a, At, node_s, leaf_s, tid);
  __syncthreads();
  f2_kt<BM, NT>(a, row0, At, tid);
  const int cpr2 = K2 >> 3;
  for (int it = tid; it < BM * cpr2; it += NT) {
    const int r = it / cpr2, c = it - r * cpr2;
    *reinterpret_cast<uint4_t*>(a.a_rows + (row0 + r) * K2 + c * 8) =
        *reinterpret_cast<const uint4_t*>(At + r * K2 + f2_chunk(r, c) * 8);
  }
}

}  // namespace euler_hip
