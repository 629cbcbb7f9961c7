// The tile kernels of the fused GCN training step (launch sequence: gcn_args.h; overview:
// gcn.hip): the edge-parallel aggregation of a 16-target tile, the MFMA operand reads from LDS
// images, the outer layer and the head.  A header, so that the head's two loss instantiations
// compile in translation units of their own: gcn.hip (sigmoid, with the layer launch) and
// gcn_head_softmax.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "hip/gcn_args.h"
#include "hip/sampling_math.h"
#include "hip/tile.h"

namespace euler_hip {

// ----------------------------------------------------------------------------
// edge-parallel weighted aggregation of a 16-target tile into an LDS fp32 accumulator
// acc[16][KP + 1]:  acc[t] = sum_e rsqrt(deg_t) rsqrt(deg_s[src_e]) x[src_e]  (+ self loop)
// ----------------------------------------------------------------------------
constexpr int kGT = 16;  // targets per tile

template <int KP, int NT = 256>
struct AggTile {
  static constexpr int NCH = KP / 8;     // column chunks of 8 (one lane each)
  static constexpr int NW = NT / NCH;    // workers per block of NT threads
  static constexpr int LDA = KP + 1;     // fp32 accumulator row stride (bank spread)
};

// one row chunk (8 columns) as loaded: bf16 rows stay packed (4 dwords) until they are
// accumulated, so a worker keeps twice as many rows in flight in the same registers
template <bool F32>
struct RowRaw {
  uint32_t w[F32 ? 8 : 4];
};

template <bool F32>
__device__ __forceinline__ void row_load(const GcnAggSrc& s, int32_t row, int c, RowRaw<F32>& r) {
  if (row < 0 || c * 8 >= s.cols) {
#pragma unroll
    for (int j = 0; j < (F32 ? 8 : 4); ++j) r.w[j] = 0u;
    return;
  }
  if constexpr (F32) {
    const float* p = static_cast<const float*>(s.x) + static_cast<int64_t>(row) * s.ld + c * 8;
    const uint4_t lo = *reinterpret_cast<const uint4_t*>(p);
    const uint4_t hi = *reinterpret_cast<const uint4_t*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r.w[j] = lo[j];
      r.w[4 + j] = hi[j];
    }
  } else {
    const uint4_t v =
        *reinterpret_cast<const uint4_t*>(static_cast<const bf16_t*>(s.x) + static_cast<int64_t>(row) * s.ld + c * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) r.w[j] = v[j];
  }
}

template <bool F32>
__device__ __forceinline__ void row_axpy(const RowRaw<F32>& r, float w, float* run) {
  if constexpr (F32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) run[j] += w * __uint_as_float(r.w[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      run[2 * j] += w * __uint_as_float(r.w[j] << 16);
      run[2 * j + 1] += w * __uint_as_float(r.w[j] & 0xffff0000u);
    }
  }
}

// enode: neighbour node ids of the hop (by-id sources read row = enode[e]); self_src:
// nullable (target t's self-loop source is t) ; nt: real targets
// per-target prelude (threads < 16, once per tile): rsqrt of the target degree, the self
// loop's source and source row, so the self items of the main loop need no extra round.
// Each worker (NCH lanes, one per 8 columns) walks a contiguous slice of the tile's edges,
// U per batch, software-pipelined: the next batch's index loads are in flight while the
// current batch's rows are accumulated, and its rows (+ source degrees) are issued before
// the loop comes back — one memory round trip per batch instead of two.
template <int KP, bool F32, int NT>
__device__ void gcn_aggregate_t(const GcnAggSrc& src, const int32_t* off, const int32_t* etgt, const int32_t* esrc,
                                const int32_t* enode, const int32_t* deg_s, const int32_t* self_src, int self_loops,
                                int64_t t0, int nt, float* acc, float* rdt, int* sself) {
  using AT = AggTile<KP, NT>;
  const int tid = threadIdx.x;
  for (int i = tid; i < kGT * AT::LDA; i += NT) acc[i] = 0.f;
  __shared__ int64_t s_e[2];
  __shared__ int s_row[kGT];
  if (tid == 0) {
    s_e[0] = off[t0];
    s_e[1] = off[t0 + kGT];
  }
  if (tid < kGT) {
    const int64_t t = t0 + tid;
    const int dt = t < nt ? static_cast<int>(off[t + 1] - off[t]) + self_loops : 0;
    rdt[tid] = dt > 0 ? rsqrtf(static_cast<float>(dt)) : 0.f;
    const int ss = t < nt ? (self_src ? self_src[t] : static_cast<int>(t)) : -1;
    sself[tid] = ss;
    s_row[tid] = ss < 0 ? -1 : (src.by_id ? src.set[ss] : ss);
  }
  __syncthreads();
  const int64_t e0 = s_e[0], E = s_e[1] - s_e[0];
  const int nself = self_loops ? static_cast<int>(nt - t0 < kGT ? (nt - t0 > 0 ? nt - t0 : 0) : kGT) : 0;
  const int64_t W = E + nself;
  const int g = tid / AT::NCH, c = tid % AT::NCH;
  const int64_t per = (W + AT::NW - 1) / AT::NW;
  const int64_t i0 = g * per, i1 = (i0 + per) < W ? (i0 + per) : W;
  constexpr int U = F32 ? 4 : 8;  // the same 32 dwords of rows in flight per batch
  float run[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int cur = -1;
  auto flush = [&]() {
    if (cur >= 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) atomicAdd(&acc[cur * AT::LDA + c * 8 + j], run[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) run[j] = 0.f;
  };
  auto load_idx = [&](int64_t i, int* tl, int* sv, int* row) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ii = i + u;
      tl[u] = -1;
      sv[u] = -1;
      row[u] = -1;
      if (ii < i1) {
        if (ii < E) {
          const int64_t e = e0 + ii;
          tl[u] = static_cast<int>(etgt[e] - t0);
          sv[u] = esrc[e];
          row[u] = src.by_id ? enode[e] : sv[u];
        } else {
          tl[u] = static_cast<int>(ii - E);
          sv[u] = sself[tl[u]];
          row[u] = s_row[tl[u]];
        }
      }
    }
  };
  auto load_rows = [&](const int* sv, const int* row, float* ds, RowRaw<F32>* x) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ds[u] = sv[u] >= 0 ? static_cast<float>(deg_s[sv[u]]) : 1.f;
      row_load<F32>(src, sv[u] >= 0 ? row[u] : -1, c, x[u]);
    }
  };
  int tl0[U], s0[U], r0[U];
  float ds0[U];
  RowRaw<F32> x0[U];
  if (i0 < i1) {
    load_idx(i0, tl0, s0, r0);
    load_rows(s0, r0, ds0, x0);
  }
  for (int64_t i = i0; i < i1; i += U) {
    int tl1[U], s1[U], r1[U];
    const bool more = i + U < i1;
    if (more) load_idx(i + U, tl1, s1, r1);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (tl0[u] < 0 || s0[u] < 0) continue;
      if (tl0[u] != cur) {
        flush();
        cur = tl0[u];
      }
      row_axpy<F32>(x0[u], rdt[tl0[u]] * rsqrtf(ds0[u]), run);
    }
    if (!more) break;
    load_rows(s1, r1, ds0, x0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      tl0[u] = tl1[u];
      s0[u] = s1[u];
    }
  }
  flush();
  __syncthreads();
}

template <int KP, int NT = 256>
__device__ void gcn_aggregate(const GcnAggSrc& src, const int32_t* off, const int32_t* etgt, const int32_t* esrc,
                              const int32_t* enode, const int32_t* deg_s, const int32_t* self_src, int self_loops,
                              int64_t t0, int nt, float* acc, float* rdt, int* sself) {
  if (src.x_fp32)
    gcn_aggregate_t<KP, true, NT>(src, off, etgt, esrc, enode, deg_s, self_src, self_loops, t0, nt, acc, rdt, sself);
  else
    gcn_aggregate_t<KP, false, NT>(src, off, etgt, esrc, enode, deg_s, self_src, self_loops, t0, nt, acc, rdt, sself);
}

// ----------------------------------------------------------------------------
// MFMA operand reads from row-major bf16 LDS images
// ----------------------------------------------------------------------------
__device__ __forceinline__ uint4_t lds16(const bf16_t* p) { return *reinterpret_cast<const uint4_t*>(p); }

// standard fragment: row r0 + (lane & 15), k = k0 + 8 (lane >> 4) .. +7
__device__ __forceinline__ uint4_t frag_std(const bf16_t* img, int ld, int r0, int k0, int lane) {
  return lds16(img + (r0 + (lane & 15)) * ld + k0 + (lane >> 4) * 8);
}
// the k permutation of tl_tr_frag: lane group g holds k0 + 4g .. +3 and k0 + 16 + 4g .. +3
__device__ __forceinline__ uint4_t frag_perm(const bf16_t* img, int ld, int r0, int k0, int lane) {
  const bf16_t* p = img + (r0 + (lane & 15)) * ld + k0 + (lane >> 4) * 4;
  const tl_uint2 lo = *reinterpret_cast<const tl_uint2*>(p);
  const tl_uint2 hi = *reinterpret_cast<const tl_uint2*>(p + 16);
  return uint4_t{lo[0], lo[1], hi[0], hi[1]};
}
template <int LD>
__device__ __forceinline__ uint4_t frag_tr(const bf16_t* img, int e0, int c0, int lane) {
  return tl_tr_frag<LD>(img, e0, c0, lane);
}

// stage an fp32 [rows][cols] matrix into a bf16 LDS image [rowsp][ld] (zero padding)
__device__ __forceinline__ void stage_w(const float* w, int rows, int cols, int rowsp, int colsp, bf16_t* img,
                                        int ld) {
  for (int i = threadIdx.x; i < rowsp * (colsp >> 1); i += 256) {
    const int r = i / (colsp >> 1), c = (i - r * (colsp >> 1)) * 2;
    const float a = (r < rows && c < cols) ? w[static_cast<int64_t>(r) * cols + c] : 0.f;
    const float b = (r < rows && c + 1 < cols) ? w[static_cast<int64_t>(r) * cols + c + 1] : 0.f;
    *reinterpret_cast<uint32_t*>(img + r * ld + c) = pack_bf16x2(a, b);
  }
}

// copy a staged bf16 image (global, 16-byte multiples) into LDS: every load in flight
template <int NT = 256>
__device__ __forceinline__ void copy_img(const uint16_t* src, bf16_t* dst, int n) {
  const uint4_t* s = reinterpret_cast<const uint4_t*>(src);
  uint4_t* d = reinterpret_cast<uint4_t*>(dst);
  const int n16 = n >> 3;
  constexpr int U = 8;
  for (int i0 = threadIdx.x; i0 < n16; i0 += NT * U) {
    uint4_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + u * NT < n16) v[u] = s[i0 + u * NT];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + u * NT < n16) d[i0 + u * NT] = v[u];
  }
}

__device__ __forceinline__ void zero_img(bf16_t* img, int n) {
  for (int i = threadIdx.x; i < (n >> 1); i += 256) reinterpret_cast<uint32_t*>(img)[i] = 0u;
}

// LDS image stride for a width: the tl_tr_frag bank-spreading strides (tile.h)
__host__ __device__ constexpr int img_ld(int w) { return w <= 64 ? 80 : 144; }

// ----------------------------------------------------------------------------
// layer (L = 2): targets S_1 in tiles of 16, sources S_2 (feature rows by node id)
// ----------------------------------------------------------------------------
// threads per 16-target tile of the layer launch (512 measured slower on PPI: 33.4 vs
// 25.2 us, profiles/r5_gcn/fused_v3/ — the tile's LDS flushes contend and fewer tiles
// are resident)
constexpr int kGcnLayerThreads = 256;

template <int KP, int HP>
__global__ __launch_bounds__(kGcnLayerThreads) void gcn_layer_kernel(GcnLayerArgs a) {
  constexpr int NT = kGcnLayerThreads;
  constexpr int LDK = img_ld(KP), LDAcc = AggTile<KP, NT>::LDA;
  __shared__ __attribute__((aligned(16))) bf16_t wimg[HP * LDK];
  __shared__ __attribute__((aligned(16))) bf16_t aimg[kGT * LDK];
  __shared__ float acc[kGT * LDAcc];
  __shared__ float rdt[kGT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = a.cnt[1];
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kGT;
  if (t0 >= nt) return;  // uniform: rows past the set are never read
  copy_img<NT>(a.wimg, wimg, HP * LDK);
  __shared__ int sself[kGT];
  gcn_aggregate<KP, NT>(a.src, a.off, a.etgt, a.esrc, a.enode, a.deg_s, nullptr, a.self_loops, t0, nt, acc, rdt,
                        sself);
  // aggregate -> bf16 image + the dW operand rows
  for (int i = tid; i < kGT * (KP / 2); i += NT) {
    const int r = i / (KP / 2), c = (i - r * (KP / 2)) * 2;
    const uint32_t pk = pack_bf16x2(acc[r * LDAcc + c], acc[r * LDAcc + c + 1]);
    *reinterpret_cast<uint32_t*>(aimg + r * LDK + c) = pk;
    *reinterpret_cast<uint32_t*>(a.agg_out + (t0 + r) * KP + c) = pk;
  }
  __syncthreads();
  // z = agg W^T, h = relu(z): wave w -> 16-column tiles w, w + NT / 64, ...
  for (int ct = wave; ct < HP / 16; ct += NT / 64) {
    float4_t z = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < KP; k0 += 32)
      z = mfma16(frag_std(aimg, LDK, 0, k0, lane), frag_std(wimg, LDK, ct * 16, k0, lane), z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = (lane >> 4) * 4 + j;
      a.h_out[(t0 + r) * HP + ct * 16 + (lane & 15)] = f2bf(fmaxf(z[j], 0.f));
    }
  }
}

// ----------------------------------------------------------------------------
// head: 16 roots per block; the last conv, fc, out_fc, loss and the row-local backward.
// Images: weights [out][in] bf16 (the fc / out_fc images at stride 144: E, C <= 128),
// activations [32 rows][width] with rows 16..31 zero (the k = 32 of the row-reduction
// MFMAs of the weight gradients).
// ----------------------------------------------------------------------------
constexpr int kWide = 144;  // LDS stride of the E- and C-wide images

__host__ __device__ inline size_t gcn_head_lds_bytes(int KP, int HP, int EP, int CP) {
  const int LK = img_ld(KP), LH = img_ld(HP);
  const size_t bf = static_cast<size_t>(HP) * LK + static_cast<size_t>(EP) * LH + static_cast<size_t>(CP) * kWide +
                    32 * LK + 32 * LH + 32 * kWide * 3 + 32 * LH;
  return bf * 2 + static_cast<size_t>(kGT) * (KP + 1) * 4 + kGT * 4 + static_cast<size_t>(kGT) * CP * 4 + 64;
}

// LOSS == kGcnLossSoftmax splits the logits phase in two around one more barrier: a row's
// statistics span the Cp / 16 <= 8 logits tiles, which the block's four waves hold between them
// (wave w: tiles w and w + 4, kept in registers across the barrier).
//   partials  per (row, tile), over the tile's 16 column lanes (xor shuffles inside the lane
//             group): max, sum exp(x - max), arg-max column, label sum, label arg-max column
//             -> sm[row][tile]; padded columns and rows beyond B enter none of them
//   merge     every wave merges its rows' tiles 0 .. ceil(C / 16) - 1 in tile order (a fixed
//             order and no atomics: the same bits in every launch) into m, Z and the label sum s,
//             and finishes its own tiles: p = exp(x - m) / Z, d = bf16((s p - y) / B),
//             row loss = sum_c y_c (m + log Z - x_c); wave 0 counts the rows whose arg-max
//             (ties: the lowest column) is the label row's: tp = correct, fp = fn = wrong
constexpr int kGcnSmTiles = 8;  // Cp <= 128
constexpr int kGcnSmStats = 5;  // max, sum, arg-max, label sum, label arg-max (its value: the label tile in LDS)
constexpr size_t kGcnSmLdsBytes = sizeof(float) * kGT * kGcnSmTiles * kGcnSmStats;  // static, beside the images

// the softmax instantiations' launch (gcn_head_softmax.hip); eh_gcn_head validates and calls it
hipError_t gcn_head_softmax_launch(const GcnHeadArgs& a, dim3 grid, size_t lds, hipStream_t s);

// the table lives in static LDS of the softmax instantiation only
template <int LOSS>
__device__ __forceinline__ float* gcn_sm_table() {
  if constexpr (LOSS == kGcnLossSoftmax) {
    __shared__ float sm[kGT * kGcnSmTiles * kGcnSmStats];
    return sm;
  } else {
    return nullptr;
  }
}

// (max, its lowest column) and the sum over the 16 column lanes of a tile row; every lane ends
// with the same bits (the butterfly combines the same pairs in every lane)
__device__ __forceinline__ void gcn_argmax16(float& m, int& am) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) {
      m = om;
      am = oa;
    }
  }
}
__device__ __forceinline__ float gcn_sum16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int KP, int HP, int LOSS>
__global__ __launch_bounds__(256) void gcn_head_kernel(GcnHeadArgs a) {
  constexpr int LK = img_ld(KP), LH = img_ld(HP), LE = kWide, LC = kWide;
  const int EP = a.Ep, CP = a.Cp;
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* Wl = lds;                 // [HP][LK] last conv W [out][in]
  bf16_t* Wf = Wl + HP * LK;        // [EP][LH] fc W [E][H]
  bf16_t* Wo = Wf + EP * LH;        // [CP][LE] out W [C][E]
  bf16_t* Ag = Wo + CP * LE;        // [32][LK] aggregate
  bf16_t* H0 = Ag + 32 * LK;        // [32][LH] relu(z)
  bf16_t* Em = H0 + 32 * LH;        // [32][LE] emb
  bf16_t* Dl = Em + 32 * LE;        // [32][LC] d logits
  bf16_t* De = Dl + 32 * LC;        // [32][LE] d emb
  bf16_t* Dz = De + 32 * LE;        // [32][LH] d z (ReLU mask applied)
  float* acc = reinterpret_cast<float*>(Dz + 32 * LH);  // [16][KP + 1]
  float* rdt = acc + kGT * AggTile<KP>::LDA;
  __shared__ float red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kGT;
  const int blk = blockIdx.x;
  // the weights (fp32 masters -> bf16) and cleared activation images
  __shared__ int sself[kGT];
  __shared__ int s_root[kGT];
  float* lab = rdt + kGT;  // [16][CP] the tile's dense labels
#define GH_STAMP(k) \
  if (a.prof && threadIdx.x == 0) a.prof[static_cast<int64_t>(blockIdx.x) * 16 + (k)] = wall_clock64()
  GH_STAMP(0);
  if (a.ostep_inc && blk == 0 && tid == 0) a.ostep_inc[0] += 1;  // read by this step's reduce launch
  if (tid < kGT) s_root[tid] = t0 + tid < a.B ? a.roots[t0 + tid] : -1;
  copy_img(a.wl_img, Wl, HP * LK);
  copy_img(a.wfc_img, Wf, EP * LH);
  copy_img(a.wout_img, Wo, CP * LE);
  zero_img(Ag, 32 * LK + 32 * LH + 32 * LE * 3 + 32 * LH);
  __syncthreads();
  GH_STAMP(1);
  {  // every label load in flight at once (16 x CP <= 2048 values: 8 per thread)
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = tid + u * 256;
      const int r = i / CP, c = i - r * CP;
      const int32_t root = i < kGT * CP ? s_root[r] : -1;
      v[u] = (root >= 0 && c < a.C) ? a.labels[static_cast<int64_t>(root) * a.C + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (tid + u * 256 < kGT * CP) lab[tid + u * 256] = v[u];
  }
  gcn_aggregate<KP>(a.src, a.off, a.etgt, a.esrc, a.enode, a.deg_s, a.rself, a.self_loops, t0, a.B, acc, rdt,
                    sself);
  for (int i = tid; i < kGT * (KP / 2); i += 256) {
    const int r = i / (KP / 2), c = (i - r * (KP / 2)) * 2;
    *reinterpret_cast<uint32_t*>(Ag + r * LK + c) = pack_bf16x2(acc[r * AggTile<KP>::LDA + c],
                                                                acc[r * AggTile<KP>::LDA + c + 1]);
    if (a.dbg_agg && t0 + r < a.B) {
      a.dbg_agg[(t0 + r) * KP + c] = acc[r * AggTile<KP>::LDA + c];
      a.dbg_agg[(t0 + r) * KP + c + 1] = acc[r * AggTile<KP>::LDA + c + 1];
    }
  }
  __syncthreads();
  GH_STAMP(2);
  // z = Ag Wl^T -> H0 = relu(z)
  for (int ct = wave; ct < HP / 16; ct += 4) {
    float4_t z = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < KP; k0 += 32)
      z = mfma16(frag_std(Ag, LK, 0, k0, lane), frag_std(Wl, LK, ct * 16, k0, lane), z);
#pragma unroll
    for (int j = 0; j < 4; ++j) H0[(lg * 4 + j) * LH + ct * 16 + lr] = f2bf(fmaxf(z[j], 0.f));
  }
  __syncthreads();
  GH_STAMP(3);
  // emb = H0 Wf^T + bfc
  for (int ct = wave; ct < EP / 16; ct += 4) {
    float4_t z = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < HP; k0 += 32)
      z = mfma16(frag_std(H0, LH, 0, k0, lane), frag_std(Wf, LH, ct * 16, k0, lane), z);
    const int col = ct * 16 + lr;
    const float b = col < a.E ? a.bfc[col] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) Em[(lg * 4 + j) * LE + col] = f2bf(col < a.E ? z[j] + b : 0.f);
  }
  __syncthreads();
  GH_STAMP(4);
  // logits = emb Wo^T -> loss, F1 counts, d logits
  float lsum = 0.f, tp = 0.f, fp = 0.f, fn = 0.f;
  if constexpr (LOSS == kGcnLossSoftmax) {
    float* const sm = gcn_sm_table<LOSS>();
    const int ntl = (a.C + 15) >> 4;  // tiles with a real column (1 .. CP / 16)
    float4_t x[2];                    // the wave's logits tiles wave, wave + 4 across the merge
    // partials
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int ct = wave + 4 * q;
      x[q] = float4_t{0.f, 0.f, 0.f, 0.f};
      if (ct >= CP / 16) continue;
      for (int k0 = 0; k0 < EP; k0 += 32)
        x[q] = mfma16(frag_std(Em, LE, 0, k0, lane), frag_std(Wo, LE, ct * 16, k0, lane), x[q]);
      const int col = ct * 16 + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = lg * 4 + j;
        const bool valid = t0 + r < a.B && col < a.C;
        const float y = lab[r * CP + col];  // zero in padded columns and rows beyond B
        float mx = valid ? x[q][j] : -INFINITY, ym = valid ? y : -INFINITY;
        int am = col, ya = col;
        gcn_argmax16(mx, am);
        gcn_argmax16(ym, ya);
        const float ze = gcn_sum16(valid ? __expf(x[q][j] - mx) : 0.f);
        const float ys = gcn_sum16(y);
        if (lr == 0) {
          float* st = sm + (r * kGcnSmTiles + ct) * kGcnSmStats;
          st[0] = mx;
          st[1] = ze;
          st[2] = __int_as_float(am);
          st[3] = ys;
          st[4] = __int_as_float(ya);
        }
      }
    }
    __syncthreads();
    // merge: each lane one row of its lane group (lg * 4 + (lr & 3)), handed to the lanes that
    // hold the row's elements below
    float M, Z = 0.f, S = 0.f;
    {
      const float* st = sm + (lg * 4 + (lr & 3)) * kGcnSmTiles * kGcnSmStats;
      M = st[0];
      for (int t = 1; t < ntl; ++t) M = fmaxf(M, st[t * kGcnSmStats]);
      if (!(M > -INFINITY)) M = 0.f;  // a row beyond B: Z = 0, and nothing below reads it
      for (int t = 0; t < ntl; ++t) {
        Z += st[t * kGcnSmStats + 1] * __expf(st[t * kGcnSmStats] - M);
        S += st[t * kGcnSmStats + 3];
      }
    }
    const float lse = M + logf(Z);
    float mj[4], zj[4], sj[4], lj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int from = (lane & 48) + j;
      mj[j] = __shfl(M, from, 64);
      zj[j] = __shfl(Z, from, 64);
      sj[j] = __shfl(S, from, 64);
      lj[j] = __shfl(lse, from, 64);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int ct = wave + 4 * q;
      if (ct >= CP / 16) continue;
      const int col = ct * 16 + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = lg * 4 + j;
        const bool valid = t0 + r < a.B && col < a.C;
        const float y = lab[r * CP + col];
        const float p = valid ? __expf(x[q][j] - mj[j]) / zj[j] : 0.f;
        if (valid) lsum += y * (lj[j] - x[q][j]);
        Dl[r * LC + col] = f2bf(valid ? (sj[j] * p - y) * a.inv_scale : 0.f);
      }
    }
    if (wave == 0) {  // lanes 0..15: row = lane; the label maxima are read back from the label tile
      const int r = lr;
      const float* st = sm + r * kGcnSmTiles * kGcnSmStats;
      float bm = st[0];
      int am = __float_as_int(st[2]), ya = __float_as_int(st[4]);
      float by = lab[r * CP + ya];
      for (int t = 1; t < ntl; ++t) {  // ties stay with the lower tile
        if (st[t * kGcnSmStats] > bm) {
          bm = st[t * kGcnSmStats];
          am = __float_as_int(st[t * kGcnSmStats + 2]);
        }
        const int c = __float_as_int(st[t * kGcnSmStats + 4]);
        const float v = lab[r * CP + c];
        if (v > by) {
          by = v;
          ya = c;
        }
      }
      const bool row = lane < 16 && t0 + r < a.B;
      tp = (row && am == ya) ? 1.f : 0.f;
      fp = fn = (row && am != ya) ? 1.f : 0.f;
    }
  } else {
    for (int ct = wave; ct < CP / 16; ct += 4) {
      float4_t z = float4_t{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < EP; k0 += 32)
        z = mfma16(frag_std(Em, LE, 0, k0, lane), frag_std(Wo, LE, ct * 16, k0, lane), z);
      const int col = ct * 16 + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = lg * 4 + j;
        const int64_t t = t0 + r;
        float d = 0.f;
        if (t < a.B && col < a.C) {
          const float y = lab[r * CP + col];
          const float x = z[j];
          lsum += fmaxf(x, 0.f) - x * y + log1pf(__expf(-fabsf(x)));
          const bool pred = x >= 0.f, pos = y > 0.5f;
          tp += (pred && pos) ? 1.f : 0.f;
          fp += (pred && !pos) ? 1.f : 0.f;
          fn += (!pred && pos) ? 1.f : 0.f;
          d = (1.f / (1.f + __expf(-x)) - y) * a.inv_scale;
        }
        Dl[r * LC + col] = f2bf(d);
      }
    }
  }
  lsum = wave_sum(lsum);
  tp = wave_sum(tp);
  fp = wave_sum(fp);
  fn = wave_sum(fn);
  if (lane == 0) {
    red[wave][0] = lsum;
    red[wave][1] = tp;
    red[wave][2] = fp;
    red[wave][3] = fn;
  }
  __syncthreads();
  GH_STAMP(5);
  if (tid < 4) {  // the mean loss's share of this block; raw F1 counts
    const float v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    a.part_stat[blk * 4 + tid] = tid == 0 ? v * a.inv_scale : v;
  }
  // d emb = d logits Wo (K = C: the rows of Wo are the reduction index); d bfc partial
  for (int ct = wave; ct < EP / 16; ct += 4) {
    float4_t z = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < CP; k0 += 32)
      z = mfma16(frag_perm(Dl, LC, 0, k0, lane), frag_tr<LE>(Wo, k0, ct * 16, lane), z);
    const int col = ct * 16 + lr;
    float cs = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      De[(lg * 4 + j) * LE + col] = f2bf(z[j]);
      cs += z[j];
    }
    cs += __shfl_xor(cs, 16, 64);
    cs += __shfl_xor(cs, 32, 64);
    if (lg == 0) a.part_bfc[static_cast<int64_t>(blk) * EP + col] = cs;
  }
  __syncthreads();
  GH_STAMP(6);
  // d z = (d emb Wf) * relu'(z)   (K = E: the rows of Wf are the reduction index)
  for (int ct = wave; ct < HP / 16; ct += 4) {
    float4_t z = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < EP; k0 += 32)
      z = mfma16(frag_perm(De, LE, 0, k0, lane), frag_tr<LH>(Wf, k0, ct * 16, lane), z);
    const int col = ct * 16 + lr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = lg * 4 + j;
      Dz[r * LH + col] = f2bf(bf_pos(H0[r * LH + col]) ? z[j] : 0.f);
    }
  }
  __syncthreads();
  GH_STAMP(7);
  // weight-gradient partials of this block's rows (k = the 32 image rows, 16..31 zero):
  // d out W = Dl^T Em [CP][EP], d fc W = De^T H0 [EP][HP], d conv W = Dz^T Ag [HP][KP]
  {
    const int n1 = (CP / 16) * (EP / 16), n2 = (EP / 16) * (HP / 16);
    constexpr int n3 = (HP / 16) * (KP / 16);
    for (int j = wave; j < n1 + n2 + n3; j += 4) {
      float4_t z = float4_t{0.f, 0.f, 0.f, 0.f};
      float* out;
      int ld, r0, c0;
      if (j < n1) {
        r0 = (j / (EP / 16)) * 16;
        c0 = (j % (EP / 16)) * 16;
        z = mfma16(frag_tr<LC>(Dl, 0, r0, lane), frag_tr<LE>(Em, 0, c0, lane), z);
        out = a.part_out + static_cast<int64_t>(blk) * CP * EP;
        ld = EP;
      } else if (j < n1 + n2) {
        const int q = j - n1;
        r0 = (q / (HP / 16)) * 16;
        c0 = (q % (HP / 16)) * 16;
        z = mfma16(frag_tr<LE>(De, 0, r0, lane), frag_tr<LH>(H0, 0, c0, lane), z);
        out = a.part_fc + static_cast<int64_t>(blk) * EP * HP;
        ld = HP;
      } else {
        const int q = j - n1 - n2;
        r0 = (q / (KP / 16)) * 16;
        c0 = (q % (KP / 16)) * 16;
        z = mfma16(frag_tr<LH>(Dz, 0, r0, lane), frag_tr<LK>(Ag, 0, c0, lane), z);
        out = a.part_w + static_cast<int64_t>(blk) * HP * KP;
        ld = KP;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) out[static_cast<int64_t>(r0 + lg * 4 + q) * ld + c0 + lr] = z[q];
    }
  }
  if (a.dagg == nullptr) {  // L = 1: no layer below
    GH_STAMP(15);
    return;
  }
  // d agg = Dz Wl (K = H: the rows of Wl are the reduction index) -> the fp32 accumulator
  __syncthreads();
  GH_STAMP(8);
  for (int ct = wave; ct < KP / 16; ct += 4) {
    float4_t z = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < HP; k0 += 32)
      z = mfma16(frag_perm(Dz, LH, 0, k0, lane), frag_tr<LK>(Wl, k0, ct * 16, lane), z);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[(lg * 4 + j) * AggTile<KP>::LDA + ct * 16 + lr] = z[j];
  }
  __syncthreads();
  GH_STAMP(9);
  // d agg rows to global: gcn_dw_kernel reads them per hop-0 edge (no d h1 scatter)
  for (int i = tid; i < kGT * KP; i += 256) {
    const int r = i / KP, c = i - r * KP;
    if (t0 + r < a.B) a.dagg[(t0 + r) * KP + c] = acc[r * AggTile<KP>::LDA + c];
  }
  GH_STAMP(15);
#undef GH_STAMP
}

}  // namespace euler_hip

// host: one instantiation per padded (input, conv) width pair
#define GCN_DISPATCH(KP, HP, KERNEL, ...)                                            \
  do {                                                                              \
    if ((KP) == 32 && (HP) == 32) KERNEL(32, 32, __VA_ARGS__);                      \
    else if ((KP) == 32 && (HP) == 64) KERNEL(32, 64, __VA_ARGS__);                 \
    else if ((KP) == 64 && (HP) == 32) KERNEL(64, 32, __VA_ARGS__);                 \
    else if ((KP) == 64 && (HP) == 64) KERNEL(64, 64, __VA_ARGS__);                 \
    else if ((KP) == 128 && (HP) == 32) KERNEL(128, 32, __VA_ARGS__);               \
    else KERNEL(128, 64, __VA_ARGS__);                                              \
  } while (0)

#define GCN_HEAD_LOSS(K, H, LOSS, grid, lds, s, A)                                                          \
  do {                                                                                                     \
    if ((lds) > 65536)                                                                                     \
      EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gcn_head_kernel<K, H, LOSS>),     \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds))); \
    hipLaunchKernelGGL((gcn_head_kernel<K, H, LOSS>), grid, dim3(256), lds, s, A);                        \
  } while (0)
