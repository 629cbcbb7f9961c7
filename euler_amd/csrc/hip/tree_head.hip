// The head launches of the fused GraphSAGE tree step (overview: tree_fwd.hip): tr_head_kernel
// (last conv + fc + out_fc + sigmoid or softmax CE + backward to dA, and the next step's sampler on the
// CUs it leaves idle) and tr_pair_head_kernel (the two towers of the unsupervised model), with
// the 16-row MFMA GEMM out of LDS that both are made of.
#include <algorithm>

#include "hip/tree_dev.h"
#include "hip/tree_plan.h"

namespace euler_hip {

// ----------------------------------------------------------------------------
// tr_head: kTrHeadRows roots per block, 16 waves; wave w owns 16-column slabs w, w+16, ...
// ----------------------------------------------------------------------------
constexpr int HB = kTrHeadRows;
constexpr int HFM = HB / 16;
constexpr int HNW = 16;
constexpr int TR_KC = 8;  // k steps (x32) per B chunk

// Head LDS tiles: rows padded by 16 bf16 (stride = 2 mod 4 16-B slots), so every
// ds_read_b128 lane group of an MFMA A-fragment read (rows 0-15 of two k-quarters:
// {0-3,12-15,20-27}, ...) lands on 16 distinct bank slots (2r + kq mod 16); the old
// +8 padding (stride 1 mod 16) put two lanes of every group on one slot.  Per-lane
// addresses stay base + constant, so the k loop folds them into the load offsets.
__device__ __forceinline__ int sw_off(int r, int col, int ld) { return r * ld + col; }

__device__ __forceinline__ void tr_prefetch(const bf16_t* __restrict__ Bf, int col0, int N, int K, int lane,
                                            uint4_t (&b)[TR_KC]) {
  const int c = col0 < N ? col0 : 0;  // branch-free: out-of-range fragments are loaded but unused
#pragma unroll
  for (int s = 0; s < TR_KC; ++s) b[s] = fm_frag(Bf, c, s * 32 < K ? s * 32 : 0, K, lane);
}

__device__ __forceinline__ void tr_mfma_chunk(const bf16_t* A, int lda, int kc, int K, const uint4_t (&b)[TR_KC],
                                              float4_t (&acc)[HFM][1], int lane) {
  const int lr = lane & 15, lk = (lane >> 4) * 8;
#pragma unroll
  for (int s = 0; s < TR_KC; ++s) {
    if (kc + s * 32 < K) {
      uint4_t av[HFM];
#pragma unroll
      for (int m = 0; m < HFM; ++m) av[m] = *reinterpret_cast<const uint4_t*>(A + sw_off(m * 16 + lr, kc + s * 32 + lk, lda));
#pragma unroll
      for (int m = 0; m < HFM; ++m) acc[m][0] = mfma16(av[m], b[s], acc[m][0]);
    }
  }
}

// acc += A_lds[rows][0:K] @ Bf[col0 .. col0+15][0:K]^T; the first chunk was prefetched
__device__ __forceinline__ void tr_gemm(const bf16_t* A, int lda, const bf16_t* __restrict__ Bf, int col0, int K,
                                        float4_t (&acc)[HFM][1], int lane, const uint4_t (&pre)[TR_KC]) {
  tr_mfma_chunk(A, lda, 0, K, pre, acc, lane);
  for (int kc = 32 * TR_KC; kc < K; kc += 32 * TR_KC) {
    uint4_t b[TR_KC];
#pragma unroll
    for (int s = 0; s < TR_KC; ++s) b[s] = fm_frag(Bf, col0, kc + s * 32 < K ? kc + s * 32 : 0, K, lane);
    tr_mfma_chunk(A, lda, kc, K, b, acc, lane);
  }
}

// tile rows -> kt layout: item = (column pair, 8-row chunk), column pairs fastest (4-byte
// LDS reads over consecutive banks), two 16-byte kt chunks per item
__device__ __forceinline__ void tr_lds_to_kt(const bf16_t* tile, int ld, int N, int64_t r0, bf16_t* kt) {
  const int np = N >> 1;
  for (int it = threadIdx.x; it < np * (HB / 8); it += HNW * 64) {
    const int q = it / np, n = (it - q * np) * 2;
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = *reinterpret_cast<const uint32_t*>(tile + sw_off(q * 8 + i, n, ld));
    uint4_t lo, hi;
    kt_pack8(w, lo, hi);
    *reinterpret_cast<uint4_t*>(kt + kt_off(r0 + q * 8, n, N)) = lo;
    *reinterpret_cast<uint4_t*>(kt + kt_off(r0 + q * 8, n + 1, N)) = hi;
  }
}

__device__ __forceinline__ int tr_head_ld(int w) { return w + 16; }  // see sw_off

// Phases (a barrier between each; every wave takes tile jobs j = wave, wave + 16, ...):
//   P0  h = relu(A W^T)                                  [A tile + A_kt, h_kt]
//   P1  logits = h Wc^T + bc -> loss, F1 counts, dlogits   (C/16 jobs, critical path)
//       emb = h Wfc^T + bfc -> emb_kt                      (fills the idle waves)
//   P2  g = (dlogits Wc) * relu'(h) -> g_kt                (H/16 jobs, critical path)
//       demb = dlogits Wout -> demb_kt, fc-bias partials   (E/16 jobs)
//       remaining emb jobs
//   P3  dA = g W (fp32 rows for the layer below)
// fc and out_fc enter the critical path only through Wc = Wout Wfc (TrCombArgs): the
// reference model has no nonlinearity between them, so logits and their gradient to h are
// the same products with two dependent GEMM phases fewer.
//
// LOSS == kTrLossSoftmax (tr_head_kernel<1>) splits the logits epilogue of P1 in two around
// one more barrier, since a row's statistics span the C / 16 <= 16 waves that hold its tiles:
//   P1a each logits wave keeps x = logits + bc of its tile in registers and reduces it over the
//       16 column lanes to per-row (max, sum exp(x - max), arg-max column; dense labels: label
//       sum, label arg-max) -> sm_s[row][tile]; padded columns enter none of them
//   P1b every logits wave merges the tiles of its rows in tile order (fixed order, no atomics:
//       the same bits in every launch) and finishes its own tile: p = exp(x - m) / Z,
//       d = bf16((s p - y) / B), row loss = sum_c y_c (m + log Z - x_c); wave 0 counts the rows
//       whose arg-max (ties: lowest column) is the label's: tp = correct, fp = fn = wrong
// The emb waves only pass the barrier.  One logits job per wave: C <= kTrSoftmaxMaxC.
constexpr int kSmStats = 6;  // per (row, tile): max, sum, arg-max, label sum, label max, label arg-max

// (max, its lowest column) and the sum over the 16 column lanes of a tile row; every lane ends
// with the same bits (the butterfly adds the same pairs in every lane)
__device__ __forceinline__ void sm_argmax16(float& m, int& am) {
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
__device__ __forceinline__ float sm_sum16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the softmax head's [HB][HNW][kSmStats] row statistics; no LDS in the sigmoid instantiation
template <int LOSS>
__device__ __forceinline__ float* sm_stats() {
  if constexpr (LOSS == kTrLossSoftmax) {
    __shared__ float sm_s[HB * HNW * kSmStats];
    return sm_s;
  } else {
    return nullptr;
  }
}

template <int LOSS>
__global__ __launch_bounds__(HNW * 64) void tr_head_kernel(TrHeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  const int nhb = static_cast<int>(gridDim.x) - a.nsample;
  if (static_cast<int>(blockIdx.x) >= nhb) {  // the next step's sampler on the CUs the head leaves idle
    tr_sample_block<HNW * 64>(a.smp, blockIdx.x - nhb, reinterpret_cast<int32_t*>(lds));
    return;
  }
  const uint32_t blk = blockIdx.x;
  TR_STAMP(a.prof, blk, 0);
  const int Hin2 = a.Hin2, H = a.H, E = a.E, C = a.C;
  const int lda = tr_head_ld(Hin2), ldh = tr_head_ld(H), ldc = tr_head_ld(C);
  bf16_t* Aa = lds;            // [HB][lda]  A rows
  bf16_t* Ah = Aa + HB * lda;  // [HB][ldh]  h (post-ReLU)
  bf16_t* Gb = Ah + HB * ldh;  // [HB][ldh]  g
  bf16_t* Dl = Gb + HB * ldh;  // [HB][ldc]  dlogits
  bf16_t* Ly = Dl + HB * ldc;  // [HB][C]    dense labels (label_mode 2)
  __shared__ int lab_s[HB];
  __shared__ float red_s[HNW][4];
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * HB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lg = lane >> 4;
  constexpr int NT = HNW * 64;

  if (a.label_mode < 2) {
    if (threadIdx.x < HB) {
      const int32_t root = a.roots[r0 + threadIdx.x];
      lab_s[threadIdx.x] = a.label_mode == 0 ? static_cast<int>(static_cast<const int16_t*>(a.labels)[root])
                                             : static_cast<const int32_t*>(a.labels)[root];
    }
  } else {
    const bf16_t* L = static_cast<const bf16_t*>(a.labels);
    const int cpl = C >> 3;
    for (int it = threadIdx.x; it < HB * cpl; it += NT) {
      const int r = it / cpl, c = it - r * cpl;
      const int64_t root = a.roots[r0 + r];
      *reinterpret_cast<uint4_t*>(Ly + r * C + c * 8) = *reinterpret_cast<const uint4_t*>(L + root * C + c * 8);
    }
  }
  // job lists of P1 / P2: (B operand, its K, output column)
  const int nl = C >> 4, ne = E >> 4, nh = H >> 4;
  const int ne1 = (HNW - nl) > 0 ? ((HNW - nl) < ne ? (HNW - nl) : ne) : 0;  // emb jobs beside the logits
  const int n1 = nl + ne1, n2 = nh + ne + (ne - ne1);
  auto job1 = [&](int j, const bf16_t*& Bf, int& cc) {
    if (j < nl) {
      Bf = a.Wc;
      cc = j * 16;
    } else {
      Bf = a.Wfc;
      cc = (j - nl) * 16;
    }
  };
  auto job2 = [&](int j, const bf16_t*& Bf, int& cc, int& K) {
    if (j < nh) {
      Bf = a.WcT;
      cc = j * 16;
      K = C;
    } else if (j < nh + ne) {
      Bf = a.WoutT;
      cc = (j - nh) * 16;
      K = C;
    } else {
      Bf = a.Wfc;
      cc = (ne1 + j - nh - ne) * 16;
      K = H;
    }
  };

  // P0: A tile -> LDS (+ A_kt); h = relu(A @ W^T)
  uint4_t pre[TR_KC];
  tr_prefetch(a.W, wave * 16, H, Hin2, lane, pre);
  const int cpa = Hin2 >> 3;
  for (int it = threadIdx.x; it < HB * cpa; it += NT) {
    const int r = it / cpa, c = it - r * cpa;
    *reinterpret_cast<uint4_t*>(Aa + sw_off(r, c * 8, lda)) =
        *reinterpret_cast<const uint4_t*>(a.A + (r0 + r) * Hin2 + c * 8);
  }
  __syncthreads();
  TR_STAMP(a.prof, blk, 1);
  tr_lds_to_kt(Aa, lda, Hin2, r0, a.A_kt);
  for (int cc = wave * 16; cc < H; cc += HNW * 16) {
    float4_t acc[HFM][1];
    tl_zero(acc);
    tr_gemm(Aa, lda, a.W, cc, Hin2, acc, lane, pre);
    if (cc + HNW * 16 < H) tr_prefetch(a.W, cc + HNW * 16, H, Hin2, lane, pre);
#pragma unroll
    for (int m = 0; m < HFM; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) Ah[sw_off(m * 16 + lg * 4 + j, cc + lr, ldh)] = f2bf(fmaxf(acc[m][0][j], 0.f));
  }
  if (wave < n1) {
    const bf16_t* Bf;
    int cc;
    job1(wave, Bf, cc);
    tr_prefetch(Bf, cc, 1 << 30, H, lane, pre);
  }
  __syncthreads();
  TR_STAMP(a.prof, blk, 2);
  tr_lds_to_kt(Ah, ldh, H, r0, a.h_kt);

  // P1: logits (+ loss, dlogits, F1 counts; padded label columns excluded) and emb
  float lsum = 0.f;
  int tp = 0, fp = 0, fn = 0;
  float sx[4], sy[4];  // softmax: the wave's logits tile and its label tile across the row merge
  float* const sm_s = sm_stats<LOSS>();
  for (int j = wave; j < n1; j += HNW) {
    const bf16_t* Bf;
    int cc;
    job1(j, Bf, cc);
    float4_t acc[HFM][1];
    tl_zero(acc);
    tr_gemm(Ah, ldh, Bf, cc, H, acc, lane, pre);
    const int col = cc + lr;
    if (j < nl) {
      const bool valid = col < a.C_real;
      const float bias = a.bc[col];
      if constexpr (LOSS == kTrLossSoftmax) {  // P1a (j == wave: n1 <= HNW)
        static_assert(HFM == 1, "the softmax head keeps one 16-row tile per wave");
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int row = lg * 4 + jj;
          sx[jj] = acc[0][0][jj] + bias;
          sy[jj] = a.label_mode < 2 ? ((lab_s[row] == col) ? 1.f : 0.f) : bf2f(Ly[row * C + col]);
          float mx = valid ? sx[jj] : -INFINITY;
          int am = col;
          sm_argmax16(mx, am);
          const float z = sm_sum16(valid ? __expf(sx[jj] - mx) : 0.f);
          float* st = sm_s + (row * HNW + j) * kSmStats;
          if (a.label_mode == 2) {
            const float ys = sm_sum16(valid ? sy[jj] : 0.f);
            float ym = valid ? sy[jj] : -INFINITY;
            int ya = col;
            sm_argmax16(ym, ya);
            if (lr == 0) {
              st[3] = ys;
              st[4] = ym;
              st[5] = __int_as_float(ya);
            }
          }
          if (lr == 0) {
            st[0] = mx;
            st[1] = z;
            st[2] = __int_as_float(am);
          }
        }
      } else {
#pragma unroll
        for (int m = 0; m < HFM; ++m) {
          float d[4];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int row = m * 16 + lg * 4 + jj;
            const float xv = acc[m][0][jj] + bias;
            const float y = a.label_mode < 2 ? ((lab_s[row] == col) ? 1.f : 0.f) : bf2f(Ly[row * C + col]);
            const float p = 1.f / (1.f + __expf(-xv));
            if (valid) {
              lsum += fmaxf(xv, 0.f) - xv * y + log1pf(__expf(-fabsf(xv)));
              const bool pred = xv >= 0.f, pos = y > 0.5f;
              tp += pred && pos;
              fp += pred && !pos;
              fn += !pred && pos;
            }
            d[jj] = valid ? bf2f(f2bf((p - y) * a.inv_scale)) : 0.f;
            Dl[sw_off(row, col, ldc)] = f2bf(d[jj]);
          }
          kt_store4(a.dlog_kt, r0 + m * 16 + lg * 4, col, C, d[0], d[1], d[2], d[3]);
        }
      }
    } else {
      const float b = a.bfc[col];
#pragma unroll
      for (int m = 0; m < HFM; ++m)
        kt_store4(a.emb_kt, r0 + m * 16 + lg * 4, col, E, acc[m][0][0] + b, acc[m][0][1] + b, acc[m][0][2] + b,
                  acc[m][0][3] + b);
    }
    if (j + HNW < n1) {  // (after the epilogue: the loss math keeps no prefetch registers live)
      const bf16_t* Bn;
      int cn;
      job1(j + HNW, Bn, cn);
      tr_prefetch(Bn, cn, 1 << 30, H, lane, pre);
    }
  }
  if constexpr (LOSS == kTrLossSoftmax) {  // P1b
    __syncthreads();
    if (wave < nl) {
      const int col = wave * 16 + lr, nlr = (a.C_real + 15) >> 4;  // tiles with a real column
      const bool valid = col < a.C_real;
      float d[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int row = lg * 4 + jj;
        const float* st = sm_s + row * HNW * kSmStats;
        float mx = st[0], ys = 1.f, ym = -INFINITY;
        int am = __float_as_int(st[2]), lab = 0;
        for (int t = 1; t < nlr; ++t)
          if (st[t * kSmStats] > mx) {  // ties stay with the lower tile
            mx = st[t * kSmStats];
            am = __float_as_int(st[t * kSmStats + 2]);
          }
        float Z = 0.f;
        for (int t = 0; t < nlr; ++t) Z += st[t * kSmStats + 1] * __expf(st[t * kSmStats] - mx);
        if (a.label_mode < 2) {
          lab = lab_s[row];
        } else {
          ys = 0.f;
          for (int t = 0; t < nlr; ++t) {
            ys += st[t * kSmStats + 3];
            if (st[t * kSmStats + 4] > ym) {
              ym = st[t * kSmStats + 4];
              lab = __float_as_int(st[t * kSmStats + 5]);
            }
          }
        }
        const float lse = mx + logf(Z);
        const float p = valid ? __expf(sx[jj] - mx) / Z : 0.f;
        if (valid) lsum += sy[jj] * (lse - sx[jj]);
        d[jj] = valid ? bf2f(f2bf((ys * p - sy[jj]) * a.inv_scale)) : 0.f;
        Dl[sw_off(row, col, ldc)] = f2bf(d[jj]);
        if (wave == 0 && lr == 0) {
          const bool ok = am == lab;
          tp += ok;
          fp += !ok;
          fn += !ok;
        }
      }
      kt_store4(a.dlog_kt, r0 + lg * 4, col, C, d[0], d[1], d[2], d[3]);
    }
  }
  {
    lsum = wave_sum(lsum);
    tp = wave_sum_i(tp);
    fp = wave_sum_i(fp);
    fn = wave_sum_i(fn);
    if (lane == 0) {
      red_s[wave][0] = lsum;
      red_s[wave][1] = static_cast<float>(tp);
      red_s[wave][2] = static_cast<float>(fp);
      red_s[wave][3] = static_cast<float>(fn);
    }
  }
  if (wave < n2) {
    const bf16_t* Bf;
    int cc, K;
    job2(wave, Bf, cc, K);
    tr_prefetch(Bf, cc, 1 << 30, K, lane, pre);
  }
  __syncthreads();
  TR_STAMP(a.prof, blk, 3);
  if (threadIdx.x < 4) {  // per-block sums, plain stores (no contended atomics)
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < HNW; ++w) v += red_s[w][threadIdx.x];
    a.head_part[blockIdx.x * 4 + threadIdx.x] = threadIdx.x == 0 ? v * a.inv_scale : v;
  }

  // P2: g = (dlogits Wc) * relu'(h); demb = dlogits Wout (+ fc-bias column sums); emb rest
  for (int j = wave; j < n2; j += HNW) {
    const bf16_t* Bf;
    int cc, K;
    job2(j, Bf, cc, K);
    float4_t acc[HFM][1];
    tl_zero(acc);
    tr_gemm(j < nh + ne ? Dl : Ah, j < nh + ne ? ldc : ldh, Bf, cc, K, acc, lane, pre);
    const int col = cc + lr;
    if (j < nh) {
#pragma unroll
      for (int m = 0; m < HFM; ++m) {
        float e[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int row = m * 16 + lg * 4 + jj;
          e[jj] = bf2f(f2bf(bf_pos(Ah[sw_off(row, col, ldh)]) ? acc[m][0][jj] : 0.f));
          Gb[sw_off(row, col, ldh)] = f2bf(e[jj]);
        }
        kt_store4(a.g_kt, r0 + m * 16 + lg * 4, col, H, e[0], e[1], e[2], e[3]);
      }
    } else if (j < nh + ne) {
      float cs = 0.f;
#pragma unroll
      for (int m = 0; m < HFM; ++m) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) cs += acc[m][0][jj];
        kt_store4(a.demb_kt, r0 + m * 16 + lg * 4, col, E, acc[m][0][0], acc[m][0][1], acc[m][0][2], acc[m][0][3]);
      }
      cs += __shfl_xor(cs, 16, 64);
      cs += __shfl_xor(cs, 32, 64);
      if (lg == 0) a.dbfc_part[static_cast<int64_t>(blockIdx.x) * E + col] = cs;
    } else {
      const float b = a.bfc[col];
#pragma unroll
      for (int m = 0; m < HFM; ++m)
        kt_store4(a.emb_kt, r0 + m * 16 + lg * 4, col, E, acc[m][0][0] + b, acc[m][0][1] + b, acc[m][0][2] + b,
                  acc[m][0][3] + b);
    }
    if (j + HNW < n2) {
      const bf16_t* Bn;
      int cn, Kn;
      job2(j + HNW, Bn, cn, Kn);
      tr_prefetch(Bn, cn, 1 << 30, Kn, lane, pre);
    }
  }
  if (a.dA) tr_prefetch(a.WT, wave * 16, Hin2, H, lane, pre);
  __syncthreads();
  TR_STAMP(a.prof, blk, 4);

  // P3: dA = g @ W (fp32 rows) for the layer below
  if (a.dA) {
    for (int cc = wave * 16; cc < Hin2; cc += HNW * 16) {
      float4_t acc[HFM][1];
      tl_zero(acc);
      tr_gemm(Gb, ldh, a.WT, cc, H, acc, lane, pre);
      if (cc + HNW * 16 < Hin2) tr_prefetch(a.WT, cc + HNW * 16, Hin2, H, lane, pre);
#pragma unroll
      for (int m = 0; m < HFM; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) a.dA[(r0 + m * 16 + lg * 4 + j) * Hin2 + cc + lr] = acc[m][0][j];
    }
  }
  TR_STAMP(a.prof, blk, 5);
}

// one kernel per loss: tr_head_kernel<kTrLossSigmoid> carries nothing of the softmax epilogue
// (its code is the untemplated kernel's, instruction for instruction: tools/kernel_isa.py)
template __global__ void tr_head_kernel<kTrLossSigmoid>(TrHeadArgs);
template __global__ void tr_head_kernel<kTrLossSoftmax>(TrHeadArgs);

// ----------------------------------------------------------------------------
// tr_pair_head: the head of the unsupervised GraphSAGE step (see TrPairHeadArgs; reference
// examples/graphsage/graphsage.py:70-98, tf_euler/python/mp_utils/base.py:49-91).  Block b:
// sources 16b..16b+15 and their context rows, 2 + K row tiles of 16 in LDS (tile 0: the
// sources, tile 1: their positives, tiles 2..: their negatives, source-major), 16 waves;
// every phase deals its (tile, 16-column slab) jobs round-robin over the waves, each one
// tr_gemm (A rows from LDS, the tile's tower's B fragments from L2):
//   P1 h1 = relu(A1 W1^T)                   -> H   (+ A1_kt, h_kt for the dW GEMMs)
//   P2 e  = h1 Wfc^T + bfc                  -> Ef  (fp32, over the dead A1 tile)
//   P3 wave i = source i: logits <e_i, e_ctx>, softplus CE, reciprocal rank, de (fp32)
//                                           -> D (bf16, + de_kt), bias / loss partials
//   P4 g  = (de Wfc) * relu'(h1)            -> G   (over the dead Ef) (+ g_kt)
//   P5 dA1 = g W1                           (fp32 rows: the routed layer-0 dW reads them)
// ----------------------------------------------------------------------------
__device__ __forceinline__ const TrPairTower& pr_tower(const TrPairHeadArgs& a, int t) { return t == 0 ? a.s : a.c; }

// first row of tile t in its tower
__device__ __forceinline__ int64_t pr_row0(const TrPairHeadArgs& a, int b, int t) {
  if (t <= 1) return static_cast<int64_t>(b) * 16;
  return static_cast<int64_t>(a.B) + static_cast<int64_t>(b) * 16 * a.K + 16 * (t - 2);
}

__global__ __launch_bounds__(HNW * 64) void tr_pair_head_kernel(TrPairHeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  const int b = blockIdx.x;
  const int NTILE = 2 + a.K, rows = 16 * NTILE;
  const int H0x2 = a.H0x2, H1 = a.H1, E = a.E;
  const int lda = tr_head_ld(H0x2), ldh = tr_head_ld(H1), lde = tr_head_ld(E);
  const int abytes = rows * lda * 2, ebytes = rows * E * 4, gbytes = rows * ldh * 2;
  const int region = ((abytes > ebytes ? abytes : ebytes) > gbytes ? (abytes > ebytes ? abytes : ebytes) : gbytes);
  bf16_t* Aa = lds;                                                   // P1 input
  float* Ef = reinterpret_cast<float*>(lds);                          // P2 -> P3 (over Aa)
  bf16_t* Gg = lds;                                                   // P4 -> P5 (over Ef)
  bf16_t* Hh = lds + region / 2;                                      // h1
  bf16_t* Dd = Hh + rows * ldh;                                       // de
  float* ps = reinterpret_cast<float*>(Dd + rows * lde);              // [2][16][E] bias partials
  __shared__ float red_s[HNW][2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lg = lane >> 4;
  constexpr int NT = HNW * 64;

  // A1 rows of every tile -> LDS (+ the kt copies for dW1)
  const int cpa = H0x2 >> 3;
  for (int it = threadIdx.x; it < rows * cpa; it += NT) {
    const int r = it / cpa, c = it - r * cpa;
    const int t = r >> 4;
    const TrPairTower& tw = pr_tower(a, t);
    *reinterpret_cast<uint4_t*>(Aa + sw_off(r, c * 8, lda)) =
        *reinterpret_cast<const uint4_t*>(tw.A1 + (pr_row0(a, b, t) + (r & 15)) * H0x2 + c * 8);
  }
  __syncthreads();
  for (int t = 0; t < NTILE; ++t) tr_lds_to_kt(Aa + 16 * t * lda, lda, H0x2, pr_row0(a, b, t), pr_tower(a, t).A1_kt);

  uint4_t pre[TR_KC];
  // P1: h1 = relu(A1 W1^T)
  {
    const int nc = H1 >> 4, nj = NTILE * nc;
    if (wave < nj) tr_prefetch(pr_tower(a, wave / nc).W1, (wave % nc) * 16, H1, H0x2, lane, pre);
    for (int j = wave; j < nj; j += HNW) {
      const int t = j / nc, cs = (j - t * nc) * 16;
      float4_t acc[HFM][1];
      tl_zero(acc);
      tr_gemm(Aa + 16 * t * lda, lda, pr_tower(a, t).W1, cs, H0x2, acc, lane, pre);
      if (j + HNW < nj) tr_prefetch(pr_tower(a, (j + HNW) / nc).W1, ((j + HNW) % nc) * 16, H1, H0x2, lane, pre);
      float v[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        v[jj] = fmaxf(acc[0][0][jj], 0.f);
        Hh[sw_off(16 * t + lg * 4 + jj, cs + lr, ldh)] = f2bf(v[jj]);
      }
      kt_store4(pr_tower(a, t).h_kt, pr_row0(a, b, t) + lg * 4, cs + lr, H1, bf2f(f2bf(v[0])), bf2f(f2bf(v[1])),
                bf2f(f2bf(v[2])), bf2f(f2bf(v[3])));
    }
  }
  __syncthreads();  // A1 dead from here (Ef takes its place)
  // P2: e = h1 Wfc^T + bfc (fp32)
  {
    const int nc = E >> 4, nj = NTILE * nc;
    if (wave < nj) tr_prefetch(pr_tower(a, wave / nc).Wfc, (wave % nc) * 16, E, H1, lane, pre);
    for (int j = wave; j < nj; j += HNW) {
      const int t = j / nc, cs = (j - t * nc) * 16;
      float4_t acc[HFM][1];
      tl_zero(acc);
      tr_gemm(Hh + 16 * t * ldh, ldh, pr_tower(a, t).Wfc, cs, H1, acc, lane, pre);
      if (j + HNW < nj) tr_prefetch(pr_tower(a, (j + HNW) / nc).Wfc, ((j + HNW) % nc) * 16, E, H1, lane, pre);
      const float bias = pr_tower(a, t).bfc[cs + lr];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) Ef[(16 * t + lg * 4 + jj) * E + cs + lr] = acc[0][0][jj] + bias;
    }
  }
  __syncthreads();
  // P3: wave i = source i of the block
  {
    // logits / gradients of the 1 + K <= 16 pairs in registers (fully unrolled: constant
    // indices, no scratch)
    const int i = wave;
    const int K = a.K;
    float l[16], g[16];
    const float* es = Ef + i * E;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      l[k] = 0.f;
      if (k > K) continue;
      const int row = k == 0 ? 16 + i : 32 + i * K + (k - 1);
      float d = 0.f;
      for (int c = lane; c < E; c += 64) d += es[c] * Ef[row * E + c];
      l[k] = wave_sum(d);
    }
    float loss = 0.f, gsum = 0.f;
    int beat = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      g[k] = 0.f;
      if (k > K) continue;
      const float x = l[k];
      loss += fmaxf(x, 0.f) + log1pf(__expf(-fabsf(x))) - (k == 0 ? x : 0.f);
      g[k] = (1.f / (1.f + __expf(-x)) - (k == 0 ? 1.f : 0.f)) * a.inv_n;
      gsum += g[k];
      if (k > 0 && x >= l[0]) ++beat;
    }
    if (lane == 0) {
      red_s[i][0] = loss * a.inv_n;
      red_s[i][1] = 1.f / static_cast<float>(1 + beat);
    }
    for (int c = lane; c < E; c += 64) {
      const float ev = es[c];
      float de = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if (k > K) continue;
        const int row = k == 0 ? 16 + i : 32 + i * K + (k - 1);
        de += g[k] * Ef[row * E + c];
        Dd[sw_off(row, c, lde)] = f2bf(g[k] * ev);
      }
      Dd[sw_off(i, c, lde)] = f2bf(de);
      ps[i * E + c] = de;                 // source-tower bias gradient share
      ps[(16 + i) * E + c] = gsum * ev;   // context-tower share: sum_k g_k e_i
    }
  }
  __syncthreads();  // Ef dead from here (G takes its place)
  for (int t = 0; t < NTILE; ++t) tr_lds_to_kt(Dd + 16 * t * lde, lde, E, pr_row0(a, b, t), pr_tower(a, t).de_kt);
  for (int c = threadIdx.x; c < 2 * E; c += NT) {  // per-block bias partials, fixed order
    const int tw = c >= E, col = c - tw * E;
    float v = 0.f;
    for (int w = 0; w < 16; ++w) v += ps[(tw * 16 + w) * E + col];
    (tw ? a.c : a.s).dbfc_part[static_cast<int64_t>(b) * E + col] = v;
  }
  if (threadIdx.x < 4) {
    float v = 0.f;
    if (threadIdx.x < 2)
      for (int w = 0; w < 16; ++w) v += red_s[w][threadIdx.x];
    a.head_part[b * 4 + threadIdx.x] = v;
  }
  // P4: g = (de Wfc) * relu'(h1)
  {
    const int nc = H1 >> 4, nj = NTILE * nc;
    if (wave < nj) tr_prefetch(pr_tower(a, wave / nc).WfcT, (wave % nc) * 16, H1, E, lane, pre);
    for (int j = wave; j < nj; j += HNW) {
      const int t = j / nc, cs = (j - t * nc) * 16;
      float4_t acc[HFM][1];
      tl_zero(acc);
      tr_gemm(Dd + 16 * t * lde, lde, pr_tower(a, t).WfcT, cs, E, acc, lane, pre);
      if (j + HNW < nj) tr_prefetch(pr_tower(a, (j + HNW) / nc).WfcT, ((j + HNW) % nc) * 16, H1, E, lane, pre);
      float v[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int row = 16 * t + lg * 4 + jj;
        v[jj] = bf2f(f2bf(bf_pos(Hh[sw_off(row, cs + lr, ldh)]) ? acc[0][0][jj] : 0.f));
        Gg[sw_off(row, cs + lr, ldh)] = f2bf(v[jj]);
      }
      kt_store4(pr_tower(a, t).g_kt, pr_row0(a, b, t) + lg * 4, cs + lr, H1, v[0], v[1], v[2], v[3]);
    }
  }
  __syncthreads();
  // P5: dA1 = g W1 (fp32 rows)
  {
    const int nc = H0x2 >> 4, nj = NTILE * nc;
    if (wave < nj) tr_prefetch(pr_tower(a, wave / nc).W1T, (wave % nc) * 16, H0x2, H1, lane, pre);
    for (int j = wave; j < nj; j += HNW) {
      const int t = j / nc, cs = (j - t * nc) * 16;
      float4_t acc[HFM][1];
      tl_zero(acc);
      tr_gemm(Gg + 16 * t * ldh, ldh, pr_tower(a, t).W1T, cs, H1, acc, lane, pre);
      if (j + HNW < nj) tr_prefetch(pr_tower(a, (j + HNW) / nc).W1T, ((j + HNW) % nc) * 16, H0x2, H1, lane, pre);
      float* out = pr_tower(a, t).dA1;
      const int64_t r0 = pr_row0(a, b, t);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) out[(r0 + lg * 4 + jj) * H0x2 + cs + lr] = acc[0][0][jj];
    }
  }
}

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

size_t eh_tr_head_lds(int Hin2, int H, int E, int C, int label_mode) {
  (void)E;
  size_t el = static_cast<size_t>(HB) * ((Hin2 + 16) + 2 * (H + 16) + (C + 16));
  if (label_mode == 2) el += static_cast<size_t>(HB) * C;
  return el * sizeof(bf16_t);
}

// static LDS the softmax head adds to eh_tr_head_lds: its row statistics (sm_stats)
size_t eh_tr_head_softmax_lds() { return static_cast<size_t>(HB) * HNW * kSmStats * sizeof(float); }

hipError_t eh_tr_head(const TrHeadArgs* a, int64_t B, hipStream_t s) {
  if (!a->A || !a->W || !a->Wfc || !a->WfcT || !a->Wout || !a->WoutT || !a->Wc || !a->WcT || !a->bc || !a->bfc ||
      !a->roots || !a->labels ||
      !a->A_kt || !a->h_kt || !a->emb_kt || !a->dlog_kt || !a->demb_kt || !a->g_kt || !a->dbfc_part || !a->head_part ||
      (a->dA && !a->WT))
    return hipErrorInvalidValue;
  if (B % 32 != 0 || a->H % 16 != 0 || a->E % 32 != 0 || a->C % 32 != 0 || a->Hin2 % 32 != 0 ||
      a->C_real > a->C || a->C_real <= 0)
    return hipErrorInvalidValue;
  if (a->label_mode < 0 || a->label_mode > 2 || (a->loss != kTrLossSigmoid && a->loss != kTrLossSoftmax))
    return hipErrorInvalidValue;
  const bool softmax = a->loss == kTrLossSoftmax;
  // softmax: one logits tile per wave (the tile stays in registers across the row merge)
  if (softmax && a->C > kTrSoftmaxMaxC) return hipErrorInvalidValue;
  const size_t lds = eh_tr_head_lds(a->Hin2, a->H, a->E, a->C, a->label_mode);
  if (lds + (softmax ? eh_tr_head_softmax_lds() : 0) > 160 * 1024 - 64) return hipErrorInvalidValue;
  const void* fn = softmax ? reinterpret_cast<const void*>(tr_head_kernel<kTrLossSoftmax>)
                           : reinterpret_cast<const void*>(tr_head_kernel<kTrLossSigmoid>);
  EULER_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  // the sampler refills its own roots array, not the one this launch reads
  if (a->nsample > 0 && (!tr_sample_ok(a->smp, kTrHeadSampleRows, a->nsample) || a->smp.roots == a->roots))
    return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>(B / HB + a->nsample));
  if (softmax)
    hipLaunchKernelGGL(tr_head_kernel<kTrLossSoftmax>, grid, dim3(HNW * 64), lds, s, *a);
  else
    hipLaunchKernelGGL(tr_head_kernel<kTrLossSigmoid>, grid, dim3(HNW * 64), lds, s, *a);
  return hipGetLastError();
}

size_t eh_tr_pair_head_lds(int K, int H0x2, int H1, int E) {
  const size_t rows = 16 * static_cast<size_t>(2 + K);
  const size_t abytes = rows * (H0x2 + 16) * 2, ebytes = rows * E * 4, gbytes = rows * (H1 + 16) * 2;
  const size_t region = std::max(std::max(abytes, ebytes), gbytes);
  return region + rows * (H1 + 16) * 2 + rows * (E + 16) * 2 + 2 * 16 * static_cast<size_t>(E) * 4;
}

hipError_t eh_tr_pair_head(const TrPairHeadArgs* a, hipStream_t s) {
  if (a->B <= 0 || a->B % 16 != 0 || a->K < 1 || a->K > 15 || a->H0x2 % 32 != 0 || a->H1 % 32 != 0 ||
      a->E % 32 != 0 || a->E > 1024)
    return hipErrorInvalidValue;
  const TrPairTower* tw[2] = {&a->s, &a->c};
  for (const TrPairTower* t : tw)
    if (!t->A1 || !t->W1 || !t->W1T || !t->Wfc || !t->WfcT || !t->bfc || !t->A1_kt || !t->h_kt || !t->de_kt ||
        !t->g_kt || !t->dA1 || !t->dbfc_part)
      return hipErrorInvalidValue;
  if (!a->head_part) return hipErrorInvalidValue;
  const size_t lds = eh_tr_pair_head_lds(a->K, a->H0x2, a->H1, a->E);
  if (lds > 160 * 1024 - 256) return hipErrorInvalidValue;
  EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(tr_pair_head_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  hipLaunchKernelGGL(tr_pair_head_kernel, dim3(static_cast<uint32_t>(a->B / 16)), dim3(HNW * 64), lds, s, *a);
  return hipGetLastError();
}

}  // extern "C"
