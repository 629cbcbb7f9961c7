// Fused GraphSAGE training step on gfx950 for 1-3 hop models (SURVEY §2.7 K1/K2/K3/K11/
// K12/K13, §7.3) — the kernels behind euler_amd.models.sage_trainer.SageTrainer, which
// NodeEstimator(device_graph=True) and bench.py run.
//
// Model (reference examples/graphsage/graphsage.py:56-67, mp_utils/base_gnn.py:75-92,
// mp_utils/base.py:24-47, convolution/sage_conv.py:33-44):
//   h_k   = relu([h_{k-1}[self] | mean_nbr h_{k-1}] @ W_k^T)     k = 0 .. L-1
//   emb   = h_{L-1} @ Wfc^T + bfc ;  logits = emb @ Wout^T
//   loss  = mean(sigmoid_ce(logits, label))
// Mini-batch = the reference SageDataFlow (sample every node of the previous hops again,
// sage_dataflow.py:35-50) without dedup, in the slotted tree layout of tree_args.h.
//
// A 2-hop step is four launches, one translation unit per kind of launch:
//   tr_fwd  (mode 0)  roots + hop 1 + hop 2 sampling (Philox, on the HBM CSR), gather of
//                     the leaf feature rows, mean, MFMA GEMM + ReLU, and the tree mean of
//                     the next layer as the epilogue -> A1 rows, A0 (kt), ReLU bits
//                                                                      (this file)
//   tr_head           last conv + fc + out_fc + loss + backward to dA1    (tree_head.hip)
//   tr_dw             grouped split-K dW of every weight; the outer layer's G operand is
//                     routed from dA1 through the tree inside the kernel (never stored)
//   tr_opt   (mode 2) split-K reduce + Adam/Adagrad/SGD/momentum + bf16 weight shadows
//                                                                      (both tree_dw.hip)
// (3 hops add one tr_fwd mode 2 and one tr_bwd; 1 hop uses tr_fwd mode 1).  Device code that
// more than one unit uses is in tree_dev.h.
//
// This unit: tr_sample_kernel, tr_fwd_kernel, tr_fwd2_kernel (with tr_comb_wave, the head's
// combined weight) and tr_bwd_kernel, the inner-layer backward of 3-hop models.
#include <cstdlib>

#include "hip/tree_dev.h"
#include "hip/tree_plan.h"

namespace euler_hip {

constexpr int kTrBN = 256;  // output columns per GEMM chunk (4 waves x 64)

// ----------------------------------------------------------------------------
// combination tiles, computed by wave 0 of the forward launch's tile blocks before their
// own work (the MFMA units are idle during the gather): Wc = Wout Wfc as 16 x 16 MFMA
// tiles of the bf16 fm shadows (an fm fragment of Wout [C][E] is also a valid A fragment:
// lane l holds row l & 15, k 8(l >> 4)..+7), all E/32 fragment pairs of a tile in
// flight; bc = Wout bfc in fp32 from the masters (one row per block).  No extra blocks:
// extra blocks would push tile blocks past the resident slots into a second round.
// ----------------------------------------------------------------------------
__device__ __forceinline__ void tr_comb_wave(const TrCombArgs& c, int first, int stride, int lane) {
  const int tcols = c.H >> 4, ntiles = (c.C >> 4) * tcols;
  for (int t = first; t < ntiles; t += stride) {
    const int c0 = (t / tcols) * 16, h0 = (t % tcols) * 16;
    float4_t acc = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < c.E; k0 += 128) {  // 4 fragment pairs in flight (register budget of the host kernel)
      uint4_t av[4], bv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = k0 + s * 32 < c.E ? k0 + s * 32 : 0;
        av[s] = fm_frag(c.wout_sh, c0, k, c.E, lane);
        bv[s] = fm_frag(c.wfcT_sh, h0, k, c.E, lane);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (k0 + s * 32 < c.E) acc = mfma16(av[s], bv[s], acc);
    }
    const int h = h0 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = c0 + (lane >> 4) * 4 + j;
      c.Wc[fm_off(r, h, c.H)] = f2bf(acc[j]);
      c.WcT[fm_off(h, r, c.C)] = f2bf(acc[j]);
    }
  }
  // bc = Wout bfc in fp32: one row per block (rows strided over the blocks like the tiles),
  // the wave's lanes split E and reduce by shuffles.  (One row per lane with a serial loop
  // over E made block 0 a 25 us straggler: 256 dependent-issue global loads per lane.)
  for (int r = first; r < c.C; r += stride) {
    const float* w = c.wout + static_cast<int64_t>(r) * c.E;
    float b = 0.f;
    for (int e = lane; e < c.E; e += 64) b += w[e] * c.bfc[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b += __shfl_xor(b, o, 64);
    if (lane == 0) c.bc[r] = b;
  }
}

__global__ __launch_bounds__(256) void tr_sample_kernel(TrSampleArgs a) {
  __shared__ int32_t node_s[kTrSampleRows];
  tr_sample_block<256>(a, blockIdx.x, node_s);
}

// ----------------------------------------------------------------------------
// tr_fwd: one SAGE layer over BM target rows per block (see TrFwdArgs)
// ----------------------------------------------------------------------------
#ifndef TR_FWD_WAVES
#define TR_FWD_WAVES 4
#endif
#ifndef TR_FWD_BPF
#define TR_FWD_BPF 2
#endif
template <typename FT, int BM, int MODE>
__global__ __launch_bounds__(256, (BM == 32 ? TR_FWD_WAVES : 2)) void tr_fwd_kernel(TrFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  constexpr bool kGather = MODE != 2;
  const int tb = static_cast<int>(blockIdx.x), ntb = static_cast<int>(gridDim.x);
  if (a.ncomb && threadIdx.x < 64) tr_comb_wave(a.comb, tb, ntb, threadIdx.x);  // the head's Wc
  const int D = a.D;
  const int K2 = 2 * D;
  const int ldsw = K2 + 8;
  const int tile = xcd_remap(tb, ntb);
  const int64_t row0 = static_cast<int64_t>(tile) * BM;
  const int H = a.H;
  const bool alias_out = H <= kTrBN && kTrBN <= K2;
  // LDS: [BM][ldsw] A tile | [BM][kTrBN + 8] output tile (modes 0/2, unless it aliases the
  // A tile) | node ids [BM] + leaf ids [BM][FL] (modes 0/1); must match eh_tr_fwd_lds
  const bool own_otile = MODE != 1 && !alias_out;
  bf16_t* otile = own_otile ? lds + BM * ldsw : lds;
  int32_t* node_s = reinterpret_cast<int32_t*>(lds + BM * ldsw + (own_otile ? BM * (kTrBN + 8) : 0));
  int32_t* leaf_s = node_s + BM;

  TR_STAMP(a.prof, tb, 0);
  constexpr int FN = 4;
  constexpr int kBP = TR_FWD_BPF;  // k-steps of weight fragments in flight
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const bf16_t* W = a.W;
  uint4_t bq[kBP][FN];
  if constexpr (kGather) {
    // ---- the sampled ids of the block (sampler output, one step ahead): coalesced
    if (tb == 0 && threadIdx.x == 0) {
      if (a.step) a.step[0] += 1;
      a.rng[1] += 1;  // this batch is consumed: the sampler draws the next counter
    }
    for (int i = tb * 256 + threadIdx.x; i < a.B; i += ntb * 256) a.roots_cur[i] = a.roots_in[i];
    if (threadIdx.x < BM) node_s[threadIdx.x] = row0 + threadIdx.x < a.M ? a.nodes[row0 + threadIdx.x] : -1;
    for (int it = threadIdx.x; it < BM * a.FL; it += 256)
      leaf_s[it] = row0 * a.FL + it < a.M * a.FL ? a.leaf[row0 * a.FL + it] : -1;
    __syncthreads();
    TR_STAMP(a.prof, tb, 1);
    // ---- gather + mean: item = (row, 8-column chunk); two items per thread with every
    // leaf load of both in flight
    const FT* x = static_cast<const FT*>(a.x);
    const int cpr = D >> 3;
    const int nitems = BM * cpr;
    constexpr int G = Feat8<FT>::kInFlight;
    for (int it = threadIdx.x; it < nitems; it += 512) {
      const int itb = it + 256;
      const bool hb = itb < nitems;
      const int ra = it / cpr, ca = it - ra * cpr;
      const int rb = hb ? itb / cpr : ra, cb = hb ? itb - rb * cpr : ca;
      const int32_t na = node_s[ra], nb = hb ? node_s[rb] : -1;
      // branch-free loads: a padding id (-1) reads row 0 and is zeroed at use, so no
      // divergent branch forces the compiler to wait on each load (vmcnt(0))
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
        // unconditional: slots past FL (ids -1) re-read the L2-resident row 0
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
        const uint4_t selfv = h ? sb.bf16() : sa.bf16(), meanv = pack_bf16x8(h ? acc_b : acc_a);
        const int64_t grow = row0 + r;
        if constexpr (MODE == 1) {
          if (grow < a.M) {
            *reinterpret_cast<uint4_t*>(a.a_next + grow * K2 + c * 8) = selfv;
            *reinterpret_cast<uint4_t*>(a.a_next + grow * K2 + D + c * 8) = meanv;
          }
        } else {
          *reinterpret_cast<uint4_t*>(lds + r * ldsw + c * 8) = selfv;
          *reinterpret_cast<uint4_t*>(lds + r * ldsw + D + c * 8) = meanv;
        }
      }
    }
    if constexpr (MODE == 1) return;
  } else {
    // ---- rows: BM rows of A [M][K2] (bf16) into the tile
    const bf16_t* A = static_cast<const bf16_t*>(a.x);
    const int cpr = K2 >> 3;
    for (int it = threadIdx.x; it < BM * cpr; it += 256) {
      const int r = it / cpr, c = it - r * cpr;
      const int64_t grow = row0 + r;
      const uint4_t v = grow < a.M ? *reinterpret_cast<const uint4_t*>(A + grow * K2 + c * 8) : uint4_t{0u, 0u, 0u, 0u};
      *reinterpret_cast<uint4_t*>(lds + r * ldsw + c * 8) = v;
    }
  }
  // the GEMM's first kBP k-steps of B fragments (weights: L2-resident) load behind the kt
  // pass; the loop below keeps kBP steps in flight (a weight-fragment load from L2 takes
  // longer than one step's MFMAs, so one step ahead leaves the chain latency-bound)
  if constexpr (MODE != 1) {
    if (wave * 64 < a.H) {
#pragma unroll
      for (int q = 0; q < kBP; ++q)
#pragma unroll
        for (int n = 0; n < FN; ++n) bq[q][n] = fm_frag(W, wave * 64 + n * 16, q * 32 < K2 ? q * 32 : 0, K2, lane);
    }
  }
  __syncthreads();
  TR_STAMP(a.prof, tb, 2);

  // ---- A tile -> kt layout (dW operand): item = (column pair, 8-row chunk q), column
  // pairs fastest so a wave's 4-byte LDS reads cover consecutive banks
  if (a.a_kt) {
    constexpr int CH = BM / 8;
    const int np = K2 >> 1;
    for (int it = threadIdx.x; it < np * CH; it += 256) {
      const int q = it / np;
      const int n = (it - q * np) * 2;
      const int64_t gr = row0 + q * 8;
      if (gr >= a.M) continue;
      uint32_t w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = *reinterpret_cast<const uint32_t*>(lds + (q * 8 + i) * ldsw + n);
      uint4_t lo, hi;
      kt_pack8(w, lo, hi);
      *reinterpret_cast<uint4_t*>(a.a_kt + kt_off(gr, n, K2)) = lo;
      *reinterpret_cast<uint4_t*>(a.a_kt + kt_off(gr, n + 1, K2)) = hi;
    }
  }

  TR_STAMP(a.prof, tb, 3);
  // ---- MFMA GEMM out of LDS; wave w owns 64-column slab w of each 256-column chunk
  constexpr int FM = BM / 16;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const int ldo = kTrBN + 8;
  for (int cchunk = 0; cchunk < H; cchunk += kTrBN) {
    const int cb = cchunk + wave * 64;
    float4_t acc[FM][FN];
    tl_zero(acc);
    if (cb < H) {
      if (cchunk > 0) {
#pragma unroll
        for (int q = 0; q < kBP; ++q)
#pragma unroll
          for (int n = 0; n < FN; ++n) bq[q][n] = fm_frag(W, cb + n * 16, q * 32 < K2 ? q * 32 : 0, K2, lane);
      }
      // kBP steps per iteration, ring slot q holds step k0 + 32 q; after its MFMAs the slot
      // is refilled with step k0 + 32 (q + kBP) (clamped to a valid fragment past the end)
      for (int k0 = 0; k0 < K2; k0 += 32 * kBP) {
#pragma unroll
        for (int q = 0; q < kBP; ++q) {
          const int ks = k0 + 32 * q;
          if (ks >= K2) break;  // uniform
          uint4_t av[FM];
#pragma unroll
          for (int m = 0; m < FM; ++m)
            av[m] = *reinterpret_cast<const uint4_t*>(lds + (m * 16 + lr) * ldsw + ks + lk);
#pragma unroll
          for (int m = 0; m < FM; ++m)
#pragma unroll
            for (int n = 0; n < FN; ++n) acc[m][n] = mfma16(av[m], bq[q][n], acc[m][n]);
          const int kn = ks + 32 * kBP;
#pragma unroll
          for (int n = 0; n < FN; ++n) bq[q][n] = fm_frag(W, cb + n * 16, kn < K2 ? kn : 0, K2, lane);
        }
      }
    }
    if (alias_out) __syncthreads();  // every wave is done reading the A tile
    if (cb < H) {
#pragma unroll
      for (int m = 0; m < FM; ++m)
#pragma unroll
        for (int n = 0; n < FN; ++n)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = m * 16 + (lane >> 4) * 4 + j;
            otile[row * ldo + wave * 64 + n * 16 + lr] = f2bf(fmaxf(acc[m][n][j], 0.f));
          }
    }
    __syncthreads();
    TR_STAMP(a.prof, tb, 4);
    const int ncols = (H - cchunk) < kTrBN ? (H - cchunk) : kTrBN;
    // tree-mean epilogue: A_next[parent] = [h[self slot] | mean_{j < Fg} h[j]] for every
    // sibling group of the block (item = (group, column pair), 4-byte stores)
    {
      const int groups = BM >> a.logPg;
      const int pairs = ncols >> 1;
      for (int it = threadIdx.x; it < groups * pairs; it += 256) {
        const int gi = it / pairs;
        const int c = (it - gi * pairs) * 2;
        const int base = gi << a.logPg;
        if (row0 + base >= a.M) continue;
        const uint32_t selfp = *reinterpret_cast<const uint32_t*>(otile + (base + a.Fg) * ldo + c);
        float s0 = 0.f, s1 = 0.f;
        for (int j = 0; j < a.Fg; ++j) {
          const uint32_t v = *reinterpret_cast<const uint32_t*>(otile + (base + j) * ldo + c);
          s0 += bf_lo(v);
          s1 += bf_hi(v);
        }
        if (a.include_self) {
          s0 += bf_lo(selfp);
          s1 += bf_hi(selfp);
        }
        const int64_t parent = (row0 >> a.logPg) + gi;
        bf16_t* dst = a.a_next + parent * 2 * H + cchunk + c;
        *reinterpret_cast<uint32_t*>(dst) = selfp;
        *reinterpret_cast<uint32_t*>(dst + H) = pack_bf16x2(s0 * a.inv_grp, s1 * a.inv_grp);
      }
    }
    // ReLU bits for the backward: word (32-row block, column) has bit i set iff row i > 0
    if (a.mask) {
      constexpr int KBB = BM / 32;
      for (int it = threadIdx.x; it < KBB * ncols; it += 256) {
        const int kbl = it / ncols, n = it - kbl * ncols;
        const int64_t gr = row0 + kbl * 32;
        if (gr >= a.M) continue;
        uint32_t bits = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) bits |= (bf_pos(otile[(kbl * 32 + i) * ldo + n]) ? 1u : 0u) << i;
        a.mask[(gr >> 5) * H + cchunk + n] = bits;
      }
    }
    __syncthreads();
  }
  TR_STAMP(a.prof, tb, 5);
}

// ----------------------------------------------------------------------------
// tr_fwd2: layer 0 (mode 0) with 64 target rows and 8 waves per block.  Versus
// tr_fwd_kernel<BM=32> (4 waves, each 64 columns x 32 rows):
//   * every wave multiplies all 64 rows by its 32 columns, so a weight fragment fetched
//     from L2 serves 64 rows instead of 32 (the GEMM phase was bound by re-fetching W
//     per 32 rows: 800 blocks x 128 KB);
//   * the A tile has no padding; 16-B chunk c of row r lives at chunk c ^ (r & 15), so
//     each ds_read_b128 lane group ({0-3,12-15,20-27}, ...: rows 0-15 x k-quarters 0/1
//     or 2/3) touches 16 distinct 16-B bank slots (the padded layout put two lanes of a
//     group on one slot: a 2-way conflict on every fragment read);
//   * the ReLU'd output goes to LDS transposed ([column][row], row stride 68 bf16 =
//     34 dwords): one 8-byte store per lane per MFMA tile instead of four 2-byte ones,
//     and the tree-mean / ReLU-bit epilogue reads whole 4-row words (ds_read_b64), all
//     bank-conflict-free (34c mod 64 is distinct for the 32 lanes of a half-wave).
// Needs D % 64 == 0 (A rows of a multiple of 16 chunks), M % 64 == 0 and sibling groups
// of at most 64 rows (else tr_fwd_kernel).
// ----------------------------------------------------------------------------
constexpr int kF2Rows = 64, kF2Threads = 512, kF2Ldt = kF2Rows + 4;
// F2_ALIAS=1: the output tile aliases the A tile (one region of max(A, O) bytes, a barrier
// between the last A read and the first O write): ~38 KB of LDS per block instead of ~70 KB
#ifndef F2_ALIAS
#define F2_ALIAS 1
#endif
// k-steps of weight fragments in flight in the GEMM (2 per wave = 16 VGPRs, 4 = 32)
#ifndef F2_WPF
#define F2_WPF 4
#endif

// GO = 1 (pipelined step, mode 3): the gather already ran in the previous launch (gather
// blocks of tr_opt, tr_gather32_tile): the A tile is loaded from a.a_rows and the kt copy
// for dW exists; only the GEMM, the tree mean, the ReLU bits and the head's Wc remain.
template <typename FT, int GO>
__global__ __launch_bounds__(kF2Threads, 4) void tr_fwd2_kernel(TrFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  constexpr int BM = kF2Rows, NT = kF2Threads;
  const int tb = static_cast<int>(blockIdx.x), ntb = static_cast<int>(gridDim.x);
  const int D = a.D, K2 = 2 * D, H = a.H;
  const int tile = xcd_remap(tb, ntb);
  const int64_t row0 = static_cast<int64_t>(tile) * BM;
  // LDS: A tile [BM][K2] (swizzled) | output tile [kTrBN][kF2Ldt] (transposed) | ids
  bf16_t* At = lds;
#if F2_ALIAS
  bf16_t* Ot = lds;
  int32_t* node_s = reinterpret_cast<int32_t*>(lds + (BM * K2 > kTrBN * kF2Ldt ? BM * K2 : kTrBN * kF2Ldt));
#else
  bf16_t* Ot = lds + BM * K2;
  int32_t* node_s = reinterpret_cast<int32_t*>(Ot + kTrBN * kF2Ldt);
#endif
  int32_t* leaf_s = node_s + BM;
  TR_STAMP(a.prof, tb, 0);
  if (a.prof && threadIdx.x == 0) a.prof[tb * 8 + 6] = static_cast<long long>(__smid());  // XCC / SE / CU
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lg = lane >> 4;
  if (tb == 0 && tid == 0) {
    if (a.step) a.step[0] += 1;
    a.rng[1] += 1;  // this batch is consumed: the sampler draws the next counter
  }
  for (int i = tb * NT + tid; i < a.B; i += ntb * NT) a.roots_cur[i] = a.roots_in[i];
  if constexpr (GO) {
    // A rows [64][K2] (row-major, 16-byte chunks) -> the swizzled LDS tile
    const int cpr2 = K2 >> 3;
    for (int it = tid; it < BM * cpr2; it += NT) {
      const int r = it / cpr2, c = it - r * cpr2;
      *reinterpret_cast<uint4_t*>(At + r * K2 + f2_chunk(r, c) * 8) =
          *reinterpret_cast<const uint4_t*>(a.a_rows + (row0 + r) * K2 + c * 8);
    }
  } else {
    if (tid < BM) node_s[tid] = a.nodes[row0 + tid];
    for (int it = tid; it < BM * a.FL; it += NT) leaf_s[it] = a.leaf[row0 * a.FL + it];
    __syncthreads();
  }
  TR_STAMP(a.prof, tb, 1);
  // ---- gather + mean: item = (used row, 8-column chunk); two items per thread, every leaf
  // load of both in flight; padding ids (-1) read row 0 and are zeroed at use.  Only the
  // Fg + 1 used slots of each sibling group are items (F2_SKIP_PAD; at fanout 25, 26 of
  // every 32 rows): the unused slots' A rows are zero-filled instead of gathered.
  if constexpr (!GO) f2_gather<FT, BM, NT>(a, At, node_s, leaf_s, tid);
  // the head's Wc tiles (wave 0, after the gather: its registers are free again)
  if (a.ncomb && wave == 0) tr_comb_wave(a.comb, tb, ntb, lane);
  // the first WPF k-steps of this wave's weight fragments load behind the kt pass (not
  // earlier: held through the gather they would push its 20 row loads in flight to spill)
  const bf16_t* W = a.W;
  constexpr int WPF = F2_WPF;
  uint4_t bq[WPF][2];
  if (wave * 32 < H) {
#pragma unroll
    for (int q = 0; q < WPF; ++q)
#pragma unroll
      for (int n = 0; n < 2; ++n) bq[q][n] = fm_frag(W, wave * 32 + n * 16, q * 32 < K2 ? q * 32 : 0, K2, lane);
  }
  __syncthreads();
  TR_STAMP(a.prof, tb, 2);
  // ---- A tile -> kt layout (dW operand): item = (column pair, 8-row chunk), column pairs
  // fastest: a half-wave's 4-byte reads cover 128 contiguous (permuted) bytes of a row
  if constexpr (!GO) f2_kt<BM, NT>(a, row0, At, tid);
  TR_STAMP(a.prof, tb, 3);
  // ---- MFMA GEMM out of LDS: wave w owns columns w*32..+31 of each 256-column chunk, all
  // 64 rows; two k-steps of weight fragments in flight
  constexpr int FM = BM / 16, FN = 2;
  for (int cchunk = 0; cchunk < H; cchunk += kTrBN) {
    const int cb = cchunk + wave * 32;
    float4_t acc[FM][FN];
    tl_zero(acc);
    if (cb < H) {
      if (cchunk > 0) {
#pragma unroll
        for (int q = 0; q < WPF; ++q)
#pragma unroll
          for (int n = 0; n < FN; ++n) bq[q][n] = fm_frag(W, cb + n * 16, q * 32 < K2 ? q * 32 : 0, K2, lane);
      }
      for (int k0 = 0; k0 < K2; k0 += 32 * WPF) {
#pragma unroll
        for (int q = 0; q < WPF; ++q) {
          const int ks = k0 + 32 * q;
          if (ks >= K2) break;  // uniform
          uint4_t av[FM];
          const int phys = f2_chunk(lr, (ks >> 3) + lg) * 8;
#pragma unroll
          for (int m = 0; m < FM; ++m) av[m] = *reinterpret_cast<const uint4_t*>(At + (m * 16 + lr) * K2 + phys);
#pragma unroll
          for (int m = 0; m < FM; ++m)
#pragma unroll
            for (int n = 0; n < FN; ++n) acc[m][n] = mfma16(av[m], bq[q][n], acc[m][n]);
          const int kn = ks + 32 * WPF;
#pragma unroll
          for (int n = 0; n < FN; ++n) bq[q][n] = fm_frag(W, cb + n * 16, kn < K2 ? kn : 0, K2, lane);
        }
      }
    }
#if F2_ALIAS
    __syncthreads();  // every wave is done reading the A tile the output tile overwrites
#endif
    if (cb < H) {
      // ReLU -> transposed output tile: 4 consecutive rows of one column per 8-byte store
#pragma unroll
      for (int m = 0; m < FM; ++m)
#pragma unroll
        for (int n = 0; n < FN; ++n) {
          tl_uint2 v;
          v[0] = pack_bf16x2(fmaxf(acc[m][n][0], 0.f), fmaxf(acc[m][n][1], 0.f));
          v[1] = pack_bf16x2(fmaxf(acc[m][n][2], 0.f), fmaxf(acc[m][n][3], 0.f));
          *reinterpret_cast<tl_uint2*>(Ot + (wave * 32 + n * 16 + lr) * kF2Ldt + m * 16 + lg * 4) = v;
        }
    }
    __syncthreads();
    TR_STAMP(a.prof, tb, 4);
    const int ncols = (H - cchunk) < kTrBN ? (H - cchunk) : kTrBN;
    // tree-mean epilogue: item = (sibling group, column); the group's rows are contiguous
    // in the column's LDS row: 8-byte reads of 4 rows
    {
      const int P = 1 << a.logPg;
      const int groups = BM >> a.logPg;
      for (int it = tid; it < groups * ncols; it += NT) {
        const int gi = it / ncols, c = it - gi * ncols;
        const bf16_t* col = Ot + c * kF2Ldt + (gi << a.logPg);
        float s = 0.f, self = 0.f;
        for (int r4 = 0; r4 < P; r4 += 4) {
          const tl_uint2 v = *reinterpret_cast<const tl_uint2*>(col + r4);
          const float e[4] = {bf_lo(v[0]), bf_hi(v[0]), bf_lo(v[1]), bf_hi(v[1])};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = r4 + j;
            s += r < a.Fg ? e[j] : 0.f;
            self = r == a.Fg ? e[j] : self;
          }
        }
        if (a.include_self) s += self;
        const int64_t parent = (row0 >> a.logPg) + gi;
        bf16_t* dst = a.a_next + parent * 2 * H + cchunk + c;
        dst[0] = f2bf(self);
        dst[H] = f2bf(s * a.inv_grp);
      }
    }
    // ReLU bits for the backward: word (32-row block, column) has bit i set iff row i > 0
    if (a.mask) {
      for (int it = tid; it < (BM / 32) * ncols; it += NT) {
        const int kbl = it / ncols, c = it - kbl * ncols;
        const bf16_t* col = Ot + c * kF2Ldt + kbl * 32;
        uint32_t bits = 0;
#pragma unroll
        for (int r4 = 0; r4 < 32; r4 += 4) {
          const tl_uint2 v = *reinterpret_cast<const tl_uint2*>(col + r4);
          bits |= (bf_pos(static_cast<bf16_t>(v[0] & 0xffffu)) ? 1u : 0u) << r4;
          bits |= (bf_pos(static_cast<bf16_t>(v[0] >> 16)) ? 1u : 0u) << (r4 + 1);
          bits |= (bf_pos(static_cast<bf16_t>(v[1] & 0xffffu)) ? 1u : 0u) << (r4 + 2);
          bits |= (bf_pos(static_cast<bf16_t>(v[1] >> 16)) ? 1u : 0u) << (r4 + 3);
        }
        a.mask[((row0 >> 5) + kbl) * H + cchunk + c] = bits;
      }
    }
    __syncthreads();
  }
  TR_STAMP(a.prof, tb, 5);
}

// ----------------------------------------------------------------------------
// tr_bwd (3-hop inner layer): G rows routed from the parent gradient through the tree
// and the ReLU bits, then dA_out = G @ W (fp32 rows)
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tr_bwd_kernel(TrBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  constexpr int BM = 32;
  const int Hk = a.Hk, K2 = a.K2out;
  const int ldg = Hk + 8;
  const int64_t row0 = static_cast<int64_t>(xcd_remap(blockIdx.x, gridDim.x)) * BM;
  const int Pm = (1 << a.logPg) - 1;
  for (int it = threadIdx.x; it < BM * Hk; it += 256) {
    const int r = it / Hk, n = it - r * Hk;
    const int64_t row = row0 + r;
    float v = 0.f;
    if (row < a.M && ((a.mask[(row >> 5) * Hk + n] >> (row & 31)) & 1u)) {
      const int64_t t = row >> a.logPg;
      const int j = static_cast<int>(row & Pm);
      const float dn = a.dA[t * 2 * Hk + Hk + n] * a.inv;
      if (j < a.Fg) v = dn;
      else if (j == a.Fg) v = a.dA[t * 2 * Hk + n] + (a.include_self ? dn : 0.f);
    }
    lds[r * ldg + n] = f2bf(v);
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  constexpr int FM = BM / 16, FN = 4;
  for (int cchunk = 0; cchunk < K2; cchunk += kTrBN) {
    const int cb = cchunk + wave * 64;
    if (cb >= K2) continue;
    float4_t acc[FM][FN];
    tl_zero(acc);
    for (int k0 = 0; k0 < Hk; k0 += 32) {
      uint4_t b[FN], av[FM];
#pragma unroll
      for (int n = 0; n < FN; ++n) b[n] = fm_frag(a.WT, cb + n * 16, k0, Hk, lane);
#pragma unroll
      for (int m = 0; m < FM; ++m) av[m] = *reinterpret_cast<const uint4_t*>(lds + (m * 16 + lr) * ldg + k0 + lk);
#pragma unroll
      for (int m = 0; m < FM; ++m)
#pragma unroll
        for (int n = 0; n < FN; ++n) acc[m][n] = mfma16(av[m], b[n], acc[m][n]);
    }
#pragma unroll
    for (int m = 0; m < FM; ++m)
#pragma unroll
      for (int n = 0; n < FN; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t row = row0 + m * 16 + (lane >> 4) * 4 + j;
          if (row < a.M) a.dA_out[row * K2 + cb + n * 16 + lr] = acc[m][n][j];
        }
  }
}

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

size_t eh_tr_fwd_lds(int D, int H, int bm, int FL, int mode) {
  const int K2 = 2 * D;
  const bool alias_out = H <= kTrBN && kTrBN <= K2;
  size_t b = static_cast<size_t>(bm) * (K2 + 8) * sizeof(bf16_t);
  if (mode != 1 && !alias_out) b += static_cast<size_t>(bm) * (kTrBN + 8) * sizeof(bf16_t);
  if (mode != 2) b += static_cast<size_t>(bm) * (1 + FL) * sizeof(int32_t);
  return b;
}

size_t eh_tr_fwd2_lds(int D, int FL) {
  const size_t a = static_cast<size_t>(kF2Rows) * 2 * D, o = static_cast<size_t>(kTrBN) * kF2Ldt;
  return (F2_ALIAS ? (a > o ? a : o) : a + o) * sizeof(bf16_t) + static_cast<size_t>(kF2Rows) * (1 + FL) * sizeof(int32_t);
}

// the 64-row / 8-wave layer-0 kernel applies (EULER_AMD_FWD2=0 disables it)
static bool fwd2_fits(const TrFwdArgs& a) {
  static const bool off = [] {
    const char* e = std::getenv("EULER_AMD_FWD2");
    return e && e[0] == '0';
  }();
  if (off || !a.a_kt) return false;
  if (a.D % 64 != 0 || a.M % kF2Rows != 0 || a.logPg < 2 || (1 << a.logPg) > kF2Rows) return false;
  if (F2_ALIAS && a.H > kTrBN) return false;  // the aliased A tile must outlive every column chunk
  return eh_tr_fwd2_lds(a.D, a.FL) <= 80 * 1024;  // two blocks per CU
}

hipError_t eh_tr_sample(const TrSampleArgs* a, hipStream_t s) {
  if (a->M <= 0) return hipSuccess;
  const int64_t nblk = ceil_div(a->M, kTrSampleRows);
  if (!tr_sample_ok(*a, kTrSampleRows, nblk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tr_sample_kernel, dim3(static_cast<uint32_t>(nblk)), dim3(256), 0, s, *a);
  return hipGetLastError();
}

hipError_t eh_tr_fwd(const TrFwdArgs* a, int mode, int feat_fp32, int bm, hipStream_t s) {
  if (a->M <= 0) return hipSuccess;
  // every pointer the chosen mode dereferences must be set
  if (!a->x || !a->a_next) return hipErrorInvalidValue;
  if (mode != 2 && (!a->nodes || !a->leaf || !a->rng || a->FL < 1 || !a->roots_in || !a->roots_cur || a->B < 1))
    return hipErrorInvalidValue;
  if (mode != 1 && !a->W) return hipErrorInvalidValue;
  if (a->D % 16 != 0 || a->D <= 0 || a->M % bm != 0) return hipErrorInvalidValue;
  if (mode != 1 && (a->H % 64 != 0 || a->H <= 0 || (bm >> a->logPg) < 1 || (bm & ((1 << a->logPg) - 1)) != 0 ||
                    a->Fg >= (1 << a->logPg)))
    return hipErrorInvalidValue;
  if (mode == 2 && feat_fp32) return hipErrorInvalidValue;
  if (a->ncomb < 0 || (a->ncomb > 0 && (mode == 2 || !a->comb.wout || !a->comb.bfc || !a->comb.Wc ||
                                        !a->comb.WcT || !a->comb.bc || !a->comb.wout_sh || !a->comb.wfcT_sh ||
                                        a->comb.C % 16 != 0 || a->comb.H % 16 != 0 || a->comb.E % 32 != 0)))
    return hipErrorInvalidValue;
  // mode 3: GEMM-only (pipelined step), the A rows come from the gather blocks
  if (mode == 3 && (!fwd2_fits(*a) || !a->a_rows)) return hipErrorInvalidValue;
  if (mode == 3 || (mode == 0 && fwd2_fits(*a))) {
    void (*const k2)(TrFwdArgs) = mode == 3  ? tr_fwd2_kernel<bf16_t, 1>
                                  : feat_fp32 ? tr_fwd2_kernel<float, 0>
                                              : tr_fwd2_kernel<bf16_t, 0>;
    const size_t l2 = eh_tr_fwd2_lds(a->D, a->FL);
    EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k2), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(l2)));
    hipLaunchKernelGGL(k2, dim3(static_cast<uint32_t>(a->M / kF2Rows)), dim3(kF2Threads), l2, s, *a);
    return hipGetLastError();
  }
  const size_t lds = eh_tr_fwd_lds(a->D, a->H, bm, a->FL, mode);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>(a->M / bm));
#define TR_FWD(FT, BMV, MODEV)                                                                               \
  do {                                                                                                       \
    EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(tr_fwd_kernel<FT, BMV, MODEV>),         \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds))); \
    hipLaunchKernelGGL((tr_fwd_kernel<FT, BMV, MODEV>), grid, dim3(256), lds, s, *a);                       \
    return hipGetLastError();                                                                                \
  } while (0)
#define TR_FWD_BM(FT, MODEV)                 \
  do {                                       \
    if (bm == 32) TR_FWD(FT, 32, MODEV);     \
    if (bm == 64) TR_FWD(FT, 64, MODEV);     \
    if (bm == 128) TR_FWD(FT, 128, MODEV);   \
  } while (0)
  if (mode == 0) {
    if (feat_fp32) TR_FWD_BM(float, 0);
    else TR_FWD_BM(bf16_t, 0);
  } else if (mode == 1) {
    if (feat_fp32) TR_FWD_BM(float, 1);
    else TR_FWD_BM(bf16_t, 1);
  } else if (mode == 2) {
    TR_FWD_BM(bf16_t, 2);
  }
#undef TR_FWD_BM
#undef TR_FWD
  return hipErrorInvalidValue;
}

hipError_t eh_tr_bwd(const TrBwdArgs* a, hipStream_t s) {
  if (!a->dA || !a->mask || !a->WT || !a->dA_out) return hipErrorInvalidValue;
  if (a->M % 32 != 0 || a->Hk % 32 != 0 || a->K2out % 64 != 0 || a->logPg < 4) return hipErrorInvalidValue;
  const size_t lds = static_cast<size_t>(32) * (a->Hk + 8) * sizeof(bf16_t);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(tr_bwd_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  hipLaunchKernelGGL(tr_bwd_kernel, dim3(static_cast<uint32_t>(a->M / 32)), dim3(256), lds, s, *a);
  return hipGetLastError();
}

}  // extern "C"
