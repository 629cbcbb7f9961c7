// Forward-only scoring of the fused graph-classification models (GIN / GraphGCN): the
// logits and pooled embeddings of an explicit request list, see GcInferArgs in
// graph_cls_args.h and GraphClsPlan::infer in binding_graph_cls.cpp.
//
// One block (4 waves) per pack of up to 16 consecutive requests whose nodes fill at most R
// LDS rows; graph q owns rows [r0_q, r0_q + n_q).  Nothing of the training step's backward
// (Z stash, dZ, dY, gradient slab) exists here, so the LDS holds
//   A   [nadj][R][R]  block-diagonal edge counts, one block per graph of the pack
//   S   [R][trp]      feature bag matrix, T [trp][D0] the embedding table
//   X   2 x [R][dmax] ping-pong activations, Z [R][kmax] the current conv's aggregate
//   P   [16][R]       graph membership (P[q][r] = 1 for r in graph q's rows)
//   PX  [16][DL], PE [16][E]  the pooled head's operands
// and every product is fp32 MFMA tiles (v_mfma_f32_16x16x4_f32, operand layout as in
// graph_cls.hip) dealt to the waves: X0 = S T; per conv Z = aggregate(A, X) and
// X' = relu(Z [W | Wf]^T + b); then the head as three GEMMs over the pack's graphs,
// PX = P X_L, PE = PX Wfc^T + n_q bfc (the pooled embedding), logits = PE Wout^T.  A is
// block-diagonal, so a row tile's aggregation only runs over the columns of the graphs that
// intersect it (s_klo / s_khi).  Every output element is written once; nothing is drawn.
#include "hip/common.h"
#include "hip/graph_cls_args.h"

namespace euler_hip {

namespace {

constexpr int kWaves = kGcThreads / 64;
constexpr int kMaxRowTiles = kGcMaxRows / 16;

__device__ __forceinline__ float4_t mfma_f32x4(float a, float b, float4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// uniform selection from a per-layer argument array (no dynamic indexing of kernel args)
template <typename T, int N>
__device__ __forceinline__ T gi_pick(const T (&arr)[N], int l) {
  T r = arr[0];
#pragma unroll
  for (int i = 1; i < N; ++i)
    if (l == i) r = arr[i];
  return r;
}

// one 16 x 16 output tile over k in [k0, k1) (multiples of 4): fa(k) / fb(k) give this
// lane's A[lane & 15][k] / B[k][lane & 15]
template <typename FA, typename FB>
__device__ __forceinline__ float4_t gi_tile(FA fa, FB fb, int k0, int k1) {
  const int lk = (threadIdx.x & 63) >> 4;
  float4_t acc = {0.f, 0.f, 0.f, 0.f};
  int k = k0;
  for (; k + 16 <= k1; k += 16) {
    float av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = fa(k + 4 * u + lk);
      bv[u] = fb(k + 4 * u + lk);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = mfma_f32x4(av[u], bv[u], acc);
  }
  for (; k < k1; k += 4) acc = mfma_f32x4(fa(k + lk), fb(k + lk), acc);
  return acc;
}

__global__ __launch_bounds__(kGcThreads) void gc_infer_kernel(GcInferArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gi_smem[];
  __shared__ int s_rec[kGcPackGraphs][kGcRec];
  __shared__ int s_r0[kGcPackGraphs];
  __shared__ int s_klo[kMaxRowTiles], s_khi[kMaxRowTiles];
  __shared__ int s_used;  // rows of the pack; -1: a pack table the host would never build
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int R = a.R, L = a.L, kind = a.kind, selfl = a.self_loops;
  auto F = [&](int32_t off) { return reinterpret_cast<float*>(gi_smem + off); };
  float* A = F(a.lds_a);
  float* IC = F(a.lds_invc);
  float* Sm = F(a.lds_s);
  float* Tt = F(a.lds_t);
  float* P = F(a.lds_p);
  const int ldx = a.ldx, ldz = a.ldz, lda = a.lda, ldsm = a.ldsm, ldt = a.ldt, trp = a.trp;

  // ---------------------------------------------------------------- the pack, staging
  const int32_t* pk = a.pack + static_cast<int64_t>(blockIdx.x) * kGcPackRec;
  const int q0 = pk[0], cnt = pk[1];
  if (q0 < 0 || cnt < 1 || cnt > kGcPackGraphs || q0 > a.n - cnt) return;  // uniform
  for (int i = tid; i < cnt * kGcRec; i += kGcThreads) {
    const int q = i / kGcRec, f = i - q * kGcRec;
    const int g = a.gidx[q0 + q];
    s_rec[q][f] = (g >= 0 && g < a.G) ? a.rec[static_cast<int64_t>(g) * kGcRec + f] : 0;
  }
  if (tid < cnt) s_r0[tid] = pk[2 + tid];
  const int D0 = a.D[0];
  for (int i = tid; i < trp * D0; i += kGcThreads) {  // the table, padding rows zero
    const int r = i / D0, c = i - r * D0;
    Tt[r * ldt + c] = r < a.tab_rows ? a.table[i] : 0.f;
  }
  for (int i = tid; i < a.nadj * R * lda; i += kGcThreads) A[i] = 0.f;
  for (int i = tid; i < a.nadj * R; i += kGcThreads) IC[i] = 0.f;
  for (int i = tid; i < R * ldsm; i += kGcThreads) Sm[i] = 0.f;
  for (int i = tid; i < kGcPackGraphs * lda; i += kGcThreads) P[i] = 0.f;
  __syncthreads();
  if (tid == 0) {
    // the graphs' rows are consecutive; each row tile's aggregation columns are those of
    // the graphs that intersect it, rounded to the MFMA's K step
    int end = 0;
    for (int q = 0; q < cnt; ++q) {
      const int n = s_rec[q][0];
      if (end >= 0 && (s_r0[q] != end || n < 0 || n > R - end)) end = -1;
      if (end >= 0) end += n;
    }
    s_used = end;
    for (int rt = 0; rt < kMaxRowTiles; ++rt) {
      int lo = R, hi = 0;
      for (int q = 0; q < cnt && end >= 0; ++q) {
        const int r0 = s_r0[q], r1 = r0 + s_rec[q][0];
        if (r1 > r0 && r0 < rt * 16 + 16 && r1 > rt * 16) {
          lo = min(lo, r0);
          hi = max(hi, r1);
        }
      }
      s_klo[rt] = lo & ~3;
      s_khi[rt] = hi > 0 ? (hi + 3) & ~3 : (lo & ~3);
    }
  }
  __syncthreads();
  const int used = s_used;
  if (used < 0) return;  // uniform
  const int nrt = (used + 15) >> 4, uk = (used + 3) & ~3;

  // ---------------------------------------------------------------- densify the pack
  // A_j[r0 + t][r0 + s] += 1 per edge t <- s, deg_j += 1; S[r0 + v][row] += bag weight; P
  // (LDS float atomics of integers / equal weights: exact in any order); a wave per graph
  for (int q = wave; q < cnt; q += kWaves) {
    const int r0 = s_r0[q], n = s_rec[q][0];
#pragma unroll
    for (int j = 0; j < kGcMaxAdj; ++j) {
      if (j < a.nadj) {
        const int32_t* pr = a.adj[j].pair;
        for (int e = s_rec[q][3 + 2 * j] + lane; e < s_rec[q][4 + 2 * j]; e += 64) {
          const int p = pr[e];
          const int t = p >> 8, s = p & 255;
          if (t >= 0 && t < n && s < n) {
            atomicAdd(A + (j * R + r0 + t) * lda + r0 + s, 1.f);
            atomicAdd(IC + j * R + r0 + t, 1.f);
          }
        }
      }
    }
    for (int f = s_rec[q][1] + lane; f < s_rec[q][2]; f += 64) {
      const int p = a.fpair[f];
      const int v = p >> 16, row = p & 0xffff;
      if (v >= 0 && v < n && row < trp) atomicAdd(Sm + (r0 + v) * ldsm + row, a.fw[f]);
    }
    for (int v = lane; v < n; v += 64) P[q * lda + r0 + v] = 1.f;
  }
  __syncthreads();
  // 1 / cnt (GraphConv mean: in-degree + self loop; 0 for padding rows)
  for (int i = tid; i < a.nadj * R; i += kGcThreads) {
    const float c = IC[i] + static_cast<float>(selfl);
    IC[i] = (i % R < used && c > 0.f) ? 1.f / c : 0.f;
  }
  // X0 = S T (the embedding bag)
  {
    float* X0 = F(a.lds_x[0]);
    const int nct = D0 >> 4;
    for (int tile = wave; tile < nrt * nct; tile += kWaves) {
      const int rt = tile / nct, ct = tile - rt * nct;
      const int v0 = rt * 16, c = ct * 16 + lr;
      const float4_t acc = gi_tile([&](int r) { return Sm[(v0 + lr) * ldsm + r]; },
                                   [&](int r) { return Tt[r * ldt + c]; }, 0, trp);
#pragma unroll
      for (int j = 0; j < 4; ++j) X0[(v0 + lk * 4 + j) * ldx + c] = acc[j];
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- convs
  float* Z = F(a.lds_z);
  int cur = 0;
  for (int l = 0; l < L; ++l) {
    const int Din = gi_pick(a.D, l), Dout = gi_pick(a.D, l + 1);
    const int K = kind == 1 ? 2 * Din : Din;
    const float* X = F(a.lds_x[cur]);
    float* Y = F(a.lds_x[cur ^ 1]);
    const int jm = gi_pick(a.adj_of, l);
    const float* Aj = A + jm * R * lda;
    const float* invc = IC + jm * R;
    const float cdiag = 1.f + (kind == 0 ? gi_pick(a.eps, l)[0] : 0.f) + static_cast<float>(selfl);
    // aggregate:  GIN  Z = A X + (1 + eps + self) X;  GraphConv  Z = [X | (A X + self X) / cnt]
    {
      const int nct = Din >> 4;
      for (int tile = wave; tile < nrt * nct; tile += kWaves) {
        const int rt = tile / nct, ct = tile - rt * nct;
        const int t0 = rt * 16, k = ct * 16 + lr;
        const float4_t acc = gi_tile([&](int s) { return Aj[(t0 + lr) * lda + s]; },
                                     [&](int s) { return X[s * ldx + k]; }, s_klo[rt], s_khi[rt]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int t = t0 + lk * 4 + j;
          const float xt = X[t * ldx + k];
          if (kind == 0) {
            Z[t * ldz + k] = acc[j] + cdiag * xt;
          } else {
            Z[t * ldz + k] = xt;
            Z[t * ldz + Din + k] = (acc[j] + static_cast<float>(selfl) * xt) * invc[t];
          }
        }
      }
    }
    __syncthreads();
    // linear:  Y = relu(Z [W | Wf]^T + b), rows beyond the pack's zero
    {
      const float* W = gi_pick(a.W, l);
      const float* Wf = gi_pick(a.Wf, l);
      const float* bias = kind == 1 ? gi_pick(a.bl, l) : nullptr;
      const int nct = Dout >> 4;
      for (int tile = wave; tile < nrt * nct; tile += kWaves) {
        const int rt = tile / nct, ct = tile - rt * nct;
        const int t0 = rt * 16, o = ct * 16 + lr;
        const float* zr = Z + (t0 + lr) * ldz;
        const float* wr = W + o * Din;
        const float* fr = Wf + o * Din - Din;
        const float4_t acc =
            gi_tile([&](int k) { return zr[k]; }, [&](int k) { return k < Din ? wr[k] : fr[k]; }, 0, K);
        const float bo = bias ? bias[o] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int t = t0 + lk * 4 + j;
          Y[t * ldx + o] = t < used ? fmaxf(acc[j] + bo, 0.f) : 0.f;
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---------------------------------------------------------------- pooled head
  // node_emb = fc(x_L), add pooling, out_fc:  PE = (P X_L) Wfc^T + n_q bfc,  logits = PE Wout^T
  const int DL = gi_pick(a.D, L), E = a.E, C = a.C;
  const float* XL = F(a.lds_x[cur]);
  float* PX = F(a.lds_px);
  float* PE = F(a.lds_pe);
  const int ldpe = a.ldpe;
  for (int ct = wave; ct < (DL >> 4); ct += kWaves) {
    const int c = ct * 16 + lr;
    const float4_t acc =
        gi_tile([&](int s) { return P[lr * lda + s]; }, [&](int s) { return XL[s * ldx + c]; }, 0, uk);
#pragma unroll
    for (int j = 0; j < 4; ++j) PX[(lk * 4 + j) * ldx + c] = acc[j];
  }
  __syncthreads();
  for (int ct = wave; ct < ((E + 15) >> 4); ct += kWaves) {
    const int e = ct * 16 + lr;
    const float* wr = a.Wfc + static_cast<int64_t>(min(e, E - 1)) * DL;
    const float4_t acc =
        gi_tile([&](int k) { return PX[lr * ldx + k]; }, [&](int k) { return e < E ? wr[k] : 0.f; }, 0, DL);
    const float be = e < E ? a.bfc[e] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = lk * 4 + j;
      const bool live = q < cnt && e < E;
      const float v = live ? acc[j] + static_cast<float>(s_rec[q][0]) * be : 0.f;
      PE[q * ldpe + e] = v;  // columns e >= E zero: the K padding of the logits' tile
      if (live) a.emb[static_cast<int64_t>(q0 + q) * E + e] = v;
    }
  }
  __syncthreads();
  for (int ct = wave; ct < ((C + 15) >> 4); ct += kWaves) {
    const int c = ct * 16 + lr;
    const float* wr = a.Wout + static_cast<int64_t>(min(c, C - 1)) * E;
    const float4_t acc = gi_tile([&](int k) { return PE[lr * ldpe + k]; },
                                 [&](int k) { return (c < C && k < E) ? wr[k] : 0.f; }, 0, (E + 3) & ~3);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = lk * 4 + j;
      if (q < cnt && c < C) a.logits[static_cast<int64_t>(q0 + q) * C + c] = acc[j];
    }
  }
}

}  // namespace

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

hipError_t eh_gc_infer(const GcInferArgs* a, hipStream_t s) {
  if (!a || a->L < 1 || a->L > kGcMaxLayers || a->n < 1 || a->npacks < 1 || a->npacks > a->n || a->G < 1 ||
      a->R < 16 || a->R % 16 != 0 || a->R > kGcMaxRows || a->nadj < 1 || a->nadj > kGcMaxAdj || a->E < 1 ||
      a->E > kGcMaxWidth || a->C < 1 || a->C > kGcMaxLabels || a->tab_rows < 1 || a->tab_rows > kGcMaxTableRows ||
      a->trp % 16 != 0 || a->trp < a->tab_rows || a->tab_rows * a->D[0] > kGcMaxTable || a->lds_bytes < 1 ||
      a->lds_bytes > 160 * 1024 - kGcInferStaticLds || !a->rec || !a->fpair || !a->fw || !a->table || !a->Wfc || !a->bfc || !a->Wout ||
      !a->gidx || !a->pack || !a->logits || !a->emb || (a->kind != 0 && a->kind != 1))
    return hipErrorInvalidValue;
  int dmax = 0;
  for (int l = 0; l <= a->L; ++l) {
    if (a->D[l] < 16 || a->D[l] % 16 != 0 || a->D[l] > kGcMaxWidth) return hipErrorInvalidValue;
    dmax = a->D[l] > dmax ? a->D[l] : dmax;
  }
  // the leading dimensions the kernel indexes with must cover what it indexes
  if (a->ldx < dmax || a->ldz < (a->kind == 1 ? 2 * dmax : dmax) || a->lda < a->R || a->ldsm < a->trp ||
      a->ldt < a->D[0] || a->ldpe < (a->E + 15) / 16 * 16)
    return hipErrorInvalidValue;
  for (int l = 0; l < a->L; ++l) {
    if (!a->W[l] || a->adj_of[l] < 0 || a->adj_of[l] >= a->nadj) return hipErrorInvalidValue;
    if (a->kind == 0 && !a->eps[l]) return hipErrorInvalidValue;
    if (a->kind == 1 && (!a->Wf[l] || !a->bl[l])) return hipErrorInvalidValue;
  }
  for (int j = 0; j < a->nadj; ++j)
    if (!a->adj[j].pair) return hipErrorInvalidValue;
  const size_t lds = static_cast<size_t>(a->lds_bytes);
  if (lds > 65536)
    EULER_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gc_infer_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  hipLaunchKernelGGL(gc_infer_kernel, dim3(static_cast<uint32_t>(a->npacks)), dim3(kGcThreads), lds, s, *a);
  return hipGetLastError();
}

}  // extern "C"
