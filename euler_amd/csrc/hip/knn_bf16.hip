// k-nearest-neighbour search over bf16 tables, searched in place: no fp32 copy of the table
// exists at any point.  Ranking key, ordering rule and partial format are those of knn.hip
// (s = ||x||^2 - 2 q.x, ascending (s, original row), sorted partials dist [nq, S, k] fp32 /
// row [nq, S, k] int64 with +inf / -1), so knn_merge serves both.  A product of two bf16
// values is exact in fp32 and every sum here is fp32.
//
//   knn_flat_scan_bf16  one block (4 waves) per (query tile of TQ, row range of X); a tile is
//     128 rows of X.  Dot products are v_mfma_f32_32x32x16_bf16 with X as the A operand and Q
//     as the B operand: lane l supplies A[i = l & 31][k = 8 (l >> 5) .. + 7] and
//     B[k = 8 (l >> 5) .. + 7][j = l & 31] (one 16-byte LDS read each) and holds C column
//     j = l & 31, rows i = (r & 3) + 8 (r >> 2) + 4 (l >> 5).  So a lane holds 16 rows of X
//     against ONE query: the threshold test is a lane-local minimum against that query's
//     threshold, in registers.  Only the queries that some lane flagged send their scores
//     through LDS (64 rows at a time, two halves per tile), where the query's owner wave
//     rescans them and inserts into the sorted k-best list (knn_wave_select).  Once the lists
//     are warm few queries are flagged per half tile, so the score traffic the fp32 kernel
//     pays for every tile is paid for those only.
//     A wave covers 64 queries (two B fragments): TQ = 128 is 2 x 2 waves of 64 queries x 64
//     rows (four accumulators, 2 MFMAs per fragment read), TQ = 64 is 1 x 4 waves of 64
//     queries x 32 rows.  The launcher picks TQ from k, as the lists take TQ * k * 8 bytes.
//     Operands are staged through LDS in chunks of 64 columns of d, zero-padded past d; the
//     next chunk's (or the next tile's first chunk's) global loads are in flight under the
//     current chunk's MFMAs.  The score half tile aliases the staging buffer, which is dead
//     between a tile's last MFMA and the next tile's first store.
//     LDS banks: the staging row stride is 72 halfwords = 144 bytes.  A 16-byte fragment read
//     is served 16 lanes at a time; those lanes read 16 consecutive rows at one column
//     offset, at byte offsets 144 r mod 256 = 16 (9 r mod 16), and r -> 9 r mod 16 is a
//     bijection, so the 16 reads cover the 64 banks once: conflict-free.  The same holds for
//     the 16-byte staging stores (8 lanes fill a row's 128 bytes, the next row starts 144
//     bytes on).  The score rows have stride 65 floats: the writes (one query per lane) go to
//     32 distinct banks per half wave, the owner's reads are contiguous.
//   knn_ivf_scan_bf16   one wave per (query, probed list).  G lanes share a row (G the power
//     of two at or above d / 8, at most 64), each with 16-byte loads of 8 bf16, so a wave
//     reads 64 / G rows per load instruction (4 at d = 128); fp32 FMAs, a butterfly over the
//     G lanes, then the list insertion of 64 rows at a time.
//   knn_row_norms_bf16  xn[i] = sum_c x[i, c]^2 in fp32, the same lane grouping, grid-strided.
// Rows that are not 16-byte aligned (d % 8 != 0 or an unaligned base) take scalar loads.
#include "hip/common.h"
#include "hip/knn_dev.h"
#include "hip/launchers.h"

#include <math.h>

namespace euler_hip {

namespace {

constexpr int kBfTR = 128;          // rows of X per tile
constexpr int kBfHR = 64;           // rows per score half tile
constexpr int kBfKC = 64;           // columns of d per LDS chunk
constexpr int kBfLd = kBfKC + 8;    // staging row stride (halfwords)
constexpr int kBfScLd = kBfHR + 1;  // score row stride (floats)

// sum_e q[e] * x_e + acc over the 8 bf16 of v
__device__ __forceinline__ float kb_dot8(const float (&q)[8], uint4_t v, float acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc = fmaf(q[2 * i], __uint_as_float(v[i] << 16), acc);
    acc = fmaf(q[2 * i + 1], __uint_as_float(v[i] & 0xffff0000u), acc);
  }
  return acc;
}

__device__ __forceinline__ void kb_unpack8(uint4_t v, float (&q)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    q[2 * i] = __uint_as_float(v[i] << 16);
    q[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
  }
}

// ---------------------------------------------------------------------------------- flat
// the second launch bound is waves per SIMD: two blocks per CU at TQ = 128 (LDS allows three up to
// k = 13, the registers two), three at TQ = 64
template <int TQ, bool VEC>
__global__ __launch_bounds__(kKnnThreads, TQ == 128 ? 2 : 3) void knn_flat_scan_bf16_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ X, const float* __restrict__ xn, int64_t nq, int64_t n,
    int d, int k, int S, int64_t tiles_per_split, int64_t items, float* __restrict__ pd, int64_t* __restrict__ pr) {
  constexpr int NWQ = TQ / 64;  // waves along the queries, 64 queries each
  constexpr int NWR = 4 / NWQ;  // waves along the rows
  constexpr int NB = 4 / NWR;   // 32-row blocks of the tile per wave: block b * NWR + wr
  constexpr int NU = (TQ + kBfTR) * (kBfKC / 8) / kKnnThreads;  // staged 16-byte units per thread and chunk
  extern __shared__ __align__(16) unsigned char knnb_smem[];
  bf16_t* Qs = reinterpret_cast<bf16_t*>(knnb_smem);  // [TQ][kBfLd]
  bf16_t* Xs = Qs + TQ * kBfLd;                        // [128][kBfLd]
  float* sc = reinterpret_cast<float*>(knnb_smem);    // [TQ][kBfScLd], over the staging buffer
  float* xns = reinterpret_cast<float*>(Xs + kBfTR * kBfLd);  // [128], +inf past n
  const KnnSel<TQ, 2> st(xns + kBfTR, k);              // a flag per query and score half tile
  static_assert(TQ * kBfScLd * 4 <= (TQ + kBfTR) * kBfLd * 2, "the score half tile must fit the staging buffer");

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int wq = w % NWQ, wr = w / NWQ;
  const int nchunk = (d + kBfKC - 1) / kBfKC;
  const int64_t ntiles = (n + kBfTR - 1) / kBfTR;
  const int64_t nqt = (nq + TQ - 1) / TQ;
  const float inf = __builtin_inff();

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t qt = item % nqt;
    const int split = static_cast<int>(item / nqt);
    const int64_t q0 = qt * TQ;
    const int64_t t_begin = split * tiles_per_split;
    int64_t t_end = t_begin + tiles_per_split;
    if (t_end > ntiles) t_end = ntiles;
    const int64_t r_begin = t_begin * kBfTR;

    __syncthreads();  // the previous item's lists and state are written out
    st.reset();

    uint4_t stage[NU];
    float stage_xn = 0.f;
    auto load_stage = [&](int64_t tile, int chunk) {
      const int64_t x0 = tile * kBfTR;
      const int k0 = chunk * kBfKC;
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int it = tid + kKnnThreads * i;
        const int row = it >> 3, c = k0 + (it & 7) * 8;
        const bool isq = row < TQ;
        const int64_t g = isq ? q0 + row : x0 + (row - TQ);
        const bool ok = (isq ? g < nq : g < n) && c < d;
        uint4_t v = {0u, 0u, 0u, 0u};
        if (ok) {
          const bf16_t* src = (isq ? Q : X) + g * d + c;
          if (VEC) {
            v = *reinterpret_cast<const uint4_t*>(src);
          } else {
            v = kb_load8_scalar(src, d - c);
          }
        }
        stage[i] = v;
      }
      if (chunk == 0 && tid < kBfTR) stage_xn = x0 + tid < n ? xn[x0 + tid] : inf;
    };
    auto store_stage = [&](int chunk) {
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int it = tid + kKnnThreads * i;
        // Xs follows Qs: rows TQ.. are X rows
        *reinterpret_cast<uint4_t*>(Qs + (it >> 3) * kBfLd + (it & 7) * 8) = stage[i];
      }
      if (chunk == 0 && tid < kBfTR) xns[tid] = stage_xn;
    };

    if (t_begin < t_end) load_stage(t_begin, 0);
    for (int64_t tile = t_begin; tile < t_end; ++tile) {
      const int64_t x0 = tile * kBfTR;
      float16_t acc[2][NB];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

      for (int chunk = 0; chunk < nchunk; ++chunk) {
        __syncthreads();  // the previous chunk's operands (and the previous tile's scores) are consumed
        store_stage(chunk);
        __syncthreads();
        if (chunk + 1 < nchunk) {
          load_stage(tile, chunk + 1);
        } else if (tile + 1 < t_end) {
          load_stage(tile + 1, 0);
        }
        int nks = (d - chunk * kBfKC + 15) / 16;
        if (nks > kBfKC / 16) nks = kBfKC / 16;
        for (int ks = 0; ks < nks; ++ks) {
          uint4_t qf[2], xf[NB];
#pragma unroll
          for (int a = 0; a < 2; ++a)
            qf[a] = *reinterpret_cast<const uint4_t*>(Qs + (wq * 64 + a * 32 + l31) * kBfLd + ks * 16 + 8 * h);
#pragma unroll
          for (int b = 0; b < NB; ++b)
            xf[b] = *reinterpret_cast<const uint4_t*>(Xs + ((b * NWR + wr) * 32 + l31) * kBfLd + ks * 16 + 8 * h);
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[a][b] = knn_mfma_bf16(xf[b], qf[a], acc[a][b]);
        }
      }

      // selection, 64 rows at a time: row block rb = b * NWR + wr belongs to half rb >> 1
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        // a lane's scores of one accumulator are 16 rows against one query (KnnSel::tile_flag)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const int rb = b * NWR + wr;
          const bool mine = NWR == 2 ? b == hf : (wr >> 1) == hf;
          if (mine) st.tile_flag(hf, acc[0][b], acc[1][b], xns + rb * 32, wq * 64 + l31);
        }
        __syncthreads();  // flags are set; at hf = 0 the tile's last fragment reads are done too
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const int rb = b * NWR + wr;
          const bool mine = NWR == 2 ? b == hf : (wr >> 1) == hf;
          if (mine) st.tile_spill(hf, acc[0][b], acc[1][b], xns + rb * 32, wq * 64 + l31, sc + (rb & 1) * 32, kBfScLd);
        }
        __syncthreads();
        const int64_t h0 = x0 + hf * kBfHR;
        st.select(hf, sc, kBfScLd, q0, nq, static_cast<int>(h0 - r_begin), h0, n);
      }
    }

    // write the partial lists of this (query tile, split)
    __syncthreads();
    st.write_back(q0, nq, pd, pr, [&](int ql) { return ((q0 + ql) * S + split) * k; }, KnnRowBase{r_begin});
  }
}

size_t knn_flat_bf16_lds(int tq, int k) {
  return static_cast<size_t>(tq + kBfTR) * kBfLd * 2 + sizeof(float) * kBfTR + knn_sel_bytes(tq, 2, 0, k);
}

// ---------------------------------------------------------------------------------- IVF
// lg = log2 of the lanes that share a row; a wave reads 64 >> lg rows per load instruction
template <bool VEC>
__global__ __launch_bounds__(kKnnThreads) void knn_ivf_scan_bf16_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ XS, const float* __restrict__ xn,
    const int64_t* __restrict__ list_ptr, const int64_t* __restrict__ row_of, const int64_t* __restrict__ probe,
    int64_t nq, int64_t n, int64_t ncent, int nprobe, int d, int k, int lg, float* __restrict__ pd,
    int64_t* __restrict__ pr) {
  extern __shared__ __align__(16) unsigned char knnb_smem[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* ld = reinterpret_cast<float*>(knnb_smem) + static_cast<size_t>(w) * 2 * k;
  int* lo = reinterpret_cast<int*>(ld + k);
  const int G = 1 << lg, RP = 64 >> lg;
  const int li = lane & (G - 1), sg = lane >> lg;
  const int W = VEC ? 8 : 1;  // columns per lane and pass
  const float inf = __builtin_inff();
  const int64_t items = nq * nprobe;
  const int64_t step = static_cast<int64_t>(gridDim.x) * (kKnnThreads / 64);

  for (int64_t item = static_cast<int64_t>(blockIdx.x) * (kKnnThreads / 64) + w; item < items; item += step) {
    const int64_t qi = item / nprobe;
    const int64_t list = probe[item];
    int64_t b = 0, e = 0;
    if (list >= 0 && list < ncent) knn_list_range(list_ptr, list, n, 64, b, e);
    const bf16_t* q = Q + qi * d;
    float qv0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (W * li < d) {
      if (VEC) {
        kb_unpack8(*reinterpret_cast<const uint4_t*>(q + 8 * li), qv0);
      } else {
        qv0[0] = bf2f(q[li]);
      }
    }
    int c = 0, to = INT_MAX;
    float td = inf;
    for (int64_t base = b; base < e; base += 64) {
      const int cnt = e - base < 64 ? static_cast<int>(e - base) : 64;
      float mine = 0.f;
      for (int r0 = 0; r0 < cnt; r0 += 4 * RP) {
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        for (int kk = W * li; kk < d; kk += W * G) {
          float qv[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) qv[i] = qv0[i];
          if (kk >= W * G) {
            if (VEC) {
              kb_unpack8(*reinterpret_cast<const uint4_t*>(q + kk), qv);
            } else {
              qv[0] = bf2f(q[kk]);
            }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int r = r0 + u * RP + sg;
            if (r < cnt) {
              const bf16_t* xp = XS + (base + r) * d + kk;
              if (VEC) {
                part[u] = kb_dot8(qv, *reinterpret_cast<const uint4_t*>(xp), part[u]);
              } else {
                part[u] = fmaf(qv[0], bf2f(*xp), part[u]);
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float v = part[u];
          for (int o = G >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o);
          // lane group g holds row r0 + u * RP + g; the lane of that number takes it
          const int rel = lane - r0 - u * RP;
          const float t = __shfl(v, (rel & (RP - 1)) << lg);
          if (rel >= 0 && rel < RP) mine = t;
        }
      }
      const bool valid = lane < cnt;
      const float s = valid ? fmaf(-2.f, mine, xn[base + lane]) : inf;
      knn_wave_select(s, static_cast<int>(base - b) + lane, valid, ld, lo, k, c, td, to);
    }
    knn_write_partial(ld, lo, c, k, pd, pr, item * k, KnnRowOf{row_of, b});
  }
}

// ---------------------------------------------------------------------------------- norms
template <bool VEC>
__global__ __launch_bounds__(kKnnThreads) void knn_row_norms_bf16_kernel(const bf16_t* __restrict__ X, int64_t n, int d,
                                                                         int lg, float* __restrict__ xn) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int G = 1 << lg, RP = 64 >> lg;
  const int li = lane & (G - 1), sg = lane >> lg;
  const int W = VEC ? 8 : 1;
  const int64_t step = static_cast<int64_t>(gridDim.x) * (kKnnThreads / 64) * RP;
  for (int64_t r0 = (static_cast<int64_t>(blockIdx.x) * (kKnnThreads / 64) + w) * RP; r0 < n; r0 += step) {
    const int64_t r = r0 + sg;
    float v = 0.f;
    if (r < n) {
      for (int kk = W * li; kk < d; kk += W * G) {
        const bf16_t* xp = X + r * d + kk;
        if (VEC) {
          float xv[8];
          const uint4_t raw = *reinterpret_cast<const uint4_t*>(xp);
          kb_unpack8(raw, xv);
          v = kb_dot8(xv, raw, v);
        } else {
          const float x = bf2f(*xp);
          v = fmaf(x, x, v);
        }
      }
    }
    for (int o = G >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (r < n && li == 0) xn[r] = v;
  }
}

// log2 of the lanes that share a row: the power of two at or above ceil(d / width), at most 64
int knn_lane_group_log2(int d, int width) {
  const int units = (d + width - 1) / width;
  int lg = 0;
  while (lg < 6 && (1 << lg) < units) ++lg;
  return lg;
}

}  // namespace

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

hipError_t eh_knn_flat_scan_bf16(const uint16_t* Q, const uint16_t* X, const float* xn, int64_t nq, int64_t n, int d,
                                 int k, int S, float* pd, int64_t* pr, hipStream_t s) {
  static const knn_flat_kernel_t<bf16_t> kern[2][2] = {
      {knn_flat_scan_bf16_kernel<64, false>, knn_flat_scan_bf16_kernel<64, true>},
      {knn_flat_scan_bf16_kernel<128, false>, knn_flat_scan_bf16_kernel<128, true>}};
  return knn_flat_launch(kern, kBfTR, 8, knn_flat_bf16_lds, Q, X, xn, nq, n, d, k, S, pd, pr, s);
}

hipError_t eh_knn_ivf_scan_bf16(const uint16_t* Q, const uint16_t* XS, const float* xn, const int64_t* list_ptr,
                                const int64_t* row_of, const int64_t* probe, int64_t nq, int64_t n, int64_t ncent,
                                int nprobe, int d, int k, float* pd, int64_t* pr, hipStream_t s) {
  KnnIvfPlan p;
  EULER_HIP_CHECK(knn_ivf_plan(Q, XS, 8, nq, n, ncent, nprobe, d, k, p));
  const int lg = knn_lane_group_log2(d, p.vec ? 8 : 1);
  hipLaunchKernelGGL(p.vec ? knn_ivf_scan_bf16_kernel<true> : knn_ivf_scan_bf16_kernel<false>, dim3(p.grid),
                     dim3(kKnnThreads), p.lds, s, Q, XS, xn, list_ptr, row_of, probe, nq, n, ncent, nprobe, d, k, lg, pd,
                     pr);
  return hipGetLastError();
}

hipError_t eh_knn_row_norms_bf16(const uint16_t* X, int64_t n, int d, float* xn, hipStream_t s) {
  if (n <= 0 || d < 1) return hipErrorInvalidValue;
  const bool vec = d % 8 == 0 && knn_aligned16(X);
  const int lg = knn_lane_group_log2(d, vec ? 8 : 1);
  const int grid = knn_grid(ceil_div(n, (kKnnThreads / 64) * (64 >> lg)), 1 << 14);
  if (vec)
    hipLaunchKernelGGL(knn_row_norms_bf16_kernel<true>, dim3(grid), dim3(kKnnThreads), 0, s, X, n, d, lg, xn);
  else
    hipLaunchKernelGGL(knn_row_norms_bf16_kernel<false>, dim3(grid), dim3(kKnnThreads), 0, s, X, n, d, lg, xn);
  return hipGetLastError();
}

}  // extern "C"
