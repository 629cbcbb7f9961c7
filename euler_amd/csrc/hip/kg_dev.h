// Device helpers shared by the row-group kernels of embed.hip (sgns_*, kg_fwd / kg_bwd, kg_step) and
// kg_proj.hip (kgp_fwd / kgp_bwd): one row per group of lp lanes, 4 fp32 / 8 bf16 columns per
// lane, row reductions as xor butterflies inside the group.  One copy, included by both, and by
// kg_transr.hip (kgr_fwd / kgr_bwd) for the score conventions and the group reductions.
#pragma once

#include "hip/common.h"

namespace euler_hip {

template <typename T>
struct EV;
template <>
struct EV<bf16_t> {
  static constexpr int N = 8;
  __device__ __forceinline__ static void load(const bf16_t* p, float* f) {
    const uint4_t u = *reinterpret_cast<const uint4_t*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(u[i] << 16);
      f[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  }
  __device__ __forceinline__ static void store(bf16_t* p, const float* f) {
    *reinterpret_cast<uint4_t*>(p) = pack_bf16x8(f);
  }
};
template <>
struct EV<float> {
  static constexpr int N = 4;
  __device__ __forceinline__ static void load(const float* p, float* f) {
    const float4_t u = *reinterpret_cast<const float4_t*>(p);
    f[0] = u[0];
    f[1] = u[1];
    f[2] = u[2];
    f[3] = u[3];
  }
  __device__ __forceinline__ static void store(float* p, const float* f) {
    *reinterpret_cast<float4_t*>(p) = float4_t{f[0], f[1], f[2], f[3]};
  }
};

// sum over aligned groups of g lanes; all lanes of a group follow the same path
__device__ __forceinline__ float emb_group_sum(float v, int g) {
  for (int o = g >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct RowLane {
  int64_t row;
  int sub;
  bool ok;
};
__device__ __forceinline__ RowLane row_lane(int lp, int64_t rows) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  RowLane r;
  r.row = wave * (64 / lp) + lane / lp;
  r.sub = lane & (lp - 1);
  r.ok = r.row < rows;
  return r;
}

// kg_proj.hip, kg_transr.hip: an id outside its table addresses the table's last row
// (utils/layers.py Embedding._rows: the padding row), so the caller needs no clamping pass and no
// id can leave the table
__device__ __forceinline__ int64_t kgp_row(int64_t id, int64_t n) { return id < 0 || id >= n ? n - 1 : id; }

// this lane's 4 columns of table row `row` (zeros outside the width or for row < 0), divided by
// the row's l2 norm (clamped at 1e-12) when `normalize`; nrm = that norm, 1 otherwise
__device__ __forceinline__ void kg_load_norm(const float* tab, int64_t row, int sub, int D, int lp, bool normalize,
                                             float* x, float& nrm) {
  float part = 0.f;
#pragma unroll
  for (int v = 0; v < 4; ++v) x[v] = 0.f;
  if (sub * 4 < D && row >= 0) {
    EV<float>::load(tab + row * D + sub * 4, x);
#pragma unroll
    for (int v = 0; v < 4; ++v) part += x[v] * x[v];
  }
  nrm = 1.f;
  if (normalize) {
    nrm = fmaxf(sqrtf(emb_group_sum(part, lp)), 1e-12f);
#pragma unroll
    for (int v = 0; v < 4; ++v) x[v] /= nrm;
  }
}

// score kinds: 0 TransE-L1, 1 TransE-L2, 2 DistMult
// this lane's part of a score; the caller reduces over the group
__device__ __forceinline__ float kg_part(int kind, const float* h, const float* r, const float* t) {
  float p = 0.f;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    if (kind == 2) {
      p += h[v] * r[v] * t[v];
    } else {
      const float d = h[v] + r[v] - t[v];
      p += kind == 0 ? fabsf(d) : d * d;
    }
  }
  return p;
}

__device__ __forceinline__ float kg_finish(int kind, float s) {
  return kind == 0 ? -s : (kind == 1 ? -sqrtf(s) : s);
}

// push the gradient w.r.t. a normalised row through x / |x| and add it to the table grad
// (occ: store it as occurrence row ``row`` instead — summed per table row afterwards by a
// segment reduction, no atomics on hot rows)
__device__ __forceinline__ void kg_scatter(float* __restrict__ dtab, int64_t row, int sub, int D, int lp,
                                           bool normalize, const float* xhat, float nrm, float* dx, bool occ = false) {
  if (normalize) {
    float p = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) p += xhat[v] * dx[v];
    const float dot = emb_group_sum(p, lp);
#pragma unroll
    for (int v = 0; v < 4; ++v) dx[v] = (dx[v] - xhat[v] * dot) / nrm;
  }
  if (sub * 4 < D && row >= 0) {
    if (occ) {
      EV<float>::store(dtab + row * D + sub * 4, dx);
      return;
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) atomicAdd(dtab + row * D + sub * 4 + v, dx[v]);
  }
}

// launch shape of a row-group kernel: lanes per row (a power of two covering `chunks` 4-column
// chunks) and 256-thread blocks of 64 / lp rows per wave
inline int row_lanes(int chunks) {
  int lp = 1;
  while (lp < chunks && lp < 64) lp <<= 1;
  return lp;
}
inline dim3 row_grid(int64_t rows, int lp) {
  const int64_t rpw = 64 / lp;
  const int64_t waves = (rows + rpw - 1) / rpw;
  return dim3(static_cast<uint32_t>((waves + 3) / 4));
}

}  // namespace euler_hip
