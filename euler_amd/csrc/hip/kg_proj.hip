// Projected translation scores (reference examples/TransX/transH.py, transD.py):
//
//   kgp_fwd / kgp_bwd   TransH and TransD scores with the projection done inside the score
//       kernel: entity / relation / projection rows gathered straight from the tables, projected
//       in registers, scored in L1 or L2, and in the backward pushed back through the projection
//       and the normalisations into the fp32 table gradients by atomics.
//
//   model 0, TransH (q = hyper[rel], r = rel[rel]):
//       w = q / max(|q|, 1e-12)     P(x) = x - (w . x) w      (entity rows are not normalised)
//       score = -| P(h) + r / max(|r|, 1e-12) - P(t) |
//   model 1, TransD (x_p = ent_t[x], r_p = rel_t[rel]):
//       y = x + (x . x_p) r_p       x_perp = y / max(|y|, 1e-12)
//       score = -| h_perp + r / max(|r|, 1e-12) - t_perp |
//
// Work split as kg_fwd (embed.hip): one group of lp lanes per triple, 4 columns per lane, every
// row reduction a butterfly inside the group, no LDS.  What is specific to these models:
//   * per-triple work is hoisted: w (normalised once) or r_p, the normalised r, and the
//     projections of h and t are computed once per triple; every negative is projected ONCE and
//     that projection serves its front and its tail score (K + 2 projections per triple, not
//     2 (1 + 2K));
//   * the backward keeps the gradient of each projected row in registers over every score the
//     row takes part in (h_perp and t_perp: up to 1 + K scores) and pushes it through the
//     projection once per entity row; the gradients of w, r_p and the normalised r are summed
//     in registers over the whole triple, pushed through their normalisation once and flushed
//     with one set of atomics per triple and table;
//   * the L2 backward takes |d| from the forward's scores instead of reducing it again.
#include "hip/common.h"
#include "hip/kg_dev.h"
#include "hip/launchers.h"

namespace euler_hip {

// corrupt: 0 front (neg replaces src), 1 tail (neg replaces dst), 2 both (front scores, then
// tail scores).  kind: 0 L1, 1 L2.  Tables fp32 [*, D]; proj_e is indexed like ent (TransD's
// entity_transfer; unused by TransH), proj_r like rel (TransH's hyper, TransD's relation_transfer).
// src / dst / neg index the n_ent entity rows, ridx the n_rel relation rows (kgp_row).
struct KgpArgs {
  const float* ent;
  const float* rel;
  const float* proj_e;
  const float* proj_r;
  const int64_t* src;
  const int64_t* dst;
  const int64_t* ridx;
  const int64_t* neg;
  int64_t B, n_ent, n_rel;
  int K, D, kind, corrupt, lp;
};

// one entity row through the projection: x its raw columns, xp its transfer row (TransD),
// s = w . x (TransH) or x . x_p (TransD), y the projected row, ny = |x + s r_p| (TransD; else 1)
struct KgpRow {
  float x[4], xp[4], y[4], s, ny;
};

// q: this triple's w (TransH, normalised) or r_p (TransD)
template <int M>
__device__ __forceinline__ void kgp_project(const KgpArgs& a, int64_t row, int sub, const float* q, KgpRow& e) {
  float one;
  kg_load_norm(a.ent, row, sub, a.D, a.lp, false, e.x, one);
  float p = 0.f;
  if (M == 0) {
#pragma unroll
    for (int v = 0; v < 4; ++v) p += q[v] * e.x[v];
    e.s = emb_group_sum(p, a.lp);
#pragma unroll
    for (int v = 0; v < 4; ++v) e.y[v] = e.x[v] - e.s * q[v];
    e.ny = 1.f;
  } else {
    kg_load_norm(a.proj_e, row, sub, a.D, a.lp, false, e.xp, one);
#pragma unroll
    for (int v = 0; v < 4; ++v) p += e.x[v] * e.xp[v];
    e.s = emb_group_sum(p, a.lp);
    float n2 = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      e.y[v] = e.x[v] + e.s * q[v];
      n2 += e.y[v] * e.y[v];
    }
    e.ny = fmaxf(sqrtf(emb_group_sum(n2, a.lp)), 1e-12f);
#pragma unroll
    for (int v = 0; v < 4; ++v) e.y[v] /= e.ny;
  }
}

// the triple-shared rows: q = w (TransH: hyper row, normalised, nq its norm) or r_p (TransD: raw,
// nq = 1), r = the normalised relation row, nr its norm
template <int M>
__device__ __forceinline__ void kgp_load_rel(const KgpArgs& a, int64_t rs, int sub, float* q, float& nq, float* r,
                                             float& nr) {
  kg_load_norm(a.proj_r, rs, sub, a.D, a.lp, M == 0, q, nq);
  kg_load_norm(a.rel, rs, sub, a.D, a.lp, true, r, nr);
}

template <int M>
__global__ __launch_bounds__(256) void kgp_fwd_kernel(KgpArgs a, float* __restrict__ pos_score,
                                                      float* __restrict__ neg_score) {
  const RowLane L = row_lane(a.lp, a.B);
  if (!L.ok) return;  // whole lane groups exit together
  float q[4], r[4], nq, nr;
  kgp_load_rel<M>(a, kgp_row(a.ridx[L.row], a.n_rel), L.sub, q, nq, r, nr);
  KgpRow h, t, n;
  kgp_project<M>(a, kgp_row(a.src[L.row], a.n_ent), L.sub, q, h);
  kgp_project<M>(a, kgp_row(a.dst[L.row], a.n_ent), L.sub, q, t);
  const float ps = kg_finish(a.kind, emb_group_sum(kg_part(a.kind, h.y, r, t.y), a.lp));
  if (L.sub == 0) pos_score[L.row] = ps;
  const int nneg = a.corrupt == 2 ? 2 * a.K : a.K;
  for (int k = 0; k < a.K; ++k) {
    kgp_project<M>(a, kgp_row(a.neg[L.row * a.K + k], a.n_ent), L.sub, q, n);
    // the two scores of a negative are independent butterflies over one projection
    const float pf = a.corrupt != 1 ? kg_part(a.kind, n.y, r, t.y) : 0.f;
    const float pt = a.corrupt != 0 ? kg_part(a.kind, h.y, r, n.y) : 0.f;
    if (a.corrupt != 1) {  // front
      const float s = kg_finish(a.kind, emb_group_sum(pf, a.lp));
      if (L.sub == 0) neg_score[L.row * nneg + k] = s;
    }
    if (a.corrupt != 0) {  // tail
      const float s = kg_finish(a.kind, emb_group_sum(pt, a.lp));
      if (L.sub == 0) neg_score[L.row * nneg + (a.corrupt == 2 ? a.K : 0) + k] = s;
    }
  }
}

// d score / d (a, r, b) of score = -|a + r - b| with upstream g, accumulated into da, dr, db;
// the L2 norm is the forward's own score (no second reduction), 0 gradient below 1e-12 as kg_grad
__device__ __forceinline__ void kgp_grad(int kind, float g, float score, const float* x, const float* r,
                                         const float* y, float* dx, float* dr, float* dy) {
  const float nrm = -score;
  const float coef = kind == 1 ? (nrm > 1e-12f ? 1.f / nrm : 0.f) : 1.f;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float d = x[v] + r[v] - y[v];
    const float gd = -g * (kind == 0 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : d * coef);
    dx[v] += gd;
    dr[v] += gd;
    dy[v] -= gd;
  }
}

// the summed gradient dy of a projected row back through its projection: the entity row's (and
// its transfer row's) table gradient by atomics, the share of q's gradient into the registers dq
template <int M>
__device__ __forceinline__ void kgp_push(const KgpArgs& a, int64_t row, int sub, const float* q, const KgpRow& e,
                                         float* dy, float* dq, float* __restrict__ dent,
                                         float* __restrict__ dproj_e) {
  float p = 0.f;
  if (M == 0) {
    // y = x - (w . x) w:  dx = dy - (w . dy) w,  dw -= (w . dy) x + (w . x) dy
#pragma unroll
    for (int v = 0; v < 4; ++v) p += q[v] * dy[v];
    const float c = emb_group_sum(p, a.lp);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      dq[v] -= c * e.x[v] + e.s * dy[v];
      dy[v] -= c * q[v];
    }
    kg_scatter(dent, row, sub, a.D, a.lp, false, e.y, 1.f, dy);
  } else {
    // x_perp = y / |y|, then y = x + (x . x_p) r_p:
    //   dx = dy + (r_p . dy) x_p,  dx_p = (r_p . dy) x,  dr_p += (x . x_p) dy
#pragma unroll
    for (int v = 0; v < 4; ++v) p += e.y[v] * dy[v];
    const float dot = emb_group_sum(p, a.lp);
    p = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      dy[v] = (dy[v] - e.y[v] * dot) / e.ny;
      p += q[v] * dy[v];
    }
    const float c = emb_group_sum(p, a.lp);
    float dxp[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      dq[v] += e.s * dy[v];
      dxp[v] = c * e.x[v];
      dy[v] += c * e.xp[v];
    }
    kg_scatter(dent, row, sub, a.D, a.lp, false, e.y, 1.f, dy);
    kg_scatter(dproj_e, row, sub, a.D, a.lp, false, e.y, 1.f, dxp);
  }
}

template <int M>
__global__ __launch_bounds__(256) void kgp_bwd_kernel(KgpArgs a, const float* __restrict__ pos_score,
                                                      const float* __restrict__ neg_score,
                                                      const float* __restrict__ gpos, const float* __restrict__ gneg,
                                                      float* __restrict__ dent, float* __restrict__ drel,
                                                      float* __restrict__ dproj_e, float* __restrict__ dproj_r) {
  const RowLane L = row_lane(a.lp, a.B);
  if (!L.ok) return;
  float q[4], r[4], nq, nr;
  const int64_t hs = kgp_row(a.src[L.row], a.n_ent), rs = kgp_row(a.ridx[L.row], a.n_rel),
                ts = kgp_row(a.dst[L.row], a.n_ent);
  kgp_load_rel<M>(a, rs, L.sub, q, nq, r, nr);
  KgpRow h, t, n;
  kgp_project<M>(a, hs, L.sub, q, h);
  kgp_project<M>(a, ts, L.sub, q, t);
  // register accumulators over the whole triple: projected h and t, normalised r, and q
  float dh[4] = {0.f, 0.f, 0.f, 0.f}, dt[4] = {0.f, 0.f, 0.f, 0.f}, dr[4] = {0.f, 0.f, 0.f, 0.f};
  float dq[4] = {0.f, 0.f, 0.f, 0.f};
  kgp_grad(a.kind, gpos[L.row], pos_score[L.row], h.y, r, t.y, dh, dr, dt);
  const int nneg = a.corrupt == 2 ? 2 * a.K : a.K;
  for (int k = 0; k < a.K; ++k) {
    const int64_t ns = kgp_row(a.neg[L.row * a.K + k], a.n_ent);
    kgp_project<M>(a, ns, L.sub, q, n);
    float dn[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.corrupt != 1) {
      const int64_t o = L.row * nneg + k;
      kgp_grad(a.kind, gneg[o], neg_score[o], n.y, r, t.y, dn, dr, dt);
    }
    if (a.corrupt != 0) {
      const int64_t o = L.row * nneg + (a.corrupt == 2 ? a.K : 0) + k;
      kgp_grad(a.kind, gneg[o], neg_score[o], h.y, r, n.y, dh, dr, dn);
    }
    kgp_push<M>(a, ns, L.sub, q, n, dn, dq, dent, dproj_e);
  }
  kgp_push<M>(a, hs, L.sub, q, h, dh, dq, dent, dproj_e);
  kgp_push<M>(a, ts, L.sub, q, t, dt, dq, dent, dproj_e);
  // one flush per triple and relation-indexed table (w's goes through its normalisation here)
  kg_scatter(drel, rs, L.sub, a.D, a.lp, true, r, nr, dr);
  kg_scatter(dproj_r, rs, L.sub, a.D, a.lp, M == 0, q, nq, dq);
}

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

static bool kgp_args(int model, const float* ent, const float* rel, const float* proj_e, const float* proj_r,
                     int64_t n_ent, int64_t n_rel, const int64_t* src, const int64_t* dst, const int64_t* ridx,
                     const int64_t* neg, int64_t B, int K, int D, int kind, int corrupt, KgpArgs* a) {
  if (D % 4 != 0 || D < 4 || D > 256 || K < 0 || kind < 0 || kind > 1 || corrupt < 0 || corrupt > 2 || model < 0 ||
      model > 1 || n_ent < 1 || n_rel < 1)
    return false;
  if (!ent || !rel || !proj_r || (model == 1 && !proj_e) || !src || !dst || !ridx || (K > 0 && !neg)) return false;
  a->ent = ent;
  a->rel = rel;
  a->proj_e = proj_e;
  a->proj_r = proj_r;
  a->src = src;
  a->dst = dst;
  a->ridx = ridx;
  a->neg = neg;
  a->B = B;
  a->n_ent = n_ent;
  a->n_rel = n_rel;
  a->K = K;
  a->D = D;
  a->kind = kind;
  a->corrupt = corrupt;
  a->lp = row_lanes(D / 4);
  return true;
}

hipError_t eh_kgp_fwd(int model, const float* ent, const float* rel, const float* proj_e, const float* proj_r,
                      int64_t n_ent, int64_t n_rel, const int64_t* src, const int64_t* dst, const int64_t* ridx,
                      const int64_t* neg, int64_t B, int K, int D, int kind, int corrupt, float* pos_score, float* neg_score, hipStream_t s) {
  if (B == 0) return hipSuccess;
  KgpArgs a;
  if (!kgp_args(model, ent, rel, proj_e, proj_r, n_ent, n_rel, src, dst, ridx, neg, B, K, D, kind, corrupt, &a))
    return hipErrorInvalidValue;
  if (model == 0)
    hipLaunchKernelGGL(kgp_fwd_kernel<0>, row_grid(B, a.lp), dim3(256), 0, s, a, pos_score, neg_score);
  else
    hipLaunchKernelGGL(kgp_fwd_kernel<1>, row_grid(B, a.lp), dim3(256), 0, s, a, pos_score, neg_score);
  return hipGetLastError();
}

hipError_t eh_kgp_bwd(int model, const float* ent, const float* rel, const float* proj_e, const float* proj_r,
                      int64_t n_ent, int64_t n_rel, const int64_t* src, const int64_t* dst, const int64_t* ridx,
                      const int64_t* neg, int64_t B, int K, int D, int kind, int corrupt, const float* pos_score, const float* neg_score,
                      const float* gpos, const float* gneg, float* dent, float* drel, float* dproj_e, float* dproj_r,
                      hipStream_t s) {
  if (B == 0) return hipSuccess;
  KgpArgs a;
  if (!kgp_args(model, ent, rel, proj_e, proj_r, n_ent, n_rel, src, dst, ridx, neg, B, K, D, kind, corrupt, &a) || !dent || !drel ||
      !dproj_r || (model == 1 && !dproj_e))
    return hipErrorInvalidValue;
  if (model == 0)
    hipLaunchKernelGGL(kgp_bwd_kernel<0>, row_grid(B, a.lp), dim3(256), 0, s, a, pos_score, neg_score, gpos, gneg,
                       dent, drel, dproj_e, dproj_r);
  else
    hipLaunchKernelGGL(kgp_bwd_kernel<1>, row_grid(B, a.lp), dim3(256), 0, s, a, pos_score, neg_score, gpos, gneg,
                       dent, drel, dproj_e, dproj_r);
  return hipGetLastError();
}

}  // extern "C"
