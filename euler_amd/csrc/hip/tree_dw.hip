// The weight-gradient and optimizer launches of the fused GraphSAGE tree step (overview:
// tree_fwd.hip): tr_dw_all_kernel (every dW of the step: the routed bodies, the stored-G plain
// and fold bodies and, fused, the optimizer in trailing blocks) and tr_opt_kernel (split-K
// reduce + optimizer + bf16 shadows, with the next step's sampler and gather tiles as extra
// blocks).  Both run the one optimizer tile, tr_opt_tile.  The host half of the planning is
// tree_plan.h.
#include "hip/tree_dev.h"
#include "hip/tree_plan.h"

namespace euler_hip {

// ----------------------------------------------------------------------------
// tr_dw: grouped split-K weight gradients, part[s][p][q] = sum_{m in split s} G[m][p] X[m][q];
// 64x64 tiles, 4 waves of 32x32
// ----------------------------------------------------------------------------
// raw operands of a route problem's G^T fragment (rows mb*32 + lk .. +7, column p): the
// ReLU bits and the parent's self / neighbour gradients
struct RouteRaw {
  uint32_t bits;
  float ds, dn;
};

__device__ __forceinline__ RouteRaw tr_route_load(const TrDwProb& pr, int mb, int p, int lk) {
  const int64_t m0 = static_cast<int64_t>(mb) * 32 + lk;
  const float* row = pr.dA + (m0 >> pr.logPg) * 2 * pr.P;
  RouteRaw r;
  r.bits = pr.mask[static_cast<int64_t>(mb) * pr.P + p] >> lk;
  r.ds = row[p];
  r.dn = row[pr.P + p];
  return r;
}

// G[m][p] for the 8 rows: neighbour slots (j < Fg) get dn / (Fg + self), the self slot
// ds (+ the neighbour share with self loops), padding 0, all masked by the ReLU bits
__device__ __forceinline__ uint4_t tr_route_frag(const TrDwProb& pr, const RouteRaw& r, int mb, int lk) {
  const int j0 = static_cast<int>((static_cast<int64_t>(mb) * 32 + lk) & ((int64_t(1) << pr.logPg) - 1));
  const float dn = r.dn * pr.inv;
  const float ds = r.ds + (pr.include_self ? dn : 0.f);
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = j0 + i;
    const float val = j < pr.Fg ? dn : (j == pr.Fg ? ds : 0.f);
    v[i] = ((r.bits >> i) & 1u) ? val : 0.f;
  }
  return pack_bf16x8(v);
}

// the same fragment with a handful of instructions (the select chain above costs ~77 VALU
// per fragment and made the routed dW issue-bound): which of the 8 rows are neighbour /
// self slots is two 8-bit masks of j0, the ReLU bits pick rows, and `lut` (256 entries,
// LDS) spreads an 8-bit row set into the 0xffff halves of 4 words; the values are the
// bf16 pair of dn (resp. ds), rounded exactly like pack_bf16x8.
// In two halves, so that a caller can put other work between the table reads and their use:
// the spread row sets of the neighbour and the self slots (b8: the ReLU bits of the 8 rows,
// dF = Fg - j0, j0 the slot of the fragment's first row within its sibling group) ...
struct RouteSpread {
  uint4_t n, s;
};
__device__ __forceinline__ RouteSpread tr_route_spread(uint32_t b8, int dF, const uint4_t* lut) {
  const uint32_t nm = dF >= 8 ? 0xffu : (dF <= 0 ? 0u : ((1u << dF) - 1u));
  const uint32_t sm = (dF >= 0 && dF < 8) ? (1u << dF) : 0u;
  return RouteSpread{lut[b8 & nm], lut[b8 & sm]};
}
// ... and the values laid over them
__device__ __forceinline__ uint4_t tr_route_combine(const TrDwProb& pr, const RouteRaw& r, const RouteSpread& m) {
  const float dn = r.dn * pr.inv;
  const float ds = r.ds + (pr.include_self ? dn : 0.f);
  const uint32_t DN = pack_bf16x2(dn, dn), DS = pack_bf16x2(ds, ds);
  uint4_t out;
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = (DN & m.n[i]) | (DS & m.s[i]);
  return out;
}

__device__ __forceinline__ uint4_t tr_route_frag_lut(const TrDwProb& pr, const RouteRaw& r, int mb, int lk,
                                                     const uint4_t* lut) {
  const int j0 = static_cast<int>((static_cast<int64_t>(mb) * 32 + lk) & ((int64_t(1) << pr.logPg) - 1));
  return tr_route_combine(pr, r, tr_route_spread(r.bits & 0xffu, pr.Fg - j0, lut));
}

// lut[b] word i = (bit 2i of b ? 0x0000ffff : 0) | (bit 2i + 1 ? 0xffff0000 : 0); one entry
// per thread of a 256-thread block (the caller synchronises before the first use)
__device__ __forceinline__ void tr_spread_lut_init(uint4_t* lut) {
  if (threadIdx.x < 256) {
    const uint32_t b = threadIdx.x;
    uint4_t w;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (((b >> (2 * i)) & 1u) ? 0x0000ffffu : 0u) | (((b >> (2 * i + 1)) & 1u) ? 0xffff0000u : 0u);
    lut[b] = w;
  }
}

// ----------------------------------------------------------------------------
// tr_dw_route: split-K dW of a layer whose output gradient is routed from the parent
// rows (the tree mean's backward). Workgroup tile 64 p x 128 q; per stage of kRKB
// k-blocks every thread builds one G^T fragment lane per k-block (p = tid & 63, 8 rows)
// into LDS, so each routed element is built once per q tile; wave w multiplies all 64 p
// rows by its 32 q columns with X fragments loaded straight from the kt layout, one
// stage (kRKB k-blocks) ahead.
// ----------------------------------------------------------------------------
#ifndef TR_RKB
#define TR_RKB 8
#endif
// kRKB k-blocks per stage; the double-buffered G tile takes 2 * kRKB * 4 KiB of LDS.
// G^T tile [64 p][32 rows], 16-B chunks swizzled (rt_off, 4 chunks per row): the MFMA
// fragment reads and the builder's stores (lanes 4i..4i+3 = the 4 chunks of p-row i, so
// an 8-lane store group covers two whole rows) are bank-conflict-free
constexpr int kRP = 64, kRQ = 128, kRKB = TR_RKB, kRLd = 32;

struct RouteStage {
  RouteRaw r[kRKB];
  uint4_t x[kRKB][2];
};

typedef bf16_t RouteLds[2][kRKB][kRP * kRLd];

// element (r, col) of a G^T tile [64 p][32 k] (4 chunks per row, no padding): chunk c of row r
// at c ^ ((r >> 2) & 2) — conflict-free for the fragment reads and for 8-lane store groups
// that cover two whole rows (rows sharing a slot quad get distinct masks)
__device__ __forceinline__ int rt_off(int r, int col) { return r * 32 + ((((col >> 3) ^ ((r >> 2) & 2))) << 3) + (col & 7); }

// The slab tile of one wave of a routed block, and the hand-off to the trailing optimizer blocks
// of a fused launch (ready != nullptr: the tile's counter).  Fused: the slab goes out as
// agent-scope relaxed atomic stores (write-through, nothing left dirty in this XCD's L2; staging
// the tile in LDS for 16-B stores measured 0.15 us slower, profiles/dw_opt_fuse/README.md), every
// wave waits for its own stores, and behind the workgroup barrier one lane adds 1 to the counter
// of the 64 x 128 tile: the add comes after the wait of every wave it signals for.  Waves past Q
// (qok false) store nothing and join the barrier.
__device__ __forceinline__ void tr_route_store(const float4_t (&acc)[4][2], float* out, int Q, bool qok,
                                               uint32_t* ready) {
  const int lane = threadIdx.x & 63, lr = lane & 15;
  if (!ready) {
    if (!qok) return;
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int fn = 0; fn < 2; ++fn)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) out[(fm * 16 + (lane >> 4) * 4 + jj) * Q + fn * 16 + lr] = acc[fm][fn][jj];
    return;
  }
  if (qok) {
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int fn = 0; fn < 2; ++fn)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          __hip_atomic_store(&out[(fm * 16 + (lane >> 4) * 4 + jj) * Q + fn * 16 + lr], acc[fm][fn][jj],
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(ready, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void tr_dw_route_body(const TrDwProb& pr, int b, RouteLds& gs, const uint4_t* lut,
                                                 long long* prof, uint32_t* ready) {
  TR_STAMP(prof, static_cast<int64_t>(b), 0);
  // XCD-aware: the tiles of one split (which read the same X rows) share b % 8
  const int j = b >> 3;
  const int tile = j % pr.ntiles;
  const int s = (j / pr.ntiles) * 8 + (b & 7);
  const int tp = tile / pr.tiles_q, tq = tile - tp * pr.tiles_q;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const int bpl = tid >> 2, blk = (tid & 3) * 8;  // builder: column p = bpl, rows blk..+7
  const int bp = tp * kRP + bpl;
  const int wq = tq * kRQ + wave * 32;                           // MFMA: columns wq..+31, all 64 rows
  const int64_t Q = pr.Q;
  const bool qok = wq < Q;  // uniform
  const int mb0 = s * pr.kps;
  const int mb1 = (mb0 + pr.kps) < pr.MB ? (mb0 + pr.kps) : pr.MB;
  float4_t acc[4][2];
  tl_zero(acc);
  if (mb0 < mb1) {
    auto load = [&](RouteStage& st, int mbs) {
#pragma unroll
      for (int u = 0; u < kRKB; ++u) {
        const int mb = (mbs + u) < mb1 ? (mbs + u) : (mb1 - 1);  // clamped: always a valid row
        st.r[u] = tr_route_load(pr, mb, bp, blk);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const int q = qok ? wq + f * 16 + lr : lr;
          st.x[u][f] = *reinterpret_cast<const uint4_t*>(pr.X + ((static_cast<int64_t>(mb) * Q + q) * 32 + lk));
        }
      }
    };
    auto build = [&](const RouteStage& st, int buf, int mbs) {
#pragma unroll
      for (int u = 0; u < kRKB; ++u) {
        const uint4_t fr = (mbs + u) < mb1 ? tr_route_frag_lut(pr, st.r[u], mbs + u, blk, lut) : uint4_t{0u, 0u, 0u, 0u};
        *reinterpret_cast<uint4_t*>(&gs[buf][u][rt_off(bpl, blk)]) = fr;
      }
    };
    auto compute = [&](const RouteStage& st, int buf, int mbs) {
      if (!qok) return;
#pragma unroll
      for (int u = 0; u < kRKB; ++u) {
        if (mbs + u >= mb1) break;  // uniform
        uint4_t a[4];
#pragma unroll
        for (int fm = 0; fm < 4; ++fm)
          a[fm] = *reinterpret_cast<const uint4_t*>(&gs[buf][u][rt_off(fm * 16 + lr, lk)]);
#pragma unroll
        for (int fn = 0; fn < 2; ++fn)
#pragma unroll
          for (int fm = 0; fm < 4; ++fm) acc[fm][fn] = mfma16(a[fm], st.x[u][fn], acc[fm][fn]);
      }
    };
    RouteStage A, B;
    load(A, mb0);
    int it = 0;
    for (int mbs = mb0; mbs < mb1; mbs += 2 * kRKB) {
      build(A, 0, mbs);
      load(B, mbs + kRKB);
      __syncthreads();
      compute(A, 0, mbs);
      if (mbs + kRKB < mb1) {
        build(B, 1, mbs + kRKB);
        load(A, mbs + 2 * kRKB);
        __syncthreads();
        compute(B, 1, mbs + kRKB);
      }
      ++it;
      if (it < 6) TR_STAMP(prof, static_cast<int64_t>(b), it);
    }
  }
  TR_STAMP(prof, static_cast<int64_t>(b), 7);
  float* out = pr.part + static_cast<int64_t>(s) * pr.P * Q;
  tr_route_store(acc, out + static_cast<int64_t>(tp * kRP) * Q + wq, static_cast<int>(Q), qok,
                 ready ? ready + tile * kTrSyncLine : nullptr);
}

// ----------------------------------------------------------------------------
// tr_dw_route_pipe: tr_dw_route_body with the three phases of a stage (build the G tile, load
// the next operands, multiply) woven into one straight-line block per stage.  Same tile, slabs,
// block mapping, G values and LDS layout; every accumulator gets the same MFMAs in the same k
// order from zero, so the slabs are the same bits.
// One register ring of kRKB k-blocks, refilled in place.  In stage t, at k-block u:
//   - the A fragments of k-block u + 1 are read from this stage's G tile (two register sets),
//   - the G fragment of k-block u of stage t + 1 is built from r[u] and stored to the OTHER tile,
//   - r[u] is reloaded with the raw operands of stage t + 2,
//   - the 8 MFMAs of k-block u run on x[u],
//   - x[u] is reloaded with the X fragments of stage t + 1.
// So every global load has one stage of MFMAs to arrive, and a stage has no phase in which the
// MFMA pipe only waits.  One barrier per stage.  Write after read: the stores of stage t go to
// the tile that stage t - 1 read; a wave reaches the barrier that ends stage t - 1 only after
// its MFMAs of that stage were issued, which wait for the fragment reads they consume, so no
// read of that tile is pending when the first store of stage t is issued.  Read after write:
// __syncthreads() waits for the wave's own LDS stores before the barrier, and the first read
// of stage t + 1 comes after it.
// A stage is branch-free (compile-time counts); the slab's last two stages take the same code
// without the refills that have nothing to fetch, and a last stage of fewer than kRKB k-blocks
// counts its MFMAs at run time (a missing k-block is skipped, not multiplied by zeros).
// Addresses: one 32-bit byte offset per thread and operand, the k-block's base is uniform.
// Waves whose 32 columns lie past Q (Q % 128 == 32 or 64) run on the tile's first columns and
// store nothing: they build their share of G and reach every barrier.
// ----------------------------------------------------------------------------
template <int N>
struct RtCount {
  __device__ constexpr operator int() const { return N; }
};

__device__ __forceinline__ void tr_dw_route_pipe_body(const TrDwProb& pr, int b, RouteLds& gs, uint4_t* lut,
                                                      long long* prof, uint32_t* ready) {
  TR_STAMP(prof, static_cast<int64_t>(b), 0);
  const int j = b >> 3;
  const int tile = j % pr.ntiles;
  const int s = (j / pr.ntiles) * 8 + (b & 7);
  const int tp = tile / pr.tiles_q, tq = tile - tp * pr.tiles_q;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const int bpl = tid >> 2, blk = (tid & 3) * 8;  // builder: column p = bpl, rows blk..+7
  const int bp = tp * kRP + bpl;
  const int wq = tq * kRQ + wave * 32;  // MFMA: columns wq..+31, all 64 rows
  const int Q = pr.Q, P = pr.P;
  const bool qok = wq < Q;  // uniform
  const int mb0 = s * pr.kps;
  const int mb1 = (mb0 + pr.kps) < pr.MB ? (mb0 + pr.kps) : pr.MB;
  // uniform byte strides per k-block and per-thread byte offsets (all below 2^31: one k-block
  // of X is Q * 64 bytes, one dA row 8 P bytes)
  const int sh = 5 - pr.logPg;  // >= 0: a k-block holds 2^sh sibling groups, < 0: a group 2^-sh k-blocks
  const uint32_t xst = static_cast<uint32_t>(Q) * 64u, mst = static_cast<uint32_t>(P) * 4u, dst = static_cast<uint32_t>(P) * 8u;
  const uint32_t xo = static_cast<uint32_t>((((qok ? wq : 0) + lr) * 32 + lk) * 2);
  const uint32_t mo = static_cast<uint32_t>(bp * 4);
  const uint32_t dso = static_cast<uint32_t>(((sh >= 0 ? (blk >> pr.logPg) : 0) * 2 * P + bp) * 4);
  const uint32_t dno = dso + static_cast<uint32_t>(P * 4);
  const uint32_t gmask = (pr.logPg < 31 ? (1u << pr.logPg) : 0u) - 1u;
  const int dFb1 = pr.Fg + 1 - static_cast<int>(static_cast<uint32_t>(blk) & gmask);
  RouteRaw r[kRKB];  // bits: the whole mask word (shifted where it is used, not where it is loaded)
  uint4_t x[kRKB][2];
  // the k-block's base is made opaque in scalar registers and the thread's offset in a vector
  // register, so that the compiler neither folds one into the other nor widens the offset: the
  // loads take the (scalar base, 32-bit vector offset) form and cost no address arithmetic
  typedef const __attribute__((address_space(1))) char* gptr_t;
  auto at = [](const void* base, uint32_t row, uint32_t stride, uint32_t off) __attribute__((always_inline)) {
    uint64_t v = reinterpret_cast<uint64_t>(base) + static_cast<uint64_t>(row) * stride;
    asm("" : "+s"(v));
    asm("" : "+v"(off));
    return (gptr_t)v + off;
  };
  auto load_raw = [&](RouteRaw& d, int mb) __attribute__((always_inline)) {
    const uint32_t row = sh >= 0 ? (static_cast<uint32_t>(mb) << sh) : (static_cast<uint32_t>(mb) >> -sh);
    d.bits = *(const __attribute__((address_space(1))) uint32_t*)at(pr.mask, mb, mst, mo);
    d.ds = *(const __attribute__((address_space(1))) float*)at(pr.dA, row, dst, dso);
    d.dn = *(const __attribute__((address_space(1))) float*)at(pr.dA, row, dst, dno);
  };
  auto load_x = [&](uint4_t (&d)[2], int mb) __attribute__((always_inline)) {
    gptr_t p = at(pr.X, mb, xst, xo);
#pragma unroll
    for (int f = 0; f < 2; ++f) d[f] = *(const __attribute__((address_space(1))) uint4_t*)(p + f * (16 * 32 * 2));
  };
  // tr_route_spread's row sets without its selects: with e = min(max(dF + 1, 0), 9) the low e
  // bits are the neighbour rows and the self row, the low e - 1 bits the neighbour rows
  auto spread = [&](const RouteRaw& d, int mb) __attribute__((always_inline)) {
    const int jm = static_cast<int>((static_cast<uint32_t>(mb) << 5) & gmask);  // uniform; 0 for groups <= 32 rows
    const int e1 = dFb1 - jm, e = e1 < 0 ? 0 : (e1 > 9 ? 9 : e1);
    const uint32_t both = (1u << e) - 1u, nm = both >> 1, b8 = (d.bits >> blk) & 0xffu;
    return RouteSpread{lut[b8 & nm], lut[b8 & (both ^ nm)]};
  };
  float4_t acc[4][2];
  tl_zero(acc);
  if (mb0 < mb1) {
    // prologue: every load of the first two stages goes out before the table is there (clamped:
    // a short slab loads its last k-block again instead of branching).  The first stage's raw
    // operands come first, into registers of their own; the rest in the order a stage issues
    // them (per k-block the raw operands of the stage after next, then X of the next stage), so
    // the first stage finds the load queue as every later stage does.
    RouteRaw r0[kRKB];
#pragma unroll
    for (int u = 0; u < kRKB; ++u) load_raw(r0[u], (mb0 + u) < mb1 ? (mb0 + u) : (mb1 - 1));
#pragma unroll
    for (int u = 0; u < kRKB; ++u) {
      load_raw(r[u], (mb0 + kRKB + u) < mb1 ? (mb0 + kRKB + u) : (mb1 - 1));
      load_x(x[u], (mb0 + u) < mb1 ? (mb0 + u) : (mb1 - 1));
      __builtin_amdgcn_sched_barrier(0);  // in this order
    }
    tr_spread_lut_init(lut);
    __syncthreads();
    const int wr = rt_off(bpl, blk), rd = rt_off(lr, lk);  // rt_off(16 fm + lr, lk) = rd + 16 fm kRLd
#pragma unroll
    for (int u = 0; u < kRKB; ++u) {
      const int mb = (mb0 + u) < mb1 ? (mb0 + u) : (mb1 - 1);
      *reinterpret_cast<uint4_t*>(&gs[0][u][wr]) = tr_route_combine(pr, r0[u], spread(r0[u], mb));
    }
    __syncthreads();
    // one stage: nc k-blocks to multiply, nb k-blocks of the next stage to build (and their X
    // to load), nr k-blocks of the stage after that to load raw.  The table reads of k-block
    // u + 1 go out with the A fragment reads of u + 1, before the MFMAs of u.
    // nb and nr are all or nothing: past the slab's end the last k-block is loaded and built
    // again (the prologue's clamp, one scalar min), so no register is written under a
    // condition; what that builds is never multiplied.  Only the slab's last stage counts its
    // MFMAs at run time, and it builds and loads nothing.
    auto stage = [&](int buf, int mbs, auto nc, auto nb, auto nr) __attribute__((always_inline)) {
      auto kb = [&](int mb) __attribute__((always_inline)) { return mb < mb1 ? mb : mb1 - 1; };
      const bf16_t* gr = &gs[buf][0][rd];
      bf16_t* gw = &gs[buf ^ 1][0][wr];
      uint4_t a[2][4];
      RouteSpread sp[2];
#pragma unroll
      for (int fm = 0; fm < 4; ++fm) a[0][fm] = *reinterpret_cast<const uint4_t*>(gr + fm * 16 * kRLd);
      if (0 < nb) sp[0] = spread(r[0], kb(mbs + kRKB));
#pragma unroll
      for (int u = 0; u < kRKB; ++u) {
        // the LDS reads of k-block u + 1 first, pinned there: left alone, the compiler sinks
        // them down to the MFMAs that use them (one register set less) and every k-block
        // waits for its own reads
        if (u + 1 < kRKB) {
#pragma unroll
          for (int fm = 0; fm < 4; ++fm)
            a[(u + 1) & 1][fm] = *reinterpret_cast<const uint4_t*>(gr + (u + 1) * kRP * kRLd + fm * 16 * kRLd);
        }
        if (u + 1 < kRKB && u + 1 < nb) sp[(u + 1) & 1] = spread(r[(u + 1) % kRKB], kb(mbs + kRKB + u + 1));
        __builtin_amdgcn_sched_barrier(0);
        if (u < nb) *reinterpret_cast<uint4_t*>(gw + u * kRP * kRLd) = tr_route_combine(pr, r[u], sp[u & 1]);
        if (u < nr) load_raw(r[u], kb(mbs + 2 * kRKB + u));
        if (u < nc) {  // uniform
#pragma unroll
          for (int fn = 0; fn < 2; ++fn)
#pragma unroll
            for (int fm = 0; fm < 4; ++fm) acc[fm][fn] = mfma16(a[u & 1][fm], x[u][fn], acc[fm][fn]);
        }
        if (u < nb) load_x(x[u], kb(mbs + kRKB + u));
        // and nothing moves across a k-block: the raw loads would all sink to the stage's
        // end, into fresh registers, and the next stage would wait for them
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // every path below is uniform per block.  Each kind of stage has its own place in the
    // control flow (a loop of stages with two more to come, then the last two written out),
    // and all kinds issue their loads in the same order, so the load-queue depth the compiler
    // counts on at a stage's top is a whole stage.
    int buf = 0, it = 0, mbs = mb0;
    auto next = [&](bool more) __attribute__((always_inline)) {
      if (more) __syncthreads();
      buf ^= 1;
      mbs += kRKB;
      ++it;
      // stamp 1: the prologue's end, stamp k + 1: the end of stage k
      if (it < 6) TR_STAMP(prof, static_cast<int64_t>(b), it + 1);
    };
    TR_STAMP(prof, static_cast<int64_t>(b), 1);
    const RtCount<kRKB> all;
    const RtCount<0> none;
    while (mb1 - mbs > 2 * kRKB) {
      stage(buf, mbs, all, all, all);
      next(true);
    }
    if (mb1 - mbs > kRKB) {
      stage(buf, mbs, all, all, none);
      next(true);
    }
    if (mb1 - mbs == kRKB) stage(buf, mbs, all, none, none);
    else stage(buf, mbs, mb1 - mbs, none, none);
    next(false);
  }
  TR_STAMP(prof, static_cast<int64_t>(b), 7);
  float* out = pr.part + static_cast<int64_t>(s) * pr.P * Q;
  tr_route_store(acc, out + static_cast<int64_t>(tp * kRP) * Q + wq, static_cast<int>(Q), qok,
                 ready ? ready + tile * kTrSyncLine : nullptr);
}

// ----------------------------------------------------------------------------
// tr_dw: grouped split-K dW of the problems with stored G operands (kt layout),
// part[s][p][q] = sum_{m in split s} G[m][p] X[m][q]; 64x64 tiles, 4 waves of 32x32,
// k-block groups double-buffered in registers (unrolled ping-pong: no register copies)
// ----------------------------------------------------------------------------
__device__ __forceinline__ void tr_dw_plain_body(const TrDwProb& pr, int local) {
  const int s = local / pr.ntiles;
  const int tile = local - s * pr.ntiles;
  const int tp = tile / pr.tiles_q, tq = tile - (tile / pr.tiles_q) * pr.tiles_q;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const int p0 = tp * 64 + (wave >> 1) * 32;
  const int q0 = tq * 64 + (wave & 1) * 32;
  const int mb0 = s * pr.kps;
  const int mb1 = (mb0 + pr.kps) < pr.MB ? (mb0 + pr.kps) : pr.MB;
  const int64_t P = pr.P, Q = pr.Q;
  if (p0 >= P || q0 >= Q) return;  // 32-wide edge of a 64-wide tile; no barriers in this body
  float4_t acc[2][2];
  tl_zero(acc);
  constexpr int KB = 4;
  struct Grp {
    uint4_t a[KB][2], b[KB][2];
  };
  auto load = [&](Grp& g, int mbs) {
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      const int64_t mb = (mbs + u) < mb1 ? (mbs + u) : (mb1 - 1);
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        g.a[u][f] = *reinterpret_cast<const uint4_t*>(pr.G + ((mb * P + p0 + f * 16 + lr) * 32 + lk));
        g.b[u][f] = *reinterpret_cast<const uint4_t*>(pr.X + ((mb * Q + q0 + f * 16 + lr) * 32 + lk));
      }
    }
  };
  auto compute = [&](const Grp& g, int mbs) {
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      if (mbs + u >= mb1) break;  // uniform
#pragma unroll
      for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fn = 0; fn < 2; ++fn) acc[fm][fn] = mfma16(g.a[u][fm], g.b[u][fn], acc[fm][fn]);
    }
  };
  if (mb0 < mb1) {
    Grp A, B;
    load(A, mb0);
    for (int mbs = mb0; mbs < mb1; mbs += 2 * KB) {
      load(B, mbs + KB);
      compute(A, mbs);
      if (mbs + KB >= mb1) break;
      load(A, mbs + 2 * KB);
      compute(B, mbs + KB);
    }
  }
  float* out = pr.part + static_cast<int64_t>(s) * P * Q;
#pragma unroll
  for (int fm = 0; fm < 2; ++fm)
#pragma unroll
    for (int fn = 0; fn < 2; ++fn)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        out[(p0 + fm * 16 + (lane >> 4) * 4 + j) * Q + q0 + fn * 16 + lr] = acc[fm][fn][j];
}

// ----------------------------------------------------------------------------
// tr_dw_fold: a stored-G problem whose F split-K slabs are summed inside the block.  One
// workgroup owns one 32x32 tile over all of K; wave w computes the slabs w, w + 4, ... one
// after the other, each exactly as tr_dw_plain_body computes it (accumulators zeroed per
// slab, the same MFMAs in k order, the same clamped loads), and parks each finished slab in
// LDS slot s.  After the barrier the 256 threads add the slots in slab order, which is the
// sum tr_opt made of the slabs in `part`: the same adds on the same operands, so the same
// bits, and the slabs never travel through memory.  The k-block groups of all the wave's slabs
// form one ping-pong sequence: the next group's loads (the next slab's, at a slab's end) are
// issued before this group's MFMAs.
// Slot layout [32 rows][32 cols] fp32 with the 16-column halves swapped in rows with bit 2 set
// (tr_fold_off).  An accumulator store (ds_write_b32, 32-lane groups) writes 16 columns of
// rows r and r + 4: the swap puts them on the two halves of the 32 banks.  The fold reads 16 B
// per thread, 8 threads per row; a 16-lane group of ds_read_b128 covers 4 rows x 16 columns
// that lie on 64 distinct banks with or without the swap (bit 2 is equal within 4 rows).
// ----------------------------------------------------------------------------
// One parameter's optimizer update from its summed gradient g, shared by the optimizer launch
// (tr_opt_tile) and the blocks of a fused dW launch.
__device__ __forceinline__ void tr_opt_update(const TrOptCore& a, float g, float& p, float& m, float& v) {
  // Which multiply-add pairs are fused is written out (fmaf) and nothing else may be contracted:
  // left to the compiler the choice follows the surrounding code, and the two callers would
  // round differently.  These are the roundings the optimizer launch has always made.
#pragma clang fp contract(off)
  const float t = static_cast<float>(a.step[0]);
  const float gi = fmaf(a.wd, p, g * a.grad_scale);
  float d;
  if (a.kind == 0) {
    const float bc1 = 1.f - __powf(a.b1, t), bc2 = 1.f - __powf(a.b2, t);
    m = fmaf(a.b1, m, (1.f - a.b1) * gi);
    v = fmaf(a.b2, v, (1.f - a.b2) * gi * gi);
    d = a.lr * (m / bc1) / (sqrtf(v / bc2) + a.eps);
  } else if (a.kind == 1) {
    v = fmaf(gi, gi, v);
    d = a.lr * gi / (sqrtf(v) + a.eps);
  } else if (a.kind == 2) {
    d = a.lr * gi;
  } else {
    m = fmaf(a.b1, m, gi);
    d = a.lr * m;
  }
  p -= d;
}

// bf16 shadows of the 8 x 32 weight tile at (r0, c0), staged in tile_s (written and barriered by
// the caller), by the 64 threads t = 0..63: rows as 16-B fm chunks (t < 32), columns of the
// transpose (t >= 32, where shT is set)
__device__ __forceinline__ void tr_opt_shadow(uint16_t* sh, uint16_t* shT, int rows, int cols, int r0, int c0,
                                              const float (*tile_s)[33], int t) {
  if (t < 32) {
    const int row = t >> 2, kc = (t & 3) * 8;
    float t8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t8[k] = tile_s[row][kc + k];
    *reinterpret_cast<uint4_t*>(sh + fm_off(r0 + row, c0 + kc, cols)) = pack_bf16x8(t8);
  } else if (t < 64 && shT) {
    const int col = t - 32;
    float t8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t8[k] = tile_s[k][col];
    *reinterpret_cast<uint4_t*>(shT + fm_off(c0 + col, r0, rows)) = pack_bf16x8(t8);
  }
}

static_assert(sizeof(RouteLds) >= kTrFoldLds, "the fold's slots alias the routed body's G tile");
static_assert(kTrFoldLds >= 32 * 33 * 4, "the fused fold stages its 32 x 32 tile in the slots");
__device__ __forceinline__ int tr_fold_off(int row, int col) { return row * 32 + (col ^ ((row & 4) << 2)); }

// fuse (a fused launch; fz: the problem's flat segment): the block applies the optimizer to its tile instead of storing
// the `part` slab: the sum below is the S == 1 gradient tr_opt_tile<2> would read back, and the
// update and the shadow writes are the code it runs (tr_opt_update, tr_opt_shadow).
__device__ __forceinline__ void tr_dw_fold_body(const TrDwProb& pr, int tile, float* slots, const TrDwOpt& o,
                                                const TrFoldSeg& fz, bool fuse) {
  const int tp = tile / pr.tiles_q, tq = tile - tp * pr.tiles_q;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const int p0 = tp * 32, q0 = tq * 32;
  const int64_t P = pr.P, Q = pr.Q;
  const int F = pr.F, MB = pr.MB, kps = pr.kps;
  constexpr int KB = 4;
  struct Grp {
    uint4_t a[KB][2], b[KB][2];
  };
  // k-blocks [m0, m1) of slab sl (empty past MB: that slab is all zeros)
  auto slab = [&](int sl, int& m0, int& m1) {
    m0 = sl * kps < MB ? sl * kps : MB;
    m1 = (m0 + kps) < MB ? (m0 + kps) : MB;
  };
  auto load = [&](Grp& g, int sl, int mbs, int mb1) {
    if (sl >= F || mbs >= mb1) return;  // uniform per wave
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      const int64_t mb = (mbs + u) < mb1 ? (mbs + u) : (mb1 - 1);
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        g.a[u][f] = *reinterpret_cast<const uint4_t*>(pr.G + ((mb * P + p0 + f * 16 + lr) * 32 + lk));
        g.b[u][f] = *reinterpret_cast<const uint4_t*>(pr.X + ((mb * Q + q0 + f * 16 + lr) * 32 + lk));
      }
    }
  };
  float4_t acc[2][2];
  tl_zero(acc);
  auto compute = [&](const Grp& g, int mbs, int mb1) {
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      if (mbs + u >= mb1) break;  // uniform
#pragma unroll
      for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fn = 0; fn < 2; ++fn) acc[fm][fn] = mfma16(g.a[u][fm], g.b[u][fn], acc[fm][fn]);
    }
  };
  // the wave's position: slab s, its k-blocks from mbs on, the slab's end mb1
  int s = wave, mbs = 0, mb1 = 0;
  // one group: the next group's loads, this group's MFMAs, and at a slab's end its tile to LDS
  auto step = [&](const Grp& cur, Grp& nxt) -> bool {
    int ns = s, nmbs = mbs + KB, nmb1 = mb1;
    if (nmbs >= mb1) {
      ns = s + 4;
      slab(ns, nmbs, nmb1);
    }
    load(nxt, ns, nmbs, nmb1);
    compute(cur, mbs, mb1);
    if (ns != s) {
      float* slot = slots + s * (32 * 32);
#pragma unroll
      for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fn = 0; fn < 2; ++fn)
#pragma unroll
          for (int j = 0; j < 4; ++j) slot[tr_fold_off(fm * 16 + (lane >> 4) * 4 + j, fn * 16 + lr)] = acc[fm][fn][j];
      tl_zero(acc);
    }
    s = ns;
    mbs = nmbs;
    mb1 = nmb1;
    return s < F;
  };
  if (s < F) {
    slab(s, mbs, mb1);
    Grp A, B;
    load(A, s, mbs, mb1);
    while (step(A, B) && step(B, A)) {
    }
  }
  __syncthreads();
  // thread = (row, 4 columns): the slots in slab order, then one whole 128-byte line of the
  // tile per 8 lanes
  const int row = tid >> 3, c4 = (tid & 7) * 4;
  const float* src = slots + tr_fold_off(row, c4);
  float4_t pw = {0.f, 0.f, 0.f, 0.f}, mw = pw, vw = pw;
  const int64_t fi = fuse ? fz.off + (p0 + row) * Q + q0 + c4 : 0;
  if (fuse) {  // uniform; the optimizer slots' latency overlaps the slot sum
    pw = *reinterpret_cast<const float4_t*>(o.p + fi);
    mw = *reinterpret_cast<const float4_t*>(o.m + fi);
    vw = *reinterpret_cast<const float4_t*>(o.v + fi);
  }
  float4_t g = {0.f, 0.f, 0.f, 0.f};
  for (int sl = 0; sl < F; ++sl) g += *reinterpret_cast<const float4_t*>(src + sl * (32 * 32));
  if (!fuse) {
    *reinterpret_cast<float4_t*>(pr.part + (p0 + row) * Q + q0 + c4) = g;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float gs = 0.f;  // the one-slab sum of tr_opt_tile
    gs += g[j];
    float pj = pw[j], mj = mw[j], vj = vw[j];
    tr_opt_update(o.c, gs, pj, mj, vj);
    pw[j] = pj;
    mw[j] = mj;
    vw[j] = vj;
  }
  *reinterpret_cast<float4_t*>(o.p + fi) = pw;
  *reinterpret_cast<float4_t*>(o.m + fi) = mw;
  *reinterpret_cast<float4_t*>(o.v + fi) = vw;
  if (!fz.sh) return;  // uniform
  // four 8 x 32 sub-tiles, one per wave, staged in the LDS the slots no longer need
  __syncthreads();
  float(*st)[33] = reinterpret_cast<float(*)[33]>(slots);
#pragma unroll
  for (int j = 0; j < 4; ++j) st[row][c4 + j] = pw[j];
  __syncthreads();
  tr_opt_shadow(fz.sh, fz.shT, pr.P, pr.Q, p0 + wave * 8, q0, st + wave * 8, lane);
}

// ----------------------------------------------------------------------------
// tr_opt: split-K reduce and/or the optimizer over the flat fp32 parameters, the bf16
// weight shadows, loss hand-off and the RNG counter advance (hipGraph-replay safe)
// ----------------------------------------------------------------------------
// GATHER: the launch also carries the next step's layer-0 gather tiles (pipelined step);
// a separate instantiation so the plain optimizer keeps its small register footprint
// one 8 x 32 (or 256-element) tile of the optimizer launch: split-K reduce and / or the
// update, the bf16 shadows of weight tiles; block 0 also reduces the head statistics
// The wait of a routed-segment tile block of a fused dW launch for the `want` producers of its
// routed tile.  Consumer form: one lane's relaxed agent-scope poll (s_sleep between polls, the
// other waves sit at the barrier), ONE agent acquire, the wait for its invalidate, the workgroup
// barrier; the slab loads that follow are agent-scope loads too.  Bounded: past a.timeout ticks
// of the wall clock the block flags the plan's status word, poisons the step's loss and goes on
// with whatever the slabs hold: a wrong, flagged result, never a hang (as in xgmi_ar.hip).
__device__ __forceinline__ void tr_fuse_wait(const TrDwOpt& a, const uint32_t* cnt, uint32_t want) {
  if (threadIdx.x == 0) {
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {
      if (wall_clock64() - t0 > a.timeout) {
        __hip_atomic_store(a.sync + kTrSyncLine, kTrFuseTimeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.c.loss_out, __builtin_nanf(""), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}

// FUSE (A = TrDwOpt, MODE 2): a trailing block of the dW launch; the slabs are read with
// agent-scope loads, and a tile of a routed segment first waits for its producers.
template <bool FUSE>
__device__ __forceinline__ float tr_slab_load(const float* p) {
  if constexpr (FUSE) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}

template <int MODE, bool FUSE = false, class A = TrOptArgs>
__device__ __forceinline__ void tr_opt_tile(const A& a, int b, float (*tile_s)[33]) {
  static_assert(!FUSE || MODE == 2, "trailing blocks run the fused reduce + update");
  const int tid = threadIdx.x;
  if (b == 0 && tid < 64 && MODE != 3 && a.c.nhead > 0) {
    // head statistics: reduce (modes 0/2) the per-block partials; hand the loss over (1/2);
    // nhead == 0: a segment-subset reduce launch that leaves them to another launch
    if constexpr (MODE != 1) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      for (int k = tid; k < a.c.nhead; k += 64)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] += a.c.head_part[k * 4 + c];
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = wave_sum(v[c]);
      if (tid == 0) {
        a.c.loss_acc[0] = v[0];
        if (a.c.stat_f) {
          a.c.stat_f[0] += v[1];
        } else if (a.c.counts) {
          a.c.counts[0] += static_cast<uint32_t>(v[1]);
          a.c.counts[1] += static_cast<uint32_t>(v[2]);
          a.c.counts[2] += static_cast<uint32_t>(v[3]);
        }
        if (MODE == 2) a.c.loss_out[0] = v[0];
      }
    } else if (tid == 0) {
      a.c.loss_out[0] = a.c.loss_acc[0];
    }
  }
  TrSeg sg = a.seg[0];
  int ks = 0;
#pragma unroll
  for (int k = 1; k < kTrMaxSegs; ++k)
    if (k < a.nseg && b >= a.seg[k].blk0) {
      sg = a.seg[k];
      ks = k;
    }
  (void)ks;
  const int local = b - sg.blk0;
  int64_t i;
  int r = 0, c = 0;
  bool valid = true;
  // vector segment with slab groups (tr_seg_layout): thread = (group, element); uniform per block
  const int grp = sg.cols == 0 && sg.sgrp > 1 ? sg.sgrp : 1;
  const int per = 256 / grp, sub = tid / per;
  if (sg.cols > 0) {  // 8 x 32 tile of a weight matrix
    const int tiles_c = sg.cols >> 5;
    const int tr = local / tiles_c, tc = local - tr * tiles_c;
    r = tr * 8 + (tid >> 5);
    c = tc * 32 + (tid & 31);
    i = sg.off + static_cast<int64_t>(r) * sg.cols + c;
  } else {
    i = sg.off + static_cast<int64_t>(local) * per + (tid - sub * per);
    valid = i < sg.off + sg.n;
    if (!valid) i = sg.off;  // clamped: no early return before the tile barrier
    valid = valid && sub == 0;  // groups 1.. only help with the slab sum
  }
  float p = a.p[i];
  // optimizer slots loaded up front: independent of the split-K sum, so their latency
  // overlaps the partial-slab loads instead of adding a round trip after them
  float m = 0.f, v = 0.f;
  if (MODE == 1 || MODE == 2) {
    m = a.m[i];
    v = a.v[i];
  }
  if constexpr (FUSE) {
    if (ks >= a.rseg0) {  // uniform: a routed segment; the 64 x 128 routed tile this 8 x 32 tile lies in
      const int rt = (r >> 6) * ((sg.cols + 127) >> 7) + (c >> 7);  // the same for the block's 8 rows x 32 columns
      const int c0 = ks == a.rseg0 ? a.cnt0[0] : a.cnt0[1];         // constant indices only
      tr_fuse_wait(a, a.sync + static_cast<int64_t>(c0 + rt) * kTrSyncLine, static_cast<uint32_t>(sg.S));
    }
  }
  if (MODE != 3) {
    float g;
    if constexpr (MODE != 1) {
      // split-K slabs: 16 loads in flight, indices clamped (no branch around a load; 32 in
      // flight measured slower: 9.38 vs 8.75 us, profiles/r3_headline/)
      const float* src = sg.part + (i - sg.off);
      g = 0.f;
      // one slab (a dW problem summed in its blocks, tr_dw_fold_body): one load; uniform
      if (sg.S == 1) g += tr_slab_load<FUSE>(src);
      // slabs sub, sub + grp, ... (grp == 1: all of them, in order)
      for (int s0 = sub; sg.S > 1 && s0 < sg.S; s0 += 16 * grp) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int sl = s0 + u * grp;
          v[u] = tr_slab_load<FUSE>(src + static_cast<int64_t>(sl < sg.S ? sl : sg.S - 1) * sg.n);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) g += (s0 + u * grp < sg.S) ? v[u] : 0.f;
      }
      if (grp > 1) {  // the groups' sums, in group order (deterministic)
        float* red = &tile_s[0][0];
        red[tid] = g;
        __syncthreads();
        const int e = tid - sub * per;
        g = red[e];
        for (int q = 1; q < grp; ++q) g += red[q * per + e];
      }
      if constexpr (MODE == 0) {
        if (valid) {
          if (a.g16) a.g16[i] = f2bf(g);
          else a.g[i] = g;
        }
        return;
      }
    } else {
      g = a.g16 ? bf2f(a.g16[i]) : a.g[i];
    }
    tr_opt_update(a.c, g, p, m, v);
    if (valid) {
      a.p[i] = p;
      a.m[i] = m;
      a.v[i] = v;
    }
  }
  // bf16 shadows of a weight tile: rows as 16-B fm chunks (threads 0-31), columns of the
  // transpose (threads 32-63)
  if (sg.cols > 0 && sg.sh) {
    tile_s[tid >> 5][tid & 31] = p;
    __syncthreads();
    if (tid < 64) tr_opt_shadow(sg.sh, sg.shT, sg.rows, sg.cols, r - (tid >> 5), c - (tid & 31), tile_s, tid);
  }
}

// every dW of the step in one launch and, fused, the optimizer in its trailing blocks (TrDwLaunch)
__global__ __launch_bounds__(256, 2) void tr_dw_all_kernel(TrDwLaunch a) {
  __shared__ __attribute__((aligned(16))) RouteLds gs;
  __shared__ uint4_t lut[256];
  const int b = blockIdx.x;
  const bool pipe = a.route_impl == 2;  // that body fills the table itself, behind its first loads
  if (!pipe && a.nroute > 0 && b < a.rwg[a.nroute]) {  // routed blocks: the fragment-spread table first
    tr_spread_lut_init(lut);
    __syncthreads();
  }
  if (pipe && a.nroute > 0 && b < a.rwg[a.nroute]) {
    // one copy of the body for both routed problems: the problem is picked into registers
    const bool second = b >= a.rwg[1];  // uniform
    TrDwProb pr = a.route[0];
    if (second) pr = a.route[1];
    uint32_t* ready = a.fuse ? a.opt.sync + static_cast<int64_t>(second ? a.opt.cnt0[1] : a.opt.cnt0[0]) * kTrSyncLine : nullptr;
    tr_dw_route_pipe_body(pr, second ? b - a.rwg[1] : b, gs, lut, second ? nullptr : a.prof, ready);
  } else if (a.nroute > 0 && b < a.rwg[1]) {
    tr_dw_route_body(a.route[0], b, gs, lut, a.prof,
                     a.fuse ? a.opt.sync + static_cast<int64_t>(a.opt.cnt0[0]) * kTrSyncLine : nullptr);
  } else if (a.nroute > 1 && b < a.rwg[2]) {
    tr_dw_route_body(a.route[1], b - a.rwg[1], gs, lut, nullptr,
                     a.fuse ? a.opt.sync + static_cast<int64_t>(a.opt.cnt0[1]) * kTrSyncLine : nullptr);
  } else if (b < a.ndw) {
    // the dW block count, not the grid's: trailing blocks do not move the stored-G blocks
    const int r = a.rwg[a.nroute];
    const int id = xcd_remap(b - r, a.ndw - r);
    // constant indices only (no dynamic indexing of kernel arguments)
    TrDwProb pr = a.plain.p[0];
    TrFoldSeg fz = a.opt.fseg[0];
#pragma unroll
    for (int i = 1; i < kTrMaxProbs; ++i)
      if (a.plain.n > i && id >= a.plain.p[i].wg0) {
        pr = a.plain.p[i];
        fz = a.opt.fseg[i];
      }
    float* slots = reinterpret_cast<float*>(&gs[0][0][0]);
    if (pr.F > 0) tr_dw_fold_body(pr, id - pr.wg0, slots, a.opt, fz, a.fuse != 0);  // uniform per block
    else tr_dw_plain_body(pr, id - pr.wg0);
  } else {
    // Trailing optimizer blocks of a fused launch.  A tile block waits only for routed blocks,
    // which have lower block ids and wait for nothing.  Workgroups are dispatched in id order,
    // so by the time a trailing block is resident every one of its producers has been
    // dispatched and runs to its end whatever the trailing blocks do: no cycle, no deadlock
    // (the assumption of the decoupled look-back scan graph_build.hip relies on).  The blocks
    // that wait for nothing come first, so they never queue behind pollers.
    tr_opt_tile<2, true>(a.opt, b - a.ndw, reinterpret_cast<float(*)[33]>(&gs[0][0][0]));
    // done ticket: taken by the polling lane behind its poll; the last of the launch zeroes the
    // counters and the ticket, so a graph replay or a second launch starts from zero without a
    // memset node.  Every other trailing block has finished polling by then, and a tile's
    // counter reached S only after all its producers' adds.
    if (threadIdx.x == 0) {
      const uint32_t nt = static_cast<uint32_t>(gridDim.x) - static_cast<uint32_t>(a.ndw);
      if (__hip_atomic_fetch_add(a.opt.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nt - 1u) {
        for (int k = 2; k < a.opt.nsync; ++k)
          __hip_atomic_store(a.opt.sync + static_cast<int64_t>(k) * kTrSyncLine, 0u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.opt.sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

template <int MODE, typename FT, int GATHER>
__global__ __launch_bounds__(256, GATHER ? 4 : 1) void tr_opt_kernel(TrOptArgs a) {
  __shared__ float tile_s[8][33];
  __shared__ int32_t node_s[kTrSampleRows];
  extern __shared__ __attribute__((aligned(16))) bf16_t glds[];  // gather tiles only
  int b = blockIdx.x;
  // GATHER launches: opt_tpb parameter tiles per block, so the parameter blocks take few of
  // the slots the gather tiles need
  const int tpb = GATHER && a.opt_tpb > 1 ? a.opt_tpb : 1;
  const int nopt = (a.nblk + tpb - 1) / tpb;
  if constexpr (GATHER) {
    // the next step's layer-0 gather (pipelined step): first in the grid unless
    // gather_first == 0
    if (a.gather_first) {
      if (b < a.ngather) {
        tr_gather32_tile<FT>(a.gat, b, glds);
        return;
      }
      b -= a.ngather;
    } else if (b >= nopt + a.nsample) {
      tr_gather32_tile<FT>(a.gat, b - nopt - a.nsample, glds);
      return;
    }
  }
  if (b >= nopt) {  // the next step's sampler (modes 1/2)
    tr_sample_block<256>(a.smp, b - nopt, node_s);
    return;
  }
  for (int r = 0; r < tpb; ++r) {
    const int bt = b * tpb + r;
    if (bt >= a.nblk) break;  // uniform across the block
    tr_opt_tile<MODE>(a, bt, tile_s);
    if (tpb > 1) __syncthreads();  // tile_s is reused by the next tile
  }
}

}  // namespace euler_hip

using namespace euler_hip;

extern "C" {

static_assert(kRP == kTrRouteP && kRQ == kTrRouteQ, "tree_plan.h plans the routed tiles of tr_dw_route");

hipError_t eh_tr_dw(TrDwLaunch* L, hipStream_t s) {
  TrDwGrid grid;
  if (!tr_dw_layout(*L, grid)) return hipErrorInvalidValue;
  if (grid.ndw == 0) return hipSuccess;
  hipLaunchKernelGGL(tr_dw_all_kernel, dim3(static_cast<uint32_t>(grid.ndw + grid.ntrail)), dim3(256), 0, s, *L);
  return hipGetLastError();
}

size_t eh_tr_gather32_lds(int D, int FL) {
  return static_cast<size_t>(kG32Rows) * 2 * D * sizeof(bf16_t) + static_cast<size_t>(kG32Rows) * (1 + FL) * sizeof(int32_t);
}

hipError_t eh_tr_opt(const TrOptArgs* ain, int mode, hipStream_t s) {
  TrOptArgs A = *ain;
  const TrOptArgs* a = &A;
  if (!(mode == 1 || mode == 2)) A.nsample = 0;  // the sampler runs in modes 1/2 only
  if (mode == 3) A.ngather = 0;
  if (!a->p || !a->g || !a->m || !a->v || !a->c.step || !a->c.loss_acc || !a->c.loss_out || !a->c.head_part ||
      a->c.nhead < 0 || (a->c.nhead == 0 && mode != 0 && mode != 3))
    return hipErrorInvalidValue;
  if (a->nblk < 1 || tr_seg_layout(A.seg, a->nseg, false) != a->nblk) return hipErrorInvalidValue;
  int extra = 0;
  if (a->nsample > 0) {
    if (!tr_sample_ok(a->smp, kTrSampleRows, a->nsample)) return hipErrorInvalidValue;
    extra = a->nsample;
  }
  size_t lds = 0;
  if (a->ngather > 0) {
    // every gather tile reads ids and features and writes both A copies of its 32 rows;
    // sibling groups must fit a tile (P <= 32) and rows be whole 16-byte chunks
    const TrFwdArgs& g = a->gat;
    if (!g.x || !g.nodes || !g.leaf || !g.a_kt || !g.a_rows || g.FL < 1 || g.D % 8 != 0 || g.D <= 0 ||
        g.M % kG32Rows != 0 || a->ngather != g.M / kG32Rows || g.logPg < 2 || (1 << g.logPg) > kG32Rows ||
        g.Fg >= (1 << g.logPg))
      return hipErrorInvalidValue;
    lds = eh_tr_gather32_lds(g.D, g.FL);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    extra += a->ngather;
  }
  const int tpb = a->ngather > 0 && a->opt_tpb > 1 ? a->opt_tpb : 1;
  const int nopt = (a->nblk + tpb - 1) / tpb;
  const dim3 grid(static_cast<uint32_t>(nopt + extra));
#define TR_OPT(MODEV, FT, G) hipLaunchKernelGGL((tr_opt_kernel<MODEV, FT, G>), grid, dim3(256), lds, s, A)
  if (a->ngather > 0 && a->gat_fp32) {
    if (mode == 0) TR_OPT(0, float, 1);
    else if (mode == 1) TR_OPT(1, float, 1);
    else if (mode == 2) TR_OPT(2, float, 1);
    else return hipErrorInvalidValue;
  } else if (a->ngather > 0) {
    if (mode == 0) TR_OPT(0, bf16_t, 1);
    else if (mode == 1) TR_OPT(1, bf16_t, 1);
    else if (mode == 2) TR_OPT(2, bf16_t, 1);
    else return hipErrorInvalidValue;
  } else {
    if (mode == 0) TR_OPT(0, bf16_t, 0);
    else if (mode == 1) TR_OPT(1, bf16_t, 0);
    else if (mode == 2) TR_OPT(2, bf16_t, 0);
    else if (mode == 3) TR_OPT(3, bf16_t, 0);
    else return hipErrorInvalidValue;
  }
#undef TR_OPT
  return hipGetLastError();
}

}  // extern "C"
