// Host-side planning and validation of the dW launch and the flat-parameter segments of the
// fused GraphSAGE tree step: split-K plans, block geometry, segment layout, the description
// of the optimizer inside the dW launch, and the sampler-argument check of the three launches
// that carry a sampler.  Each rule is written once here and read by both the launchers
// (tree_dw.hip: eh_tr_dw, eh_tr_opt; tree_fwd.hip: eh_tr_sample; tree_head.hip: eh_tr_head)
// and the binding (binding_tree.cpp).  Plain
// C++17, host only: no torch, no device code, no HIP runtime call, so
// csrc/tests/tree_plan_selftest.cc checks it on a CPU.
#pragma once
#include "hip/tree_args.h"

namespace euler_hip {

// ----------------------------------------------------------------------------- the sampler
// The sampler blocks of a launch (tr_sample_block: rows_per_block target rows each) can run on
// a: every array they read or write is set, a leaf fanout, a level the slot chain knows, and
// nblocks blocks cover the M target rows exactly.
inline bool tr_sample_ok(const TrSampleArgs& a, int rows_per_block, int64_t nblocks) {
  if (!a.g.indptr || !a.g.nbr || !a.g.cumw || !a.g.prob || !a.g.alias || !a.tr.rng || !a.roots || !a.nodes || !a.leaf)
    return false;
  if (a.FL < 1 || a.lv < 0 || a.lv > 2 || rows_per_block < 1) return false;
  return nblocks == (a.M + rows_per_block - 1) / rows_per_block;
}

// ----------------------------------------------------------------------------- split-K plans
// Stored-G problem (P, Q, MB set): ~target workgroups of 64x64 tiles, at least min_kps 32-row
// k-blocks per slab.  With `fold` and at most kTrFoldMax slabs the block sums them (F = the
// slab count, S = 1: `part` and the optimizer see one slab); more slabs keep the global path
// (F = 0, S = the slab count).
inline void tr_plan_stored(TrDwProb& p, int64_t target, int64_t min_kps, bool fold) {
  const int64_t MB = p.MB;
  const int64_t tiles = ((p.P + 63) / 64) * ((p.Q + 63) / 64);
  int64_t kps = (MB * tiles + target - 1) / target;
  if (kps < min_kps) kps = min_kps;
  if (kps > MB) kps = MB;
  const int64_t slabs = (MB + kps - 1) / kps;
  p.kps = static_cast<int32_t>(kps);
  p.F = fold && slabs <= kTrFoldMax ? static_cast<int32_t>(slabs) : 0;
  p.S = p.F ? 1 : static_cast<int32_t>(slabs);
}

// routed problems run on kTrRouteP x kTrRouteQ tiles (tree_dw.hip: kRP, kRQ)
constexpr int kTrRouteP = 64, kTrRouteQ = 128;
inline int32_t tr_route_tiles_q(const TrDwProb& p) { return (p.Q + kTrRouteQ - 1) / kTrRouteQ; }
inline int32_t tr_route_tiles(const TrDwProb& p) { return (p.P / kTrRouteP) * tr_route_tiles_q(p); }

// Routed problem (P, Q, MB set): S a multiple of 8 (the XCD mapping) near target workgroups
// and at most MB rounded up to 8; S >= ceil(MB / kps), so trailing slabs may be empty (they
// are written as zeros).  False: no plan (P no positive multiple of the tile, Q, MB or target
// below 1).
inline bool tr_plan_routed(TrDwProb& p, int64_t target) {
  if (p.P < kTrRouteP || p.P % kTrRouteP != 0 || p.Q < 1 || p.MB < 1 || target < 1) return false;
  const int64_t MB = p.MB, tiles = tr_route_tiles(p);
  int64_t S = (target + tiles - 1) / tiles;
  S = (S + 7) / 8 * 8;
  if (S > (MB + 7) / 8 * 8) S = (MB + 7) / 8 * 8;
  p.kps = static_cast<int32_t>((MB + S - 1) / S);
  p.S = static_cast<int32_t>(S);
  return true;
}

// ----------------------------------------------------------------------------- segments
// vector segments with many split-K slabs (the fc bias: one slab per head block) spread each
// element's slab sum over 4 threads (256 / 4 elements per block): one round of 16 loads in
// flight per thread instead of S / 16 dependent rounds, which made the bias block the tail
// of the optimizer launch
inline int tr_seg_groups(const TrSeg& s) { return s.cols == 0 && s.S > 16 ? 4 : 1; }
inline int tr_seg_blocks(const TrSeg& s) {
  if (s.cols > 0) return (s.rows / 8) * (s.cols / 32);
  const int64_t per = 256 / tr_seg_groups(s);
  return static_cast<int>((s.n + per - 1) / per);
}

// The layout of a segment array: blocks are handed out in order (blk0 of a segment = the
// blocks of those before it) and vector segments carry their slab groups (sgrp).  fill: set
// blk0 and sgrp; otherwise they must already hold these values.  Returns the block total, or
// -1 when the array is no valid argument of the kernels: n outside 1..kTrMaxSegs, a segment
// without slabs, a weight segment that is not whole 8 x 32 tiles of exactly n elements, a
// vector segment with shadows, or (!fill) a blk0 / sgrp that is not the layout's.
inline int tr_seg_layout(TrSeg* seg, int n, bool fill) {
  if (n < 1 || n > kTrMaxSegs) return -1;
  int blk = 0;
  for (int k = 0; k < n; ++k) {
    TrSeg& g = seg[k];
    if (fill) {
      g.blk0 = blk;
      g.sgrp = tr_seg_groups(g);
    }
    if (!g.part || g.S < 1 || g.blk0 != blk) return -1;
    if (g.cols > 0) {
      if (g.rows % 8 != 0 || g.cols % 32 != 0 || static_cast<int64_t>(g.rows) * g.cols != g.n) return -1;
    } else if (g.cols < 0 || g.sh || g.shT || g.sgrp != tr_seg_groups(g)) {
      return -1;
    }
    blk += tr_seg_blocks(g);
  }
  return blk;
}

// ----------------------------------------------------------------------------- the dW launch
struct TrDwGrid {
  int32_t ndw = 0;             // dW blocks: the routed problems' (rtiles[r] * S each), then the stored-G ones
  int32_t ntrail = 0;          // trailing optimizer blocks of a fused launch
  int32_t rtiles[2] = {0, 0};  // tiles of routed problem r (one hand-off line each when fused)
};

// Lays out launch L: tiles_q / ntiles / wg0 of every problem, the routed block prefix rwg, ndw
// and, fused, the first hand-off line cnt0 of every routed problem.  False: L is no valid
// argument of tr_dw_all_kernel.  A fused launch (L.fuse, L.opt from tr_dw_fuse) needs every
// stored-G problem folded with a flat segment of its own, the trailing segments vectors first,
// then one weight segment per routed problem whose slabs are that problem's, and a hand-off
// line for the ticket, the status and every routed tile.
inline bool tr_dw_layout(TrDwLaunch& L, TrDwGrid& grid) {
  grid = TrDwGrid{};
  TrDwProbs& pr = L.plain;
  if (pr.n < 0 || pr.n > kTrMaxProbs || L.nroute < 0 || L.nroute > 2) return false;
  L.rwg[0] = 0;
  for (int r = 0; r < L.nroute; ++r) {
    TrDwProb& p = L.route[r];
    if (!p.route || !p.dA || !p.mask || !p.X || !p.part) return false;
    if (p.P % kTrRouteP != 0 || p.Q % 32 != 0 || p.MB < 1 || p.kps < 1 || p.logPg < 3) return false;
    // the XCD-aware block mapping needs S % 8 == 0 (splits past MB write zero slabs)
    if (p.S % 8 != 0 || static_cast<int64_t>(p.S) * p.kps < p.MB) return false;
    p.tiles_q = tr_route_tiles_q(p);
    p.ntiles = tr_route_tiles(p);
    p.wg0 = 0;
    grid.rtiles[r] = p.ntiles;
    L.rwg[r + 1] = L.rwg[r] + p.ntiles * p.S;
  }
  int wg = 0;
  for (int i = 0; i < pr.n; ++i) {
    TrDwProb& p = pr.p[i];
    if (p.P % 32 != 0 || p.Q % 32 != 0 || p.MB < 1 || p.kps < 1) return false;
    if (p.route || !p.G || !p.X || !p.part) return false;
    if (p.F < 0 || p.F > kTrFoldMax || p.S < 1) return false;
    // folded: F slabs cover K, one `part` slab, one workgroup per 32x32 tile; else one per
    // 64x64 tile and slab
    if (p.F > 0 && p.S != 1) return false;
    if (static_cast<int64_t>(p.F > 0 ? p.F : p.S) * p.kps < p.MB) return false;
    const int t = p.F > 0 ? 32 : 64;
    p.tiles_q = (p.Q + t - 1) / t;
    p.ntiles = ((p.P + t - 1) / t) * p.tiles_q;
    p.wg0 = wg;
    wg += p.ntiles * p.S;
  }
  L.ndw = grid.ndw = L.rwg[L.nroute] + wg;
  if (grid.ndw == 0 || !L.fuse) return true;
  TrDwOpt& o = L.opt;
  if (L.fuse != 1 || !o.p || !o.m || !o.v || !o.c.step || !o.c.loss_acc || !o.c.loss_out || !o.c.head_part ||
      o.c.nhead < 1 || !o.sync || o.timeout < 1 || o.rseg0 < 0 || o.rseg0 + L.nroute != o.nseg)
    return false;
  for (int i = 0; i < pr.n; ++i)
    if (pr.p[i].F < 1 || o.fseg[i].off < 0 || o.fseg[i].off % 4 != 0 || (o.fseg[i].shT && !o.fseg[i].sh)) return false;
  const int trail = tr_seg_layout(o.seg, o.nseg, false);
  if (trail < 0 || trail != o.nblk) return false;
  int line = 2;
  for (int k = 0; k < o.nseg; ++k) {
    const TrSeg& g = o.seg[k];
    if (k < o.rseg0) {
      if (g.cols != 0) return false;
      continue;
    }
    const TrDwProb& p = L.route[k - o.rseg0];
    if (g.cols < 1 || g.part != p.part || g.S != p.S || g.rows != p.P || g.cols != p.Q || (g.shT && !g.sh))
      return false;
    o.cnt0[k - o.rseg0] = line;
    line += p.ntiles;
  }
  if (line != o.nsync) return false;
  grid.ntrail = trail;
  return true;
}

// TrDwOpt of the laid-out launch L from the optimizer arguments o of tr_opt mode 2: each flat
// segment is found by the `part` slabs it sums.  Stored-G problems must be folded (their blocks
// update the tile themselves); vector segments, then the routed problems' segments in the
// launch's order, go to trailing blocks.  f.sync is left to the caller (f.nsync lines of
// kTrSyncLine words).  False: this launch cannot carry the optimizer (an unfolded stored-G
// problem, a problem or segment without its counterpart, no head statistics to reduce).
inline bool tr_dw_fuse(const TrDwLaunch& L, const TrOptArgs& o, TrDwOpt& f) {
  f = TrDwOpt{};
  const TrSeg* rseg[2] = {nullptr, nullptr};
  bool pseg[kTrMaxProbs] = {};
  int nvec = 0;
  for (int k = 0; k < o.nseg; ++k) {
    const TrSeg& g = o.seg[k];
    if (g.cols == 0) {
      f.seg[nvec++] = g;
      continue;
    }
    bool found = false;
    for (int r = 0; r < L.nroute && !found; ++r)
      if (L.route[r].part == g.part && !rseg[r]) {
        rseg[r] = &g;
        found = true;
      }
    for (int i = 0; i < L.plain.n && !found; ++i) {
      const TrDwProb& p = L.plain.p[i];
      if (p.part != g.part || pseg[i]) continue;
      if (p.F < 1 || g.S != 1 || g.rows != p.P || g.cols != p.Q || g.off % 4 != 0) return false;
      f.fseg[i] = TrFoldSeg{g.off, g.sh, g.shT};
      pseg[i] = true;
      found = true;
    }
    if (!found) return false;
  }
  for (int i = 0; i < L.plain.n; ++i)
    if (!pseg[i]) return false;
  f.rseg0 = nvec;
  f.nseg = nvec + L.nroute;
  if (f.nseg > kTrMaxSegs) return false;
  f.nsync = 2;
  for (int r = 0; r < L.nroute; ++r) {
    if (!rseg[r]) return false;
    f.seg[nvec + r] = *rseg[r];
    f.nsync += L.route[r].ntiles;
  }
  f.nblk = tr_seg_layout(f.seg, f.nseg, true);
  if (f.nblk < 0) return false;
  f.p = o.p;
  f.m = o.m;
  f.v = o.v;
  f.c = o.c;
  f.timeout = kTrFuseWaitTicks;
  return o.c.nhead > 0;
}

}  // namespace euler_hip
