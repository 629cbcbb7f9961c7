// CPU self-test of the dW / optimizer planner (hip/tree_plan.h): split plans, launch geometry,
// segment layout, the fused-optimizer description, the sampler-argument check and what each of
// them refuses.  Host code only: no HIP runtime call, nothing to link; pointers are dummies that
// are never followed.
// The shapes are those of the GPU tests that pin the same numbers through the plans
// (tests/test_dw_opt_fuse.py, test_dw_route_pipe.py, test_dw_fold.py), re-derived by hand.
#include <cstddef>
#include <cstdio>

#include "hip/tree_plan.h"

using namespace euler_hip;

namespace {

int failures = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                               \
    }                                                           \
  } while (0)

// distinct non-null dummies
float fbuf[16];
uint16_t hbuf[16];
uint32_t ubuf[64];
int64_t step;

TrDwProb routed(int P, int Q, int MB, int64_t target, float* part) {
  TrDwProb p{};
  p.P = P;
  p.Q = Q;
  p.MB = MB;
  p.route = 1;
  p.X = hbuf;
  p.dA = fbuf;
  p.mask = ubuf;
  p.part = part;
  p.logPg = 4;
  CHECK(tr_plan_routed(p, target));
  return p;
}

TrDwProb stored(int P, int Q, int MB, int64_t min_kps, bool fold, float* part) {
  TrDwProb p{};
  p.P = P;
  p.Q = Q;
  p.MB = MB;
  p.G = hbuf;
  p.X = hbuf + 1;
  p.part = part;
  tr_plan_stored(p, 512, min_kps, fold);
  return p;
}

TrSeg weight_seg(int64_t off, const TrDwProb& p) {
  TrSeg g{};
  g.off = off;
  g.n = static_cast<int64_t>(p.P) * p.Q;
  g.part = p.part;
  g.S = p.S;
  g.rows = p.P;
  g.cols = p.Q;
  return g;
}

TrSeg vec_seg(int64_t off, int64_t n, int S) {
  TrSeg g{};
  g.off = off;
  g.n = n;
  g.part = fbuf + 15;
  g.S = S;
  g.rows = 1;
  return g;
}

TrOptArgs opt_of(const TrSeg* segs, int n) {
  TrOptArgs o{};
  o.p = o.g = o.m = o.v = fbuf;
  for (int k = 0; k < n; ++k) o.seg[k] = segs[k];
  o.nseg = n;
  o.nblk = tr_seg_layout(o.seg, n, true);
  o.c.step = &step;
  o.c.head_part = o.c.loss_acc = o.c.loss_out = fbuf;
  o.c.nhead = 8;
  o.c.counts = ubuf;
  o.c.lr = 0.25f;
  o.c.kind = 3;
  return o;
}

// the fused launch of L: describe, attach, lay out again
bool fuse(TrDwLaunch& L, const TrOptArgs& o, TrDwGrid& g) {
  L.fuse = 0;
  if (!tr_dw_layout(L, g) || !tr_dw_fuse(L, o, L.opt)) return false;
  L.opt.sync = ubuf;
  L.fuse = 1;
  return tr_dw_layout(L, g);
}

// (a) tests/test_dw_opt_fuse.py::test_more_workgroups_than_the_device_holds
TrDwLaunch launch_a(TrOptArgs& o) {
  TrDwLaunch L{};
  L.route[0] = routed(256, 256, 64, 256, fbuf + 1);
  L.nroute = 1;
  L.plain.p[0] = stored(256, 512, 4, 4, true, fbuf + 2);
  L.plain.p[1] = stored(64, 256, 4, 4, true, fbuf + 3);
  L.plain.p[2] = stored(64, 64, 4, 4, true, fbuf + 4);
  L.plain.n = 3;
  const TrSeg segs[5] = {weight_seg(0, L.route[0]), weight_seg(65536, L.plain.p[0]), weight_seg(196608, L.plain.p[1]),
                         vec_seg(212992, 64, 8), weight_seg(213056, L.plain.p[2])};
  o = opt_of(segs, 5);
  return L;
}

void test_headline_like() {
  TrOptArgs o;
  TrDwLaunch L = launch_a(o);
  CHECK(L.route[0].S == 32 && L.route[0].kps == 2);
  for (int i = 0; i < 3; ++i) CHECK(L.plain.p[i].F == 1 && L.plain.p[i].S == 1 && L.plain.p[i].kps == 4);
  TrDwGrid g;
  CHECK(tr_dw_layout(L, g));
  CHECK(g.rtiles[0] == 8 && L.rwg[1] == 256);
  CHECK(L.plain.p[0].ntiles == 128 && L.plain.p[1].ntiles == 16 && L.plain.p[2].ntiles == 4);
  CHECK(L.plain.p[0].wg0 == 0 && L.plain.p[1].wg0 == 128 && L.plain.p[2].wg0 == 144);
  CHECK(g.ndw == 404 && L.ndw == 404 && g.ntrail == 0);
  CHECK(o.nblk == 256 + 128 * 4 + 16 * 4 + 1 + 4 * 4);  // tr_opt's own grid: one block per 8 x 32 tile
  CHECK(fuse(L, o, g));
  CHECK(g.ndw == 404 && g.ntrail == 257 && g.ndw + g.ntrail == 661);
  const TrDwOpt& f = L.opt;
  CHECK(f.nseg == 2 && f.rseg0 == 1 && f.nblk == 257 && f.nsync == 10 && f.cnt0[0] == 2);
  CHECK(f.seg[0].cols == 0 && f.seg[0].blk0 == 0 && f.seg[0].sgrp == 1);
  CHECK(f.seg[1].part == L.route[0].part && f.seg[1].blk0 == 1);
  CHECK(f.fseg[0].off == 65536 && f.fseg[1].off == 196608 && f.fseg[2].off == 213056);
  CHECK(f.c.nhead == 8 && f.timeout == kTrFuseWaitTicks && f.c.step == &step);
  // the whole core is the optimizer launch's
  CHECK(f.c.lr == 0.25f && f.c.kind == 3 && f.c.counts == ubuf && f.c.loss_out == fbuf && f.c.stat_f == nullptr);
  // the core sits where the flat fields sat: both kernels' argument layouts are unchanged
  static_assert(sizeof(TrOptCore) == 88 && offsetof(TrOptCore, head_part) == 40 && offsetof(TrOptCore, stat_f) == 80,
                "TrOptCore layout");
  static_assert(offsetof(TrOptArgs, c) == 56 + sizeof(TrSeg) * kTrMaxSegs, "TrOptArgs layout");
  static_assert(offsetof(TrOptArgs, smp) == offsetof(TrOptArgs, c) + 88, "TrOptArgs layout");
  static_assert(offsetof(TrDwOpt, sync) == offsetof(TrDwOpt, c) + 88, "TrDwOpt layout");
}

// the sampler-argument check of the three launches that carry a sampler
void test_sampler_args() {
  static int64_t i64[2];
  static int32_t i32[8];
  TrSampleArgs a{};
  a.g.indptr = i64;
  a.g.nbr = a.g.alias = i32;
  a.g.cumw = a.g.prob = fbuf;
  a.tr.rng = i64;
  a.roots = i32 + 1;
  a.nodes = i32 + 2;
  a.leaf = i32 + 3;
  a.M = 130;
  a.lv = 1;
  a.FL = 10;
  CHECK(tr_sample_ok(a, 64, 3) && tr_sample_ok(a, 256, 1));  // the optimizer's and the head's sampler blocks
  CHECK(!tr_sample_ok(a, 64, 2) && !tr_sample_ok(a, 64, 4) && !tr_sample_ok(a, 256, 3) && !tr_sample_ok(a, 0, 3));
  TrSampleArgs b = a;
  b.lv = 0;
  CHECK(tr_sample_ok(b, 64, 3));
  b.lv = 2;
  CHECK(tr_sample_ok(b, 64, 3));
  b.lv = 3;
  CHECK(!tr_sample_ok(b, 64, 3));
  b.lv = -1;
  CHECK(!tr_sample_ok(b, 64, 3));
  b = a;
  b.FL = 0;
  CHECK(!tr_sample_ok(b, 64, 3));
#define NULLED(field)              \
  do {                             \
    b = a;                         \
    b.field = nullptr;             \
    CHECK(!tr_sample_ok(b, 64, 3)); \
  } while (0)
  NULLED(g.indptr);
  NULLED(g.nbr);
  NULLED(g.cumw);
  NULLED(g.prob);
  NULLED(g.alias);
  NULLED(tr.rng);
  NULLED(roots);
  NULLED(nodes);
  NULLED(leaf);
#undef NULLED
  // optional arrays stay optional
  b = a;
  b.g.root_rows = nullptr, b.tr.root_in = nullptr;
  CHECK(tr_sample_ok(b, 64, 3));
}

void test_split_plans() {
  // (b) tests/test_dw_route_pipe.py::test_zero_slabs_and_a_short_last_slab
  TrDwLaunch L{};
  L.route[0] = routed(64, 64, 80, 32, fbuf);
  L.nroute = 1;
  CHECK(L.route[0].S == 32 && L.route[0].kps == 3 && L.route[0].S * L.route[0].kps >= 80);
  TrDwGrid g;
  CHECK(tr_dw_layout(L, g) && g.ndw == 32 && g.rtiles[0] == 1);
  // (c) tests/test_dw_opt_fuse.py::test_fold_minimum_eight_routed_slabs
  TrDwProb r = routed(64, 64, 48, 8, fbuf);
  CHECK(r.S == 8 && r.kps == 6);
  TrDwProb p = stored(64, 128, 3, 1, true, fbuf);
  CHECK(p.kps == 1 && p.F == 3 && p.S == 1);
  p = stored(64, 128, 3, 1, false, fbuf);
  CHECK(p.kps == 1 && p.F == 0 && p.S == 3);
  // (d) more than kTrFoldMax slabs keep the global path (tests/test_dw_fold.py)
  static_assert(kTrFoldMax == 16, "the fold's LDS holds 16 tiles");
  p = stored(64, 64, 80, 4, true, fbuf);
  CHECK(p.kps == 4 && p.F == 0 && p.S == 20);
  p = stored(64, 64, 64, 4, true, fbuf);
  CHECK(p.kps == 4 && p.F == 16 && p.S == 1);
  // no routed plan without whole tiles or a target
  TrDwProb bad{};
  bad.P = 96, bad.Q = 64, bad.MB = 8;
  CHECK(!tr_plan_routed(bad, 256));
  bad.P = 64;
  CHECK(!tr_plan_routed(bad, 0));
  CHECK(tr_plan_routed(bad, 256) && bad.S == 8 && bad.kps == 1);
}

void test_segments() {
  // (e) slab groups of a vector segment
  TrSeg s[3] = {vec_seg(0, 100, 17), vec_seg(100, 300, 16), weight_seg(400, stored(64, 96, 4, 4, true, fbuf))};
  CHECK(tr_seg_layout(s, 3, true) == 2 + 2 + 8 * 3);
  CHECK(s[0].sgrp == 4 && s[0].blk0 == 0 && tr_seg_blocks(s[0]) == 2);  // 64 elements per block
  CHECK(s[1].sgrp == 1 && s[1].blk0 == 2 && s[2].blk0 == 4);
  CHECK(tr_seg_layout(s, 3, false) == 28);
  // (g) what a segment array is refused for
  CHECK(tr_seg_layout(s, 0, true) == -1 && tr_seg_layout(s, kTrMaxSegs + 1, true) == -1);
  TrSeg t[3] = {s[0], s[1], s[2]};
  t[1].blk0 = 3;
  CHECK(tr_seg_layout(t, 3, false) == -1);
  t[1] = s[1];
  t[0].sgrp = 1;
  CHECK(tr_seg_layout(t, 3, false) == -1);
  t[0] = s[0];
  t[2].cols = 48, t[2].n = 64 * 48;
  CHECK(tr_seg_layout(t, 3, true) == -1);
  t[2] = s[2];
  t[2].rows = 60, t[2].n = 60 * 96;
  CHECK(tr_seg_layout(t, 3, true) == -1);
  t[2] = s[2];
  t[2].n += 1;
  CHECK(tr_seg_layout(t, 3, true) == -1);
  t[2] = s[2];
  t[1].sh = hbuf;
  CHECK(tr_seg_layout(t, 3, true) == -1);
  t[1] = s[1];
  t[1].S = 0;
  CHECK(tr_seg_layout(t, 3, true) == -1);
  t[1] = s[1];
  t[1].part = nullptr;
  CHECK(tr_seg_layout(t, 3, true) == -1);
  t[1] = s[1];
  CHECK(tr_seg_layout(t, 3, true) == 28);
}

// (f) the pair step: two routed problems, four folded ones, two bias vectors
void test_two_routed() {
  TrDwLaunch L{};
  L.route[0] = routed(64, 128, 16, 256, fbuf + 1);   // 1 tile, S = 16
  L.route[1] = routed(128, 256, 64, 256, fbuf + 2);  // 4 tiles, S = 64
  L.nroute = 2;
  for (int i = 0; i < 4; ++i) L.plain.p[i] = stored(64, 128, 8, 4, true, fbuf + 3 + i);
  L.plain.n = 4;
  const TrSeg segs[8] = {weight_seg(0, L.route[0]),    weight_seg(8192, L.plain.p[0]),  weight_seg(16384, L.plain.p[1]),
                         vec_seg(24576, 32, 2),        weight_seg(24608, L.route[1]),   weight_seg(57376, L.plain.p[2]),
                         weight_seg(65568, L.plain.p[3]), vec_seg(73760, 32, 2)};
  const TrOptArgs o = opt_of(segs, 8);
  TrDwGrid g;
  CHECK(fuse(L, o, g));
  CHECK(L.route[0].S == 16 && L.route[1].S == 64 && g.rtiles[0] == 1 && g.rtiles[1] == 4);
  CHECK(L.rwg[0] == 0 && L.rwg[1] == 16 && L.rwg[2] == 16 + 256);
  CHECK(g.ndw == 272 + 4 * 8);
  const TrDwOpt& f = L.opt;
  CHECK(f.rseg0 == 2 && f.nseg == 4 && f.cnt0[0] == 2 && f.cnt0[1] == f.cnt0[0] + L.route[0].ntiles);
  CHECK(f.nsync == 2 + 1 + 4);
  CHECK(f.seg[2].part == L.route[0].part && f.seg[3].part == L.route[1].part);
  CHECK(g.ntrail == 1 + 1 + 8 * 4 + 16 * 8 && f.seg[3].blk0 == 2 + 32);
}

// (g) launches and fused descriptions that are refused
void test_rejections() {
  TrOptArgs o;
  TrDwGrid g;
  const TrDwLaunch good = launch_a(o);
  TrDwLaunch L = good;
  CHECK(fuse(L, o, g));
  L = good;
  L.route[0].S = 28, L.route[0].kps = 3;  // covers MB, but no multiple of 8
  CHECK(!tr_dw_layout(L, g));
  L = good;
  L.route[0].kps = 1;  // 32 slabs of one k-block do not cover MB = 64
  CHECK(!tr_dw_layout(L, g));
  L = good;
  L.plain.p[1].S = 2;  // folded problems have one slab
  CHECK(!tr_dw_layout(L, g));
  L = good;
  L.plain.p[1].F = kTrFoldMax + 1;
  CHECK(!tr_dw_layout(L, g));
  L = good;
  L.plain.p[1].G = nullptr;
  CHECK(!tr_dw_layout(L, g));
  L = good;
  L.nroute = 3;
  CHECK(!tr_dw_layout(L, g));
  // an unfolded stored-G problem: the launch is valid, but cannot carry the optimizer
  L = good;
  L.plain.p[2] = stored(64, 64, 4, 4, false, fbuf + 4);
  CHECK(L.plain.p[2].F == 0 && tr_dw_layout(L, g) && g.ndw == 256 + 128 + 16 + 1);
  CHECK(!tr_dw_fuse(L, o, L.opt));
  L.opt = TrDwOpt{};
  CHECK(fuse(L = good, o, g));
  L.plain.p[2].F = 0;  // ... and a fused launch with one is refused
  CHECK(!tr_dw_layout(L, g));
  // a routed segment whose slabs are not the problem's
  CHECK(fuse(L = good, o, g));
  L.opt.seg[1].part = fbuf + 9;
  CHECK(!tr_dw_layout(L, g));
  CHECK(fuse(L = good, o, g));
  L.opt.seg[1].blk0 = 2;
  CHECK(!tr_dw_layout(L, g));
  CHECK(fuse(L = good, o, g));
  L.opt.nsync = 9;
  CHECK(!tr_dw_layout(L, g));
  CHECK(fuse(L = good, o, g));
  L.opt.rseg0 = 0;
  CHECK(!tr_dw_layout(L, g));
  CHECK(fuse(L = good, o, g));
  L.opt.sync = nullptr;
  CHECK(!tr_dw_layout(L, g));
  // descriptions: a problem without its segment, a segment without its problem, no head blocks
  L = good;
  CHECK(tr_dw_layout(L, g));
  TrOptArgs q = o;
  q.seg[2].part = fbuf + 9;
  CHECK(!tr_dw_fuse(L, q, L.opt));
  q = o;
  q.nseg = 4;  // drops the segment of plain problem 2
  CHECK(!tr_dw_fuse(L, q, L.opt));
  q = o;
  q.seg[0].part = fbuf + 9;  // the routed problem finds no segment
  CHECK(!tr_dw_fuse(L, q, L.opt));
  q = o;
  q.seg[1].off = 65538;  // the fold's 16-byte stores
  CHECK(!tr_dw_fuse(L, q, L.opt));
  q = o;
  q.c.nhead = 0;
  CHECK(!tr_dw_fuse(L, q, L.opt));
  CHECK(tr_dw_fuse(L, o, L.opt));
}

}  // namespace

int main() {
  test_headline_like();
  test_sampler_args();
  test_split_plans();
  test_segments();
  test_two_routed();
  test_rejections();
  if (failures) {
    std::printf("tree_plan_selftest: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("tree_plan_selftest OK\n");
  return 0;
}
