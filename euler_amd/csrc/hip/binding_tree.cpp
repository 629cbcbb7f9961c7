// torch binding of the fused GraphSAGE tree step (tree_fwd.hip, tree_head.hip, tree_dw.hip).
//
// A TreePlan is built once per trainer from a dict of device tensors and sizes: every
// operand is validated here (PlanDict, binding_util.h: dtype, device, contiguity and the exact
// element count the kernels' grids assume), the kernel argument blocks are filled once, and
// the per-step methods only launch on torch's current stream (hipGraph-capturable, no
// allocation, no host sync, no per-call Python marshalling).
#include <cstdio>
#include <cstdlib>

#include "hip/binding_util.h"
#include "hip/tree_plan.h"

using namespace euler_bind;
using namespace euler_hip;

namespace {

// EULER_AMD_TREE_SYNC=1: synchronise after every launch and name the kernel that failed
// (debugging aid; never set it for timing or graph capture)
bool sync_debug() {
  static const bool on = [] {
    const char* e = std::getenv("EULER_AMD_TREE_SYNC");
    return e && e[0] == '1';
  }();
  return on;
}

void tree_ok(hipError_t e, const char* what) {
  launch_ok(e, what);
  if (sync_debug()) {
    const hipError_t s = hipStreamSynchronize(cur_stream());
    TORCH_CHECK(s == hipSuccess, "euler_amd tree kernel '", what, "' faulted: ", hipGetErrorString(s));
    fprintf(stderr, "[tree-sync] %s ok\n", what);
  }
}

// The sampled graph (CSR, root alias table) and the sampler fields of the tree, from the keys
// every tree-sampling plan shares: indptr, num_types, nbr, cumw, node_prob, node_alias,
// root_rows (optional), rng.  F / logP / m: fan-out, slot-group bits and edge mask of hops 1, 2
void fill_graph_tree(PlanDict& pd, TrGraph& g, TrTree& tr, int64_t F1, int64_t F2, int64_t logP1, int64_t logP2,
                     uint32_t m1, uint32_t m2) {
  torch::Tensor indptr = pd.T("indptr"), rng = pd.T("rng");
  pd.need(indptr, torch::kInt64, -1, "indptr");
  pd.need(rng, torch::kInt64, 2, "rng");
  const int64_t nt = pd.geti("num_types");
  TORCH_CHECK(nt >= 1 && nt <= 32 && (indptr.numel() - 1) % nt == 0, pd.name(), ": indptr must be [N*T+1]");
  g.indptr = indptr.data_ptr<int64_t>();
  g.num_types = static_cast<int32_t>(nt);
  g.num_rows = (indptr.numel() - 1) / nt;
  torch::Tensor nbr = pd.T("nbr"), cumw = pd.T("cumw"), prob = pd.T("node_prob");
  pd.need(nbr, torch::kInt32, -1, "nbr");
  pd.need(cumw, torch::kFloat32, nbr.numel(), "cumw");
  g.nbr = nbr.data_ptr<int32_t>();
  g.cumw = cumw.data_ptr<float>();
  pd.need(prob, torch::kFloat32, -1, "node_prob");
  g.pop = prob.numel();
  TORCH_CHECK(g.pop > 0, pd.name(), ": empty root population");
  g.prob = prob.data_ptr<float>();
  g.alias = pd.i32("node_alias", g.pop);
  // candidate -> row map of the root sampler (node-type subset)
  g.root_rows = pd.has("root_rows") ? pd.i32("root_rows", g.pop) : nullptr;
  tr.rng = rng.data_ptr<int64_t>();
  tr.F1 = static_cast<int32_t>(F1);
  tr.F2 = static_cast<int32_t>(F2);
  tr.logP1 = static_cast<int32_t>(logP1);
  tr.logP2 = static_cast<int32_t>(logP2);
  tr.m1 = m1;
  tr.m2 = m2;
}

// body of the routed dW problems, the key every plan shares: dw_route_impl (2: the pipelined
// stage loop; 0: build, load and multiply one after the other, the equality baseline; 1 was a
// body that built G per wave in registers: slower than both, profiles/dw_route_pipe/README.md)
int plan_route_impl(const PlanDict& pd) {
  const int64_t impl = pd.has("dw_route_impl") ? pd.geti("dw_route_impl") : 2;
  TORCH_CHECK(impl == 0 || impl == 2, pd.name(), ": dw_route_impl must be 0 or 2");
  return static_cast<int>(impl);
}

// the optimizer inside the dW launch, the key every plan shares: dw_opt_fuse (1: the single-process
// step runs the split-K reduce and the update in the dW launch, where the plan allows it; 0: the
// optimizer launch of its own)
bool plan_fuse_key(const PlanDict& pd) {
  const int64_t f = pd.has("dw_opt_fuse") ? pd.geti("dw_opt_fuse") : 1;
  TORCH_CHECK(f == 0 || f == 1, pd.name(), ": dw_opt_fuse must be 0 or 1");
  return f == 1;
}

// The dW problems of a plan, the optimizer over its flat parameters and, where the plan fuses,
// the optimizer inside the dW launch of every problem: its TrDwOpt and hand-off state are built
// once (try_fuse), a fused launch patches only lr, grad_scale and prof.  All geometry comes from
// tree_plan.h.
class DwPlan {
 public:
  explicit DwPlan(PlanDict& pd) : pd_(pd), route_impl_(plan_route_impl(pd)), fuse_key_(plan_fuse_key(pd)) {}

  std::vector<TrDwProb> probs;  // in the plan's order: the indices of launch() and splits()
  TrOptArgs opt{};              // tr_opt over the flat parameters

  // dW = G^T X [P][Q] over M rows, with its split plan and plan-owned partials.  dA: routed (G
  // built from the parent gradient through the tree and the ReLU bits), S from dw_route_wg
  // (256); else stored-G, from dw_target_wg (512), dw_min_kps (4) and dw_fold (1; 0 = every
  // slab goes through `part`)
  const TrDwProb& add(int64_t P, int64_t Q, int64_t M, const uint16_t* G, const uint16_t* X, const float* dA,
                      const uint32_t* mask, int64_t logPg, int64_t Fg, int64_t self) {
    TORCH_CHECK(M % 32 == 0 && P % 32 == 0 && Q % 32 == 0, pd_.name(), ": dW problem shapes");
    TrDwProb p{};
    p.P = static_cast<int32_t>(P);
    p.Q = static_cast<int32_t>(Q);
    p.MB = static_cast<int32_t>(M / 32);
    if (dA) {
      TORCH_CHECK(tr_plan_routed(p, pd_.has("dw_route_wg") ? pd_.geti("dw_route_wg") : 256), pd_.name(),
                  ": routed dW needs P % 64 == 0 and a positive dw_route_wg");
      p.route = 1;
      p.dA = dA;
      p.mask = mask;
      p.logPg = static_cast<int32_t>(logPg);
      p.Fg = static_cast<int32_t>(Fg);
      p.include_self = static_cast<int32_t>(self);
      p.inv = 1.f / static_cast<float>(Fg + self);
    } else {
      const int64_t target = pd_.has("dw_target_wg") ? pd_.geti("dw_target_wg") : 512;
      const int64_t minkps = pd_.has("dw_min_kps") ? pd_.geti("dw_min_kps") : 4;
      const int64_t fold = pd_.has("dw_fold") ? pd_.geti("dw_fold") : 1;
      TORCH_CHECK(target >= 1 && minkps >= 1 && (fold == 0 || fold == 1), pd_.name(),
                  ": dw_target_wg / dw_min_kps must be positive, dw_fold 0 or 1");
      tr_plan_stored(p, target, minkps, fold == 1);
    }
    p.part = pd_.zeros_ptr<float>(static_cast<int64_t>(p.S) * P * Q, torch::kFloat32);
    p.G = G;
    p.X = X;
    probs.push_back(p);
    return probs.back();
  }

  // the next flat segment, at offset off: the weight of problem p (sums its slabs; optional fm
  // shadows), or a vector of n elements summed from S partials
  void add_seg(int64_t off, const TrDwProb& p, const uint16_t* sh, const uint16_t* shT) {
    TrSeg& g = next_seg();
    g.off = off;
    g.n = static_cast<int64_t>(p.P) * p.Q;
    g.part = p.part;
    g.S = p.S;
    g.rows = p.P;
    g.cols = p.Q;
    g.sh = const_cast<uint16_t*>(sh);
    g.shT = const_cast<uint16_t*>(shT);
  }
  void add_vec_seg(int64_t off, int64_t n, const float* part, int64_t S) {
    TrSeg& g = next_seg();
    g.off = off;
    g.n = n;
    g.part = part;
    g.S = static_cast<int32_t>(S);
    g.rows = 1;
  }
  void layout_segs() {
    opt.nblk = tr_seg_layout(opt.seg, opt.nseg, true);
    TORCH_CHECK(opt.nblk >= 1, pd_.name(), ": weight segments need rows % 8, cols % 32");
  }

  // state, hyper-parameters and loss hand-off of the optimizer from the keys every optimizing
  // plan shares: flat (n parameters, then padding), grad, m, v, step, lr, beta1, beta2, eps,
  // weight_decay, opt_kind, loss_acc, loss_out and the head's second statistic (rank_stat:
  // mrr_sum, the reciprocal ranks of a pair model; else counts: tp, fp, fn)
  void fill_opt(int64_t n, const float* head_part, int64_t nhead, bool rank_stat) {
    torch::Tensor flat = pd_.T("flat");
    pd_.need(flat, torch::kFloat32, -1, "flat");
    const int64_t nbuf = flat.numel();
    TORCH_CHECK(n <= nbuf, pd_.name(), ": offsets must lie inside the flat buffer");
    opt.n = n;
    opt.p = flat.data_ptr<float>();
    opt.g = pd_.f32("grad", nbuf);
    opt.m = pd_.f32("m", nbuf);
    opt.v = pd_.f32("v", nbuf);
    TrOptCore& c = opt.c;
    c.step = pd_.ptr<int64_t>("step", torch::kInt64, 1);
    c.lr = static_cast<float>(pd_.getf("lr"));
    c.b1 = static_cast<float>(pd_.getf("beta1"));
    c.b2 = static_cast<float>(pd_.getf("beta2"));
    c.eps = static_cast<float>(pd_.getf("eps"));
    c.wd = static_cast<float>(pd_.getf("weight_decay"));
    c.grad_scale = 1.f;
    c.kind = static_cast<int32_t>(pd_.geti("opt_kind"));
    c.head_part = head_part;
    c.nhead = static_cast<int32_t>(nhead);
    c.loss_acc = pd_.f32("loss_acc", 1);
    c.loss_out = pd_.f32("loss_out", 1);
    if (rank_stat) c.stat_f = pd_.f32("mrr_sum", 1);
    else c.counts = reinterpret_cast<uint32_t*>(pd_.i32("counts", 3));
  }

  // plan key dw_opt_fuse: the launch of every problem carries the optimizer, where the plan
  // allows it and tr_dw_fuse finds a place for every segment
  void try_fuse(bool allowed) {
    TrDwGrid grid;
    TrDwLaunch L = launch_of(all(), false, grid);
    if (!fuse_key_ || !allowed || !tr_dw_fuse(L, opt, fopt_)) return;
    sync_ = pd_.zeros(static_cast<int64_t>(fopt_.nsync) * kTrSyncLine, torch::kInt32);
    fopt_.sync = reinterpret_cast<uint32_t*>(sync_.data_ptr<int32_t>());
    fused_ = true;
  }
  bool fused() const { return fused_; }
  // the status word of the hand-off state (0: every wait of every fused launch so far was met);
  // synchronises
  int64_t fuse_error() const { return sync_.defined() ? sync_[kTrSyncLine].item<int64_t>() : 0; }

  std::vector<int64_t> all() const {
    std::vector<int64_t> w(probs.size());
    for (size_t i = 0; i < w.size(); ++i) w[i] = static_cast<int64_t>(i);
    return w;
  }

  // dW of the given problems, one launch: routed problems first, the others grouped.  fuse (a
  // fused() plan, every problem in the plan's order): the launch also runs the optimizer, what
  // tr_opt mode 2 with grad_scale would do after it
  void launch(const std::vector<int64_t>& which, c10::optional<torch::Tensor> prof, bool fuse, double grad_scale) {
    const c10::DeviceGuard g(pd_.device());
    TrDwGrid grid;
    TrDwLaunch L = launch_of(which, fuse, grid);
    if (fuse) L.opt.c.grad_scale = static_cast<float>(grad_scale);
    if (prof.has_value()) {
      pd_.need(*prof, torch::kInt64, -1, "prof");
      L.prof = reinterpret_cast<long long*>(prof->data_ptr<int64_t>());
    }
    tree_ok(eh_tr_dw(&L, cur_stream()), fuse ? "tr_dw+opt" : "tr_dw");
  }
  // workgroups of the launch of the given problems (fuse: with its trailing optimizer blocks)
  int64_t blocks(const std::vector<int64_t>& which, bool fuse) const {
    TrDwGrid grid;
    launch_of(which, fuse, grid);
    return grid.ndw + grid.ntrail;
  }
  std::vector<int64_t> splits() const {
    std::vector<int64_t> s;
    for (const auto& p : probs) s.push_back(p.S);
    return s;
  }
  // slabs each problem sums inside its blocks (0: none, its S slabs go through `part`)
  std::vector<int64_t> folds() const {
    std::vector<int64_t> f;
    for (const auto& p : probs) f.push_back(p.F);
    return f;
  }
  void set_lr(double lr) { opt.c.lr = fopt_.c.lr = static_cast<float>(lr); }
  // the flat fp32 gradient the reduce writes and the optimizer reads (e.g. a view of the xGMI
  // all-reduce's IPC input region, so the all-reduce runs in place there); exact: of opt.n
  // elements, else at least as many
  void set_grad(torch::Tensor g, bool exact) {
    pd_.need(g, torch::kFloat32, exact ? opt.n : -1, "grad");
    TORCH_CHECK(g.numel() >= opt.n, "grad has ", g.numel(), " elements, fewer than the ", opt.n, " parameters");
    grad_ = g;
    opt.g = g.data_ptr<float>();
  }

 private:
  PlanDict& pd_;
  int route_impl_;
  bool fuse_key_, fused_ = false;
  TrDwOpt fopt_{};      // the optimizer of the fused launch of all(); set_lr keeps its lr equal to opt's
  torch::Tensor sync_;  // its hand-off state (TrDwOpt::sync)
  torch::Tensor grad_;

  TrSeg& next_seg() {
    TORCH_CHECK(opt.nseg < kTrMaxSegs, pd_.name(), ": too many optimizer segments");
    return opt.seg[opt.nseg++] = TrSeg{};
  }

  // the laid-out launch of the given problems
  TrDwLaunch launch_of(const std::vector<int64_t>& which, bool fuse, TrDwGrid& grid) const {
    TrDwLaunch L{};
    L.route_impl = route_impl_;
    bool every = which.size() == probs.size();
    for (size_t k = 0; k < which.size(); ++k) {
      const int64_t i = which[k];
      TORCH_CHECK(i >= 0 && i < (int64_t)probs.size(), "dw: problem index out of range");
      every = every && i == (int64_t)k;
      if (probs[i].route) {
        TORCH_CHECK(L.nroute < 2, "dw: at most two routed problems per launch");
        L.route[L.nroute++] = probs[i];
      } else {
        TORCH_CHECK(L.plain.n < kTrMaxProbs, "dw: too many problems");
        L.plain.p[L.plain.n++] = probs[i];
      }
    }
    if (fuse) {
      TORCH_CHECK(fused_ && every, pd_.name(),
                  ": the optimizer runs in the dW launch of every problem, in the plan's order, of a fused() plan only");
      L.opt = fopt_;
      L.fuse = 1;
    }
    TORCH_CHECK(tr_dw_layout(L, grid), pd_.name(), ": the dW launch is not one the kernel takes");
    return L;
  }
};

class TreePlan : private PlanDict {
 public:
  explicit TreePlan(py::dict d) : PlanDict(d, "TreePlan") {
    L_ = geti("L");
    B_ = geti("B");
    TORCH_CHECK(L_ >= 1 && L_ <= 3, "TreePlan: 1..3 hops");
    TORCH_CHECK(B_ > 0 && B_ % 32 == 0, "TreePlan: batch must be a positive multiple of 32");
    F_ = getv("F");
    logP_ = getv("logP");  // logP[k] for levels k = 1..L-1 (index 0 unused)
    masks_ = getv("masks");
    dims_ = getv("H");     // padded conv widths H_0..H_{L-1}
    TORCH_CHECK((int)F_.size() == L_ + 1 && (int)masks_.size() == L_ + 1 && (int)logP_.size() >= L_ &&
                    (int)dims_.size() == L_,
                "TreePlan: F/masks need L+1 entries (index 0 unused), logP L, H L");
    D_ = geti("D");
    E_ = geti("E");
    C_ = geti("C");
    C_real_ = geti("C_real");
    self_ = geti("include_self");
    for (int k = 1; k < L_; ++k) TORCH_CHECK(logP_[k] >= 4 && (1 << logP_[k]) > F_[k], "TreePlan: slot group too small");
    for (int k = 0; k < L_; ++k) TORCH_CHECK(dims_[k] % 64 == 0, "TreePlan: conv widths must be padded to 64");
    TORCH_CHECK(D_ % 16 == 0 && E_ % 32 == 0 && C_ % 32 == 0 && C_real_ <= C_, "TreePlan: padded dims");
    // level sizes M[k] = B * P1 * ... * Pk
    M_.assign(L_, 0);
    M_[0] = B_;
    for (int k = 1; k < L_; ++k) M_[k] = M_[k - 1] << logP_[k];
    fill_graph_tree(*this, graph_, tree_, L_ > 1 ? F_[1] : 0, L_ > 2 ? F_[2] : 0, L_ > 1 ? logP_[1] : 0,
                    L_ > 2 ? logP_[2] : 0, static_cast<uint32_t>(masks_[1]),
                    L_ > 2 ? static_cast<uint32_t>(masks_[2]) : 0u);
    build_fwd();
    build_comb();
    build_head();
    build_dw();
    build_opt();
    // the optimizer in the dW launch of all problems, unless the step is pipelined (its
    // optimizer launch carries the next batch's gather)
    dw_.try_fuse(!pipeline_ok());
  }

  bool fused() const { return dw_.fused(); }
  int64_t fuse_error() const { return dw_.fuse_error(); }

  void sample() {
    const c10::DeviceGuard g(device());
    tree_ok(eh_tr_sample(&sample_, cur_stream()), "tr_sample");
  }

  // gemm_only (pipelined step): layer 0 from the A rows the previous optimizer launch's
  // gather blocks wrote (opt(..., with_gather=True))
  void fwd(c10::optional<torch::Tensor> prof, bool gemm_only) {
    const c10::DeviceGuard g(device());
    TORCH_CHECK(!gemm_only || pipeline_ok(), "TreePlan: no pipelined forward for this plan");
    TrFwdArgs a0 = fwd0_;
    if (prof.has_value()) {
      need(*prof, torch::kInt64, (fwd0_.M / (gemm_only ? 64 : bm0_)) * 8, "prof");
      a0.prof = reinterpret_cast<long long*>(prof->data_ptr<int64_t>());
    }
    tree_ok(eh_tr_fwd(&a0, gemm_only ? 3 : (L_ == 1 ? 1 : 0), feat_fp32_, bm0_, cur_stream()), "tr_fwd");
    if (L_ == 3) tree_ok(eh_tr_fwd(&fwd1_, 2, 0, bm1_, cur_stream()), "tr_fwd(inner)");
  }

  // with_sample: extra blocks of the launch draw the next step's batch
  void head(c10::optional<torch::Tensor> prof, bool with_sample) {
    const c10::DeviceGuard g(device());
    TrHeadArgs a = head_;
    if (with_sample) {
      a.smp = sample_;
      a.nsample = static_cast<int32_t>((sample_.M + kTrHeadSampleRows - 1) / kTrHeadSampleRows);
    }
    if (prof.has_value()) {
      need(*prof, torch::kInt64, (B_ / kTrHeadRows) * 8, "prof");
      a.prof = reinterpret_cast<long long*>(prof->data_ptr<int64_t>());
    }
    tree_ok(eh_tr_head(&a, B_, cur_stream()), "tr_head");
  }

  void bwd() {
    if (L_ != 3) return;
    const c10::DeviceGuard g(device());
    tree_ok(eh_tr_bwd(&bwd1_, cur_stream()), "tr_bwd");
  }

  // DwPlan::launch; fuse: what opt(2, grad_scale) would do after it runs in the launch
  void dw(std::vector<int64_t> which, c10::optional<torch::Tensor> prof, bool fuse, double grad_scale) {
    dw_.launch(which, prof, fuse, grad_scale);
  }
  // workgroups of the dW launch of every problem (fuse: with its trailing optimizer blocks)
  int64_t dw_blocks(bool fuse) const { return dw_.blocks(dw_.all(), fuse); }

  std::vector<int64_t> problems(bool route) const {
    std::vector<int64_t> out;
    for (size_t i = 0; i < dw_.probs.size(); ++i)
      if (static_cast<bool>(dw_.probs[i].route) == route) out.push_back(static_cast<int64_t>(i));
    return out;
  }

  // mode 0 reduce, 1 optimizer, 2 fused, 3 shadows only
  // with_sample: modes 1/2 also draw the next step's batch (extra blocks of the launch)
  // with_gather: extra blocks gather the NEXT step's layer-0 inputs (the tree the head's
  // sampler drew) into A0_kt and A0_rows, so that step's forward is GEMM-only
  void opt(int64_t mode, double grad_scale, bool with_sample, bool with_gather) {
    const c10::DeviceGuard g(device());
    TORCH_CHECK(!with_gather || pipeline_ok(), "TreePlan: no pipelined gather for this plan");
    TrOptArgs a = dw_.opt;
    a.c.grad_scale = static_cast<float>(grad_scale);
    if (!with_sample) a.nsample = 0;
    if (with_gather) {
      a.gat = fwd0_;
      a.ngather = static_cast<int32_t>(fwd0_.M / 32);
      a.gat_fp32 = feat_fp32_;
      static const int first = [] {
        const char* e = std::getenv("EULER_AMD_GATHER_FIRST");
        return e ? std::atoi(e) : 1;
      }();
      a.gather_first = first;
      static const int tpb = [] {
        const char* e = std::getenv("EULER_AMD_OPT_TPB");
        return e ? std::atoi(e) : 4;
      }();
      a.opt_tpb = tpb;
    }
    tree_ok(eh_tr_opt(&a, static_cast<int>(mode), cur_stream()), "tr_opt");
  }

  // the pipelined step applies: 2 hops, the 64-row layer-0 kernel, A0_rows given, sibling
  // groups of at most 32 rows (one gather tile)
  bool pipeline_ok() const {
    return L_ == 2 && fwd0_.a_rows != nullptr && !cached_ && bm0_ <= 64 && logP_[1] <= 5 && D_ % 64 == 0 &&
           fwd0_.M % 64 == 0 && dims_[0] <= 256 &&
           eh_tr_gather32_lds(static_cast<int>(D_), static_cast<int>(fwd0_.FL)) <= 64 * 1024;
  }

  // split-K reduce (mode 0) of a subset of the flat segments (data-parallel buckets);
  // head_stats: this launch also reduces the head's loss / F1 partials
  void opt_segments(int64_t mode, std::vector<int64_t> segs, bool head_stats) {
    TORCH_CHECK(mode == 0, "opt_segments: only the reduce (mode 0) runs on a segment subset");
    TORCH_CHECK(!segs.empty() && (int64_t)segs.size() <= dw_.opt.nseg, "opt_segments: bad segment list");
    const c10::DeviceGuard g(device());
    TrOptArgs a = dw_.opt;
    a.nseg = 0;
    for (int64_t k : segs) {
      TORCH_CHECK(k >= 0 && k < dw_.opt.nseg, "opt_segments: segment index out of range");
      a.seg[a.nseg++] = dw_.opt.seg[k];
    }
    a.nblk = tr_seg_layout(a.seg, a.nseg, true);
    a.nsample = 0;
    if (!head_stats) a.c.nhead = 0;
    tree_ok(eh_tr_opt(&a, 0, cur_stream()), "tr_opt(segments)");
  }

  int64_t fwd_blocks() const { return fwd0_.M / bm0_; }
  void set_lr(double lr) { dw_.set_lr(lr); }
  void set_grad(torch::Tensor g) { dw_.set_grad(g, true); }
  // bf16 gradient buffer for the data-parallel hand-off (None: fp32 grad)
  void set_grad16(c10::optional<torch::Tensor> g16) {
    if (!g16.has_value()) {
      dw_.opt.g16 = nullptr;
      g16_ = torch::Tensor();
      return;
    }
    need(*g16, torch::kBFloat16, dw_.opt.n, "grad16");
    g16_ = *g16;
    dw_.opt.g16 = reinterpret_cast<uint16_t*>(g16_.data_ptr());
  }
  int64_t num_problems() const { return (int64_t)dw_.probs.size(); }
  // blocks of the routed problem i in a dw launch (the prof rows it stamps)
  int64_t route_blocks(int64_t i) const { return dw_.probs.at(i).route ? dw_.blocks({i}, false) : 0; }
  std::vector<int64_t> splits() const { return dw_.splits(); }
  std::vector<int64_t> folds() const { return dw_.folds(); }

 private:
  int L_, B_, D_, E_, C_, C_real_, self_;
  int feat_fp32_ = 0, bm0_ = 32, bm1_ = 32;
  bool cached_ = false;
  std::vector<int64_t> F_, logP_, masks_, dims_, M_;
  TrGraph graph_{};
  TrTree tree_{};
  TrSampleArgs sample_{};
  TrFwdArgs fwd0_{}, fwd1_{};
  TrHeadArgs head_{};
  TrBwdArgs bwd1_{};
  DwPlan dw_{*this};  // conv layers 0..L-1, then fc and out_fc
  torch::Tensor roots_cur_;  // the forward's copy of the batch's roots (read by the head)
  torch::Tensor g16_;

  int64_t Hin(int k) const { return k == 0 ? D_ : dims_[k - 1]; }

  void build_fwd() {
    // "fwd_features" (+ "fwd_nodes" / "fwd_leaf" cache positions): the forward gathers from
    // a feature cache filled by the sharded-feature exchange instead of the whole table
    const bool cached = has("fwd_features");
    torch::Tensor x = cached ? T("fwd_features") : T("features");
    feat_fp32_ = !need_bf16_or_f32(x, -1, "features");
    TORCH_CHECK(x.dim() == 2 && x.size(1) == D_, "features must be [N, D] with D padded to 16");
    TORCH_CHECK(cached || x.size(0) == graph_.num_rows, "features must have one row per graph row");
    const int lv = L_ - 1;           // level of layer 0's target rows
    const int64_t M = M_[lv];
    TrSampleArgs& sm = sample_;
    sm.g = graph_;
    sm.tr = tree_;
    sm.M = M;
    sm.lv = lv;
    sm.FL = static_cast<int32_t>(F_[L_]);
    sm.mL = static_cast<uint32_t>(masks_[L_]);
    sm.hopL = L_;
    sm.roots = i32("roots", B_);
    sm.nodes = i32("nodes", M);
    sm.leaf = i32("leaf", M * sm.FL);
    TrFwdArgs& a = fwd0_;
    a.x = x.data_ptr();
    a.D = D_;
    a.M = M;
    a.FL = sm.FL;
    a.include_self = self_;
    a.inv_leaf = 1.f / static_cast<float>(a.FL + self_);
    cached_ = cached;
    a.nodes = cached ? i32("fwd_nodes", M) : sm.nodes;
    a.leaf = cached ? i32("fwd_leaf", M * sm.FL) : sm.leaf;
    a.roots_in = sm.roots;
    roots_cur_ = zeros(B_, torch::kInt32);
    a.roots_cur = roots_cur_.data_ptr<int32_t>();
    a.B = B_;
    a.step = ptr<int64_t>("step", torch::kInt64, 1);
    a.rng = ptr<int64_t>("rng", torch::kInt64, 2);
    if (L_ == 1) {
      a.a_next = bf("A0", B_ * 2 * D_);  // the head's input rows [B][2D]
      bm0_ = 32;
      return;
    }
    a.W = bf("W0_sh", dims_[0] * 2 * D_);
    a.H = static_cast<int32_t>(dims_[0]);
    a.a_kt = bf("A0_kt", M * 2 * D_);
    a.mask = i32_as_u32("mask0", (M / 32) * dims_[0]);
    a.logPg = static_cast<int32_t>(logP_[lv]);
    a.Fg = static_cast<int32_t>(F_[lv]);
    a.inv_grp = 1.f / static_cast<float>(a.Fg + self_);
    a.a_next = bf("A1", M_[lv - 1] * 2 * dims_[0]);
    a.a_rows = has("A0_rows") ? bf("A0_rows", M * 2 * D_) : nullptr;
    bm0_ = (1 << a.logPg) > 32 ? (1 << a.logPg) : 32;
    if (has("fwd_bm")) bm0_ = std::max<int>(bm0_, static_cast<int>(geti("fwd_bm")));
    TORCH_CHECK(bm0_ == 32 || bm0_ == 64 || bm0_ == 128, "TreePlan: fwd rows per block must be 32, 64 or 128");
    TORCH_CHECK(M % bm0_ == 0, "TreePlan: target rows must be a multiple of the fwd block rows");
    if (L_ == 3) {
      TrFwdArgs& b = fwd1_;
      b.x = T("A1").data_ptr();
      b.D = static_cast<int32_t>(dims_[0]);
      b.M = M_[1];
      b.include_self = self_;
      b.W = bf("W1_sh", dims_[1] * 2 * dims_[0]);
      b.H = static_cast<int32_t>(dims_[1]);
      b.a_kt = bf("A1_kt", M_[1] * 2 * dims_[0]);
      b.mask = i32_as_u32("mask1", (M_[1] / 32) * dims_[1]);
      b.logPg = static_cast<int32_t>(logP_[1]);
      b.Fg = static_cast<int32_t>(F_[1]);
      b.inv_grp = 1.f / static_cast<float>(b.Fg + self_);
      b.a_next = bf("A2", B_ * 2 * dims_[1]);
      bm1_ = (1 << b.logPg) > 32 ? (1 << b.logPg) : 32;
    }
  }

  // fc and out_fc combined for the head (TrCombArgs): rebuilt every step by extra blocks
  // of the first forward launch from the fp32 masters in the flat buffer
  void build_comb() {
    torch::Tensor flat = T("flat");
    need(flat, torch::kFloat32, -1, "flat");
    std::vector<int64_t> off = getv("offsets");  // L convs, fc W, fc b, out W, end
    TORCH_CHECK((int)off.size() == L_ + 4 && off.back() == flat.numel(), "TreePlan: offsets must cover the flat buffer");
    const int64_t H = dims_[L_ - 1];
    TORCH_CHECK(off[L_ + 1] - off[L_] == (int64_t)E_ * H && off[L_ + 3] - off[L_ + 2] == (int64_t)C_ * E_,
                "TreePlan: fc / out_fc segments do not match E, H, C");
    TORCH_CHECK(C_ % 16 == 0 && H % 16 == 0 && E_ % 32 == 0, "TreePlan: combination tiles need C % 16, H % 16, E % 32");
    float* base = flat.data_ptr<float>();
    TrCombArgs& c = fwd0_.comb;
    c.bfc = base + off[L_ + 1];
    c.wout = base + off[L_ + 2];
    c.wout_sh = bf("Wout_sh", (int64_t)C_ * E_);
    c.wfcT_sh = bf("Wfc_shT", (int64_t)E_ * H);
    c.C = C_;
    c.E = E_;
    c.H = static_cast<int32_t>(H);
    c.Wc = zeros_ptr<uint16_t>((int64_t)C_ * H, torch::kBFloat16);
    c.WcT = zeros_ptr<uint16_t>((int64_t)C_ * H, torch::kBFloat16);
    c.bc = zeros_ptr<float>(C_, torch::kFloat32);
    fwd0_.ncomb = 1;
  }

  uint32_t* i32_as_u32(const std::string& k, int64_t numel) { return reinterpret_cast<uint32_t*>(i32(k, numel)); }

  void build_head() {
    const int last = L_ - 1;
    const int64_t Hin2 = 2 * Hin(last), H = dims_[last];
    TrHeadArgs& a = head_;
    a.A = bf("A" + std::to_string(last), B_ * Hin2);
    a.Hin2 = static_cast<int32_t>(Hin2);
    a.H = static_cast<int32_t>(H);
    a.E = E_;
    a.C = C_;
    a.C_real = C_real_;
    a.W = bf("W" + std::to_string(last) + "_sh", H * Hin2);
    a.WT = L_ > 1 ? bf("W" + std::to_string(last) + "_shT", H * Hin2) : nullptr;
    a.Wfc = bf("Wfc_sh", (int64_t)E_ * H);
    a.WfcT = bf("Wfc_shT", (int64_t)E_ * H);
    a.Wout = bf("Wout_sh", (int64_t)C_ * E_);
    a.WoutT = bf("Wout_shT", (int64_t)C_ * E_);
    a.bfc = f32("bfc", E_);
    a.Wc = fwd0_.comb.Wc;
    a.WcT = fwd0_.comb.WcT;
    a.bc = fwd0_.comb.bc;
    a.roots = fwd0_.roots_cur;
    const int mode = static_cast<int>(geti("label_mode"));
    torch::Tensor lab = T("labels");
    need_any(lab, "labels");
    TORCH_CHECK(mode >= 0 && mode <= 2, "label_mode must be 0, 1 or 2");
    // "label_rows": a label table over other rows than the graph's (the row-sharded trainer
    // hands the head a [B] table of the batch's labels with roots = 0 .. B-1)
    const int64_t lrows = has("label_rows") ? geti("label_rows") : graph_.num_rows;
    if (mode == 0) {
      TORCH_CHECK(lab.scalar_type() == torch::kInt16 && lab.numel() == lrows, "TreePlan: labels int16 [N]");
    } else if (mode == 1) {
      TORCH_CHECK(lab.scalar_type() == torch::kInt32 && lab.numel() == lrows, "TreePlan: labels int32 [N]");
    } else {
      TORCH_CHECK(lab.scalar_type() == torch::kBFloat16 && lab.numel() == lrows * C_, "TreePlan: labels bf16 [N, C]");
    }
    a.labels = lab.data_ptr();
    a.label_mode = mode;
    // "loss": 0 = per-column sigmoid cross-entropy (default), 1 = row softmax cross-entropy
    const int loss = has("loss") ? static_cast<int>(geti("loss")) : kTrLossSigmoid;
    TORCH_CHECK(loss == kTrLossSigmoid || loss == kTrLossSoftmax, "TreePlan: loss must be 0 (sigmoid) or 1 (softmax)");
    TORCH_CHECK(loss != kTrLossSoftmax || C_ <= kTrSoftmaxMaxC, "TreePlan: the softmax head holds one 16-column ",
                "logits tile per wave of its block: at most ", kTrSoftmaxMaxC, " (padded) classes, got ", C_);
    a.loss = loss;
    a.inv_scale = loss == kTrLossSoftmax ? 1.f / static_cast<float>(B_) : 1.f / static_cast<float>(B_ * C_real_);
    a.A_kt = bf("A" + std::to_string(last) + "_kt", B_ * Hin2);
    a.h_kt = bf("h_kt", B_ * H);
    a.emb_kt = bf("emb_kt", (int64_t)B_ * E_);
    a.dlog_kt = bf("dlog_kt", (int64_t)B_ * C_);
    a.demb_kt = bf("demb_kt", (int64_t)B_ * E_);
    a.g_kt = bf("g_kt", B_ * H);
    a.dA = L_ > 1 ? f32("dA" + std::to_string(last), B_ * Hin2) : nullptr;
    const int64_t nblk = B_ / kTrHeadRows;
    a.dbfc_part = zeros_ptr<float>(nblk * E_, torch::kFloat32);
    a.head_part = zeros_ptr<float>(nblk * 4, torch::kFloat32);
    a.prof = nullptr;
    const size_t lds = eh_tr_head_lds(a.Hin2, a.H, a.E, a.C, mode);
    TORCH_CHECK(lds + (loss == kTrLossSoftmax ? eh_tr_head_softmax_lds() : 0) <= 160 * 1024 - 64,
                "TreePlan: head tile does not fit in LDS (", lds, " bytes)");
    if (L_ == 3) {
      TrBwdArgs& b = bwd1_;
      b.dA = f32("dA2", B_ * 2 * dims_[1]);
      b.mask = i32_as_u32("mask1", (M_[1] / 32) * dims_[1]);
      b.WT = bf("W1_shT", dims_[1] * 2 * dims_[0]);
      b.Hk = static_cast<int32_t>(dims_[1]);
      b.K2out = static_cast<int32_t>(2 * dims_[0]);
      b.M = M_[1];
      b.logPg = static_cast<int32_t>(logP_[1]);
      b.Fg = static_cast<int32_t>(F_[1]);
      b.include_self = self_;
      b.inv = 1.f / static_cast<float>(b.Fg + self_);
      b.dA_out = f32("dA1", M_[1] * 2 * dims_[0]);
    }
  }

  void build_dw() {
    for (int k = 0; k < L_; ++k) {
      const int64_t P = dims_[k], Q = 2 * Hin(k);
      const std::string ks = std::to_string(k);
      if (k < L_ - 1) {
        const int lvl = L_ - 1 - k;  // target level of layer k
        dw_.add(P, Q, M_[lvl], nullptr, bf("A" + ks + "_kt", M_[lvl] * Q),
                f32("dA" + std::to_string(k + 1), M_[lvl - 1] * 2 * P), i32_as_u32("mask" + ks, (M_[lvl] / 32) * P),
                logP_[lvl], F_[lvl], self_);
      } else {
        dw_.add(P, Q, B_, bf("g_kt", B_ * P), bf("A" + ks + "_kt", B_ * Q), nullptr, nullptr, 0, 0, 0);
      }
    }
    const int64_t H = dims_[L_ - 1];
    dw_.add(E_, H, B_, bf("demb_kt", (int64_t)B_ * E_), bf("h_kt", B_ * H), nullptr, nullptr, 0, 0, 0);
    dw_.add(C_, E_, B_, bf("dlog_kt", (int64_t)B_ * C_), bf("emb_kt", (int64_t)B_ * E_), nullptr, nullptr, 0, 0, 0);
  }

  void build_opt() {
    std::vector<int64_t> off = getv("offsets");  // L convs, fc W, fc b, out W, end
    TORCH_CHECK((int)off.size() == L_ + 4 && off.back() == T("flat").numel(),
                "TreePlan: offsets must cover the flat buffer");
    // segments: conv weights [H_k][2 Hin_k] (+ transposed shadows where a backward GEMM
    // reads them), fc W [E][H], fc bias [E] (vector: the head's per-block sums), out W [C][E]
    const int64_t H = dims_[L_ - 1], nhead = B_ / kTrHeadRows;
    for (int k = 0; k < L_ + 3; ++k) {
      const int64_t n = off[k + 1] - off[k];
      if (k == L_ + 1) {
        dw_.add_vec_seg(off[k], n, head_.dbfc_part, nhead);
        continue;
      }
      const TrDwProb& p = dw_.probs[k < L_ + 1 ? k : L_ + 1];
      TORCH_CHECK(n == (int64_t)p.P * p.Q, "TreePlan: flat segment ", k, " does not match its dW problem");
      if (k < L_) {
        const std::string ks = std::to_string(k);
        dw_.add_seg(off[k], p, bf("W" + ks + "_sh", n), k >= 1 ? bf("W" + ks + "_shT", n) : nullptr);
      } else if (k == L_) {
        dw_.add_seg(off[k], p, bf("Wfc_sh", (int64_t)E_ * H), bf("Wfc_shT", (int64_t)E_ * H));
      } else {
        dw_.add_seg(off[k], p, bf("Wout_sh", (int64_t)C_ * E_), bf("Wout_shT", (int64_t)C_ * E_));
      }
    }
    dw_.layout_segs();
    dw_.fill_opt(off.back(), head_.head_part, nhead, false);
    dw_.opt.smp = sample_;
    dw_.opt.nsample = static_cast<int32_t>((sample_.M + 63) / 64);
  }
};

// Layer 0 of a 2-hop SAGE tower over GIVEN roots (pair / unsupervised models, where the
// roots are a node's sampled positive and negatives): the tree sampler draws hop 1 and the
// leaves from the roots in `roots_in`, tr_fwd (mode 0) gathers the leaf rows, runs the
// layer-0 GEMM + ReLU and the tree mean of hop 1, producing the last conv's input rows
// A1 = [h0(root) | mean h0(hop-1 nbrs)] [R][2H0] bf16.  The backward takes dA1 (fp32),
// routes it through the tree and the ReLU bits inside the split-K dW kernel and reduces
// the partials into the fp32 gradient of W0.  The rest of the tower (last conv, fc, loss)
// is ordinary torch on [R][2H0] rows (euler_amd/models/sage_tower.py).
class TowerPlan : private PlanDict {
 public:
  explicit TowerPlan(py::dict d) : PlanDict(d, "TowerPlan") {
    R_ = geti("R");
    F1_ = geti("F1");
    F2_ = geti("F2");
    logP_ = geti("logP");
    D_ = geti("D");
    H_ = geti("H");
    self_ = geti("include_self");
    TORCH_CHECK(R_ > 0 && R_ % 32 == 0, "TowerPlan: roots must be a positive multiple of 32");
    TORCH_CHECK(logP_ >= 4 && (1 << logP_) > F1_ && F1_ >= 1 && F2_ >= 1, "TowerPlan: slot group too small");
    TORCH_CHECK(D_ % 16 == 0 && H_ % 64 == 0, "TowerPlan: padded dims (D % 16, H % 64)");
    M_ = R_ << logP_;
    // graph + tree; root_rows is used when the roots are drawn in the sampler (PairPlan), not
    // when they are given
    fill_graph_tree(*this, g_, tree_, F1_, 0, logP_, 0, static_cast<uint32_t>(geti("mask1")), 0u);
    tree_.root_in = i32("roots_in", R_);
    // sampler: level-1 slots (hop 1 of each root) and their F2 leaves
    sample_.g = g_;
    sample_.tr = tree_;
    sample_.M = M_;
    sample_.lv = 1;
    sample_.FL = static_cast<int32_t>(F2_);
    sample_.mL = static_cast<uint32_t>(geti("mask2"));
    sample_.hopL = 2;
    sample_.roots = has("roots_out") ? ptr<int32_t>("roots_out", torch::kInt32, R_) : owned_i32(R_);
    sample_.nodes = ptr<int32_t>("nodes", torch::kInt32, M_);
    sample_.leaf = ptr<int32_t>("leaf", torch::kInt32, M_ * F2_);
    // layer 0 (mode 0)
    torch::Tensor x = T("features");
    feat_fp32_ = !need_bf16_or_f32(x, -1, "features");
    TORCH_CHECK(x.dim() == 2 && x.size(1) == D_ && x.size(0) == g_.num_rows, "features must be [N, D]");
    TrFwdArgs& a = fwd_;
    a.x = x.data_ptr();
    a.D = static_cast<int32_t>(D_);
    a.M = M_;
    a.FL = static_cast<int32_t>(F2_);
    a.include_self = static_cast<int32_t>(self_);
    a.inv_leaf = 1.f / static_cast<float>(F2_ + self_);
    a.nodes = sample_.nodes;
    a.leaf = sample_.leaf;
    a.roots_in = sample_.roots;
    a.roots_cur = owned_i32(R_);
    a.B = static_cast<int32_t>(R_);
    a.step = nullptr;
    a.rng = ptr<int64_t>("rng", torch::kInt64, 2);
    a.W = ptr<uint16_t>("W0_sh", torch::kBFloat16, H_ * 2 * D_);
    a.H = static_cast<int32_t>(H_);
    a.a_kt = ptr<uint16_t>("A0_kt", torch::kBFloat16, M_ * 2 * D_);
    a.mask = reinterpret_cast<uint32_t*>(ptr<int32_t>("mask0", torch::kInt32, (M_ / 32) * H_));
    a.logPg = static_cast<int32_t>(logP_);
    a.Fg = static_cast<int32_t>(F1_);
    a.inv_grp = 1.f / static_cast<float>(F1_ + self_);
    a.a_next = ptr<uint16_t>("A1", torch::kBFloat16, R_ * 2 * H_);
    a.ncomb = 0;
    bm_ = (1 << logP_) > 32 ? (1 << logP_) : 32;
    TORCH_CHECK(bm_ <= 128 && M_ % bm_ == 0, "TowerPlan: sibling groups of at most 128 rows");
    // routed dW of W0 (G routed from dA1 through the tree and the ReLU bits)
    const TrDwProb& p = dw_.add(H_, 2 * D_, M_, nullptr, a.a_kt, ptr<float>("dA1", torch::kFloat32, R_ * 2 * H_),
                                a.mask, logP_, F1_, self_);
    // reduce into the fp32 gradient / bf16 shadow of the fp32 master (one weight segment)
    TrOptArgs& o = dw_.opt;
    float* w = ptr<float>("W0", torch::kFloat32, H_ * 2 * D_);
    o.p = o.m = o.v = w;
    o.g = ptr<float>("gW0", torch::kFloat32, H_ * 2 * D_);
    o.n = H_ * 2 * D_;
    dw_.add_seg(0, p, a.W, nullptr);
    dw_.layout_segs();
    o.c.step = zeros_ptr<int64_t>(1, torch::kInt64);
    o.c.head_part = o.c.loss_acc = o.c.loss_out = zeros_ptr<float>(8, torch::kFloat32);
    o.c.kind = 2;
  }

  // the tower's backward hands a gradient to torch's optimizer: no optimizer in its dW launch
  // (dw_opt_fuse is accepted and checked; bwd() is a reduce into gW0, mode 0, which keeps tr_opt)
  bool fused() const { return dw_.fused(); }
  int64_t fuse_error() const { return dw_.fuse_error(); }

  // refresh the bf16 fm shadow of W0 from the fp32 master (call after each update)
  void shadow() {
    const c10::DeviceGuard g(device());
    tree_ok(eh_tr_opt(&dw_.opt, 3, cur_stream()), "tower shadow");
  }
  void sample() {
    const c10::DeviceGuard g(device());
    tree_ok(eh_tr_sample(&sample_, cur_stream()), "tower sample");
  }
  void fwd() {
    const c10::DeviceGuard g(device());
    tree_ok(eh_tr_fwd(&fwd_, 0, feat_fp32_, bm_, cur_stream()), "tower fwd");
  }
  // internals for PairPlan (the fused pair step reuses this tower's sampler / forward /
  // routed dW description)
  const TrSampleArgs& sample_args() const { return sample_; }
  const TrFwdArgs& fwd_args() const { return fwd_; }
  const TrDwProb& prob() const { return dw_.probs[0]; }
  int feat_fp32() const { return feat_fp32_; }
  int bm() const { return bm_; }
  int64_t R() const { return R_; }
  int64_t H() const { return H_; }
  int64_t D() const { return D_; }
  using PlanDict::device;

  // dA1 (the plan's buffer) -> gW0 (the plan's buffer)
  void bwd() {
    dw_.launch({0}, c10::nullopt, false, 1.0);
    const c10::DeviceGuard g(device());
    tree_ok(eh_tr_opt(&dw_.opt, 0, cur_stream()), "tower reduce");
  }

 private:
  int64_t R_, F1_, F2_, logP_, D_, H_, self_, M_;
  int feat_fp32_ = 0, bm_ = 32;
  TrGraph g_{};
  TrTree tree_{};
  TrSampleArgs sample_{};
  TrFwdArgs fwd_{};
  DwPlan dw_{*this};  // the routed W0 problem and its segment

  int32_t* owned_i32(int64_t n) { return full(n, -1, torch::kInt32).data_ptr<int32_t>(); }
};

// The fused unsupervised GraphSAGE step (models/sage_tower.py, fused mode): both towers'
// layer 0 (their TowerPlan samplers + forwards; the roots are drawn inside the samplers:
// source roots from the alias table, the context tower's positives as one out-neighbour of
// the recomputed source root and its negatives from a stream of their own), the pair head
// (tr_pair_head: last conv + fc of both towers, pair loss, backward to dA1), ONE dW launch
// (both routed W0 problems + W1 / Wfc of both towers) and ONE optimizer launch over the
// flat parameters (split-K reduce, Adam / Adagrad / SGD / momentum, bf16 shadows, loss and
// reciprocal-rank hand-off): 7 launches per step.
class PairPlan : private PlanDict {
 public:
  PairPlan(const TowerPlan& s, const TowerPlan& c, py::dict d) : PlanDict(d, "PairPlan", s.device()) {
    B_ = geti("B");
    K_ = geti("K");
    H0_ = s.H();
    H1_ = geti("H1");
    E_ = geti("E");
    TORCH_CHECK(c.R() == B_ * (1 + K_) && s.R() == B_, "PairPlan: tower roots must be B and B (1 + K)");
    TORCH_CHECK(c.H() == H0_ && c.D() == s.D(), "PairPlan: towers must have the same layer-0 shape");
    TORCH_CHECK(B_ % 32 == 0 && K_ >= 1 && K_ <= 15, "PairPlan: B % 32 == 0 and 1 <= K <= 15");
    TORCH_CHECK(H1_ % 64 == 0 && E_ % 32 == 0, "PairPlan: padded dims (H1 % 64, E % 32)");
    TORCH_CHECK(eh_tr_pair_head_lds(static_cast<int>(K_), static_cast<int>(2 * H0_), static_cast<int>(H1_),
                                    static_cast<int>(E_)) <= 160 * 1024 - 256,
                "PairPlan: the pair head does not fit in LDS (K / widths too large)");
    fpx_ = s.feat_fp32();
    bm_s_ = s.bm();
    bm_c_ = c.bm();
    // samplers: roots drawn in the kernels
    ss_ = s.sample_args();
    sc_ = c.sample_args();
    ss_.tr.root_in = nullptr;
    ss_.tr.root_mode = 0;
    ss_.tr.stream_off = 0;
    sc_.tr.root_in = nullptr;
    sc_.tr.root_mode = 1;
    sc_.tr.pair_B = static_cast<int32_t>(B_);
    sc_.tr.pair_mask = static_cast<uint32_t>(geti("pos_mask"));
    sc_.tr.stream_off = 8;
    // forwards: the source tower's block 0 advances the Adam step and the RNG counter
    fs_ = s.fwd_args();
    fc_ = c.fwd_args();
    fs_.roots_in = ss_.roots;  // roots_cur: the roots the samplers drew
    fc_.roots_in = sc_.roots;
    fs_.step = ptr<int64_t>("step", torch::kInt64, 1);
    fc_.step = nullptr;
    fc_.rng = zeros_ptr<int64_t>(2, torch::kInt64);
    // head
    nblk_ = B_ / 16;
    TrPairHeadArgs& h = head_;
    h.B = static_cast<int32_t>(B_);
    h.K = static_cast<int32_t>(K_);
    h.H0x2 = static_cast<int32_t>(2 * H0_);
    h.H1 = static_cast<int32_t>(H1_);
    h.E = static_cast<int32_t>(E_);
    h.inv_n = 1.f / static_cast<float>(B_ * (1 + K_));
    h.head_part = zeros_ptr<float>(nblk_ * 4, torch::kFloat32);
    tower(h.s, s, "s");
    tower(h.c, c, "c");
    // dW: routed W0 of both towers (their plans and partials), then W1 / Wfc of each tower
    const TowerPlan* tp[2] = {&s, &c};
    const TrPairTower* tw[2] = {&h.s, &h.c};
    for (int t = 0; t < 2; ++t) dw_.probs.push_back(tp[t]->prob());
    for (int t = 0; t < 2; ++t) {
      dw_.add(H1_, 2 * H0_, tp[t]->R(), tw[t]->g_kt, tw[t]->A1_kt, nullptr, nullptr, 0, 0, 0);  // dW1 = g^T A1
      dw_.add(E_, H1_, tp[t]->R(), tw[t]->de_kt, tw[t]->h_kt, nullptr, nullptr, 0, 0, 0);      // dWfc = de^T h1
    }
    // optimizer over the flat buffer, which may end in padding (parallel/flat.py pads to a
    // multiple of 8): per tower W0, W1, Wfc, bfc
    std::vector<int64_t> off = getv("offsets");
    TORCH_CHECK(off.size() == 9, "PairPlan: offsets = 8 segments + end");
    for (int t = 0; t < 2; ++t) {
      const TrPairTower& T_ = *tw[t];
      dw_.add_seg(off[4 * t], dw_.probs[t], tp[t]->fwd_args().W, nullptr);
      dw_.add_seg(off[4 * t + 1], dw_.probs[2 + 2 * t], T_.W1, T_.W1T);
      dw_.add_seg(off[4 * t + 2], dw_.probs[3 + 2 * t], T_.Wfc, T_.WfcT);
      dw_.add_vec_seg(off[4 * t + 3], E_, T_.dbfc_part, nblk_);
      TORCH_CHECK(off[4 * t + 4] - off[4 * t + 3] == E_, "PairPlan: bias segment must be E long");
    }
    dw_.layout_segs();
    dw_.fill_opt(off.back(), h.head_part, nblk_, true);
    dw_.try_fuse(true);
  }

  bool fused() const { return dw_.fused(); }
  int64_t fuse_error() const { return dw_.fuse_error(); }

  void sample() {
    const c10::DeviceGuard g(device());
    tree_ok(eh_tr_sample(&ss_, cur_stream()), "pair sample (source)");
    tree_ok(eh_tr_sample(&sc_, cur_stream()), "pair sample (context)");
  }
  void fwd() {
    const c10::DeviceGuard g(device());
    tree_ok(eh_tr_fwd(&fs_, 0, fpx_, bm_s_, cur_stream()), "pair fwd (source)");
    tree_ok(eh_tr_fwd(&fc_, 0, fpx_, bm_c_, cur_stream()), "pair fwd (context)");
  }
  void head() {
    const c10::DeviceGuard g(device());
    tree_ok(eh_tr_pair_head(&head_, cur_stream()), "pair head");
  }
  // fuse (a fused() plan): the launch also runs the optimizer, what opt(2, grad_scale) would do
  void dw(bool fuse, double grad_scale) { dw_.launch(dw_.all(), c10::nullopt, fuse, grad_scale); }
  // 0: split-K reduce into the flat gradient; 1: optimizer from it (scaled); 2: both; 3: shadows
  void opt(int mode, double grad_scale) {
    const c10::DeviceGuard g(device());
    TrOptArgs a = dw_.opt;
    a.c.grad_scale = static_cast<float>(grad_scale);
    tree_ok(eh_tr_opt(&a, mode, cur_stream()), "pair opt");
  }
  void set_lr(double lr) { dw_.set_lr(lr); }
  void set_grad(torch::Tensor g) { dw_.set_grad(g, false); }
  // the dW launch's problems, routed first: slabs the optimizer sums / slabs summed in the block
  std::vector<int64_t> splits() const { return dw_.splits(); }
  std::vector<int64_t> folds() const { return dw_.folds(); }

 private:
  int64_t B_, K_, H0_, H1_, E_, nblk_;
  int fpx_ = 0, bm_s_ = 32, bm_c_ = 32;
  TrSampleArgs ss_{}, sc_{};
  TrFwdArgs fs_{}, fc_{};
  TrPairHeadArgs head_{};
  DwPlan dw_{*this};  // W0 of both towers (routed), then W1, Wfc of the source and of the context tower

  void tower(TrPairTower& t, const TowerPlan& tp, const std::string& x) {
    const int64_t R = tp.R();
    t.A1 = tp.fwd_args().a_next;
    t.W1 = bf(("W1_sh_" + x).c_str(), H1_ * 2 * H0_);
    t.W1T = bf(("W1_shT_" + x).c_str(), H1_ * 2 * H0_);
    t.Wfc = bf(("Wfc_sh_" + x).c_str(), E_ * H1_);
    t.WfcT = bf(("Wfc_shT_" + x).c_str(), E_ * H1_);
    t.bfc = ptr<float>(("bfc_" + x).c_str(), torch::kFloat32, E_);
    t.A1_kt = zeros_ptr<uint16_t>(R * 2 * H0_, torch::kBFloat16);
    t.h_kt = zeros_ptr<uint16_t>(R * H1_, torch::kBFloat16);
    t.de_kt = zeros_ptr<uint16_t>(R * E_, torch::kBFloat16);
    t.g_kt = zeros_ptr<uint16_t>(R * H1_, torch::kBFloat16);
    t.dA1 = const_cast<float*>(tp.prob().dA);
    t.dbfc_part = zeros_ptr<float>(nblk_ * E_, torch::kFloat32);
  }
};

}  // namespace

void register_tree_ops(py::module& m) {
  static_assert(kTrHeadSampleRows == 256, "head sampler blocks: 1024 threads, 256 rows");
  py::class_<TreePlan>(m, "TreePlan")
      .def(py::init<py::dict>())
      .def("sample", &TreePlan::sample)
      .def("fwd", &TreePlan::fwd, py::arg("prof") = py::none(), py::arg("gemm_only") = false)
      .def("fwd_blocks", [](const TreePlan& t) { return t.fwd_blocks(); })
      .def("head", &TreePlan::head, py::arg("prof") = py::none(), py::arg("with_sample") = false)
      .def("bwd", &TreePlan::bwd)
      .def("dw", &TreePlan::dw, py::arg("which"), py::arg("prof") = py::none(), py::arg("fuse") = false,
           py::arg("grad_scale") = 1.0)
      .def("fused", &TreePlan::fused)
      .def("dw_blocks", &TreePlan::dw_blocks, py::arg("fuse"))
      .def("fuse_error", &TreePlan::fuse_error)
      .def("route_blocks", &TreePlan::route_blocks)
      .def("opt", &TreePlan::opt, py::arg("mode"), py::arg("grad_scale") = 1.0, py::arg("with_sample") = false,
           py::arg("with_gather") = false)
      .def("pipeline_ok", &TreePlan::pipeline_ok)
      .def("opt_segments", &TreePlan::opt_segments, py::arg("mode"), py::arg("segs"), py::arg("head_stats"))
      .def("set_lr", &TreePlan::set_lr)
      .def("set_grad16", &TreePlan::set_grad16, py::arg("g16"))
      .def("set_grad", &TreePlan::set_grad, py::arg("g"))
      .def("num_problems", &TreePlan::num_problems)
      .def("splits", &TreePlan::splits)
      .def("folds", &TreePlan::folds)
      .def("problems", &TreePlan::problems, py::arg("route"));
  m.attr("tree_head_rows") = kTrHeadRows;
  py::class_<TowerPlan>(m, "TowerPlan")
      .def(py::init<py::dict>())
      .def("shadow", &TowerPlan::shadow)
      .def("sample", &TowerPlan::sample)
      .def("fwd", &TowerPlan::fwd)
      .def("bwd", &TowerPlan::bwd)
      .def("fused", &TowerPlan::fused)
      .def("fuse_error", &TowerPlan::fuse_error);
  py::class_<PairPlan>(m, "PairPlan")
      .def(py::init<const TowerPlan&, const TowerPlan&, py::dict>(), py::keep_alive<1, 2>(), py::keep_alive<1, 3>())
      .def("sample", &PairPlan::sample)
      .def("fwd", &PairPlan::fwd)
      .def("head", &PairPlan::head)
      .def("dw", &PairPlan::dw, py::arg("fuse") = false, py::arg("grad_scale") = 1.0)
      .def("fused", &PairPlan::fused)
      .def("fuse_error", &PairPlan::fuse_error)
      .def("opt", &PairPlan::opt, py::arg("mode"), py::arg("grad_scale") = 1.0)
      .def("set_lr", &PairPlan::set_lr)
      .def("set_grad", &PairPlan::set_grad)
      .def("splits", &PairPlan::splits)
      .def("folds", &PairPlan::folds);
}
