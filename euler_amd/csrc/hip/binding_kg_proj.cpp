// torch binding of the projected KG score kernels (kg_proj.hip), registered on the submodule
// _hip_ops.kg_proj.  Host-only; operands go through binding_util.h (rules R1-R3 there).  The
// outputs are allocated here, never inside a launcher.  Ids need no range check: the kernels map
// an id outside its table to the table's last row.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

struct KgpIn {
  int64_t B, K, D, nneg;
  const float* proj_e;
};

// model 0 (TransH): proj_e absent, proj_r = hyper; model 1 (TransD): proj_e = ent_t, proj_r = rel_t
KgpIn kgp_check(const Operands& c, int64_t model, const torch::Tensor& ent, const torch::Tensor& rel,
                const c10::optional<torch::Tensor>& proj_e, const torch::Tensor& proj_r, const torch::Tensor& src,
                const torch::Tensor& dst, const torch::Tensor& ridx, const torch::Tensor& neg, int64_t kind,
                int64_t corrupt) {
  c.f32(ent, "ent");
  c.f32(rel, "rel");
  c.f32(proj_e, "proj_e");
  c.f32(proj_r, "proj_r");
  c.i64(src, "src");
  c.i64(dst, "dst");
  c.i64(ridx, "ridx");
  c.i64(neg, "neg");
  TORCH_CHECK(model == 0 || model == 1, "kg_proj: model must be 0 (transh) or 1 (transd)");
  TORCH_CHECK(proj_e.has_value() == (model == 1), "kg_proj: proj_e goes with model 1 (transd) only");
  TORCH_CHECK(ent.dim() == 2 && rel.dim() == 2 && ent.size(1) == rel.size(1) && ent.size(0) >= 1 && rel.size(0) >= 1,
              "kg_proj: ent [Ne, D], rel [Nr, D]");
  TORCH_CHECK(proj_r.sizes() == rel.sizes(), "kg_proj: proj_r must have rel's shape");
  TORCH_CHECK(!proj_e.has_value() || proj_e->sizes() == ent.sizes(), "kg_proj: proj_e must have ent's shape");
  const int64_t B = src.numel(), D = ent.size(1);
  TORCH_CHECK(dst.numel() == B && ridx.numel() == B, "kg_proj: src / dst / ridx must have B entries");
  TORCH_CHECK(B == 0 || neg.numel() % B == 0, "kg_proj: neg must be [B, K]");
  TORCH_CHECK(D >= 4 && D % 4 == 0 && D <= 256, "kg_proj: the kernels need D % 4 == 0 and D <= 256");
  TORCH_CHECK(kind >= 0 && kind <= 1 && corrupt >= 0 && corrupt <= 2, "kg_proj: bad kind / corrupt");
  const int64_t K = B ? neg.numel() / B : 0;
  TORCH_CHECK(K <= INT32_MAX / 2, "kg_proj: too many negatives");
  return KgpIn{B, K, D, corrupt == 2 ? 2 * K : K, proj_e.has_value() ? proj_e->data_ptr<float>() : nullptr};
}

// (pos scores [B], corrupted scores [B, K or 2K])
std::vector<torch::Tensor> kgp_fwd(int64_t model, torch::Tensor ent, torch::Tensor rel,
                                   c10::optional<torch::Tensor> proj_e, torch::Tensor proj_r, torch::Tensor src,
                                   torch::Tensor dst, torch::Tensor ridx, torch::Tensor neg, int64_t kind,
                                   int64_t corrupt) {
  const Operands c("kg_proj.fwd", ent, "ent");
  const KgpIn k = kgp_check(c, model, ent, rel, proj_e, proj_r, src, dst, ridx, neg, kind, corrupt);
  const auto g = c.guard();
  auto pos_s = torch::empty({k.B}, ent.options());
  auto neg_s = torch::empty({k.B, k.nneg}, ent.options());
  launch_ok(eh_kgp_fwd(static_cast<int>(model), ent.data_ptr<float>(), rel.data_ptr<float>(), k.proj_e,
                       proj_r.data_ptr<float>(), ent.size(0), rel.size(0), src.data_ptr<int64_t>(),
                       dst.data_ptr<int64_t>(), ridx.data_ptr<int64_t>(), neg.data_ptr<int64_t>(), k.B, static_cast<int>(k.K),
                       static_cast<int>(k.D), static_cast<int>(kind), static_cast<int>(corrupt),
                       pos_s.data_ptr<float>(), neg_s.data_ptr<float>(), cur_stream()),
            "kgp_fwd");
  return {pos_s, neg_s};
}

// adds the table gradients into dent / drel / dproj_e / dproj_r (zeroed by the caller); pos_s / neg_s
// are the forward's scores, gpos / gneg their upstream gradients
void kgp_bwd(int64_t model, torch::Tensor ent, torch::Tensor rel, c10::optional<torch::Tensor> proj_e,
             torch::Tensor proj_r, torch::Tensor src, torch::Tensor dst, torch::Tensor ridx, torch::Tensor neg,
             int64_t kind, int64_t corrupt, torch::Tensor pos_s, torch::Tensor neg_s, torch::Tensor gpos,
             torch::Tensor gneg, torch::Tensor dent, torch::Tensor drel, c10::optional<torch::Tensor> dproj_e,
             torch::Tensor dproj_r) {
  const Operands c("kg_proj.bwd", ent, "ent");
  const KgpIn k = kgp_check(c, model, ent, rel, proj_e, proj_r, src, dst, ridx, neg, kind, corrupt);
  c.f32(pos_s, "pos_s");
  c.f32(neg_s, "neg_s");
  c.f32(gpos, "gpos");
  c.f32(gneg, "gneg");
  c.f32(dent, "dent");
  c.f32(drel, "drel");
  c.f32(dproj_e, "dproj_e");
  c.f32(dproj_r, "dproj_r");
  TORCH_CHECK(pos_s.numel() == k.B && neg_s.numel() == k.B * k.nneg && gpos.numel() == k.B &&
                  gneg.numel() == k.B * k.nneg,
              "kg_proj.bwd: scores and score grads must be [B] and [B, K or 2K]");
  TORCH_CHECK(dent.sizes() == ent.sizes() && drel.sizes() == rel.sizes() && dproj_r.sizes() == rel.sizes(),
              "kg_proj.bwd: table grads must match the tables");
  TORCH_CHECK(dproj_e.has_value() == (model == 1) && (!dproj_e.has_value() || dproj_e->sizes() == ent.sizes()),
              "kg_proj.bwd: dproj_e goes with model 1 (transd) and must have ent's shape");
  const auto g = c.guard();
  launch_ok(eh_kgp_bwd(static_cast<int>(model), ent.data_ptr<float>(), rel.data_ptr<float>(), k.proj_e,
                       proj_r.data_ptr<float>(), ent.size(0), rel.size(0), src.data_ptr<int64_t>(),
                       dst.data_ptr<int64_t>(), ridx.data_ptr<int64_t>(), neg.data_ptr<int64_t>(), k.B, static_cast<int>(k.K),
                       static_cast<int>(k.D), static_cast<int>(kind), static_cast<int>(corrupt),
                       pos_s.data_ptr<float>(), neg_s.data_ptr<float>(), gpos.data_ptr<float>(),
                       gneg.data_ptr<float>(), dent.data_ptr<float>(), drel.data_ptr<float>(),
                       dproj_e.has_value() ? dproj_e->data_ptr<float>() : nullptr, dproj_r.data_ptr<float>(),
                       cur_stream()),
            "kgp_bwd");
}

}  // namespace

void register_kg_proj_ops(py::module& m) {
  m.def("fwd", &kgp_fwd, py::arg("model"), py::arg("ent"), py::arg("rel"), py::arg("proj_e"), py::arg("proj_r"),
        py::arg("src"), py::arg("dst"), py::arg("ridx"), py::arg("neg"), py::arg("kind"), py::arg("corrupt"));
  m.def("bwd", &kgp_bwd, py::arg("model"), py::arg("ent"), py::arg("rel"), py::arg("proj_e"), py::arg("proj_r"),
        py::arg("src"), py::arg("dst"), py::arg("ridx"), py::arg("neg"), py::arg("kind"), py::arg("corrupt"),
        py::arg("pos_s"), py::arg("neg_s"), py::arg("gpos"), py::arg("gneg"), py::arg("dent"), py::arg("drel"),
        py::arg("dproj_e"), py::arg("dproj_r"));
}
