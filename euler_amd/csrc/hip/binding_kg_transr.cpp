// torch binding of the TransR score kernels (kg_transr.hip), registered on the submodule
// _hip_ops.kg_transr.  Host-only; operands go through binding_util.h (rules R1-R3 there).  The
// outputs are allocated here, never inside a launcher.  Ids need no range check: the kernels map
// an id outside its table to the table's last row.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

struct KgrIn {
  int64_t B, K, E, R, nneg;
};

KgrIn kgr_check(const Operands& c, const torch::Tensor& ent, const torch::Tensor& rel, const torch::Tensor& mat,
                const torch::Tensor& src, const torch::Tensor& dst, const torch::Tensor& ridx,
                const torch::Tensor& neg, int64_t kind, int64_t corrupt) {
  c.f32(ent, "ent");
  c.f32(rel, "rel");
  c.f32(mat, "mat");
  c.i64(src, "src");
  c.i64(dst, "dst");
  c.i64(ridx, "ridx");
  c.i64(neg, "neg");
  TORCH_CHECK(ent.dim() == 2 && rel.dim() == 2 && ent.size(0) >= 1 && rel.size(0) >= 1,
              "kg_transr: ent [Ne, E], rel [Nr, R]");
  const int64_t B = src.numel(), E = ent.size(1), R = rel.size(1);
  TORCH_CHECK(mat.dim() == 2 && mat.size(0) == rel.size(0) && mat.size(1) == E * R,
              "kg_transr: mat must be [Nr, E * R]");
  TORCH_CHECK(dst.numel() == B && ridx.numel() == B, "kg_transr: src / dst / ridx must have B entries");
  TORCH_CHECK(B == 0 || neg.numel() % B == 0, "kg_transr: neg must be [B, K]");
  TORCH_CHECK(E >= 4 && E % 4 == 0 && E <= 128 && R >= 4 && R % 4 == 0 && R <= 128,
              "kg_transr: the kernels need E % 4 == 0, R % 4 == 0 and 4 <= E, R <= 128");
  TORCH_CHECK(kind >= 0 && kind <= 1 && corrupt >= 0 && corrupt <= 2, "kg_transr: bad kind / corrupt");
  const int64_t K = B ? neg.numel() / B : 0;
  TORCH_CHECK(K <= 14, "kg_transr: the kernels take at most 14 negatives per triple");
  // the kernels read table rows with 16-byte loads
  for (const torch::Tensor* t : {&ent, &rel, &mat})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "kg_transr: tables must be 16-byte aligned");
  return KgrIn{B, K, E, R, corrupt == 2 ? 2 * K : K};
}

// (pos scores [B], corrupted scores [B, K or 2K])
std::vector<torch::Tensor> kgr_fwd(torch::Tensor ent, torch::Tensor rel, torch::Tensor mat, torch::Tensor src,
                                   torch::Tensor dst, torch::Tensor ridx, torch::Tensor neg, int64_t kind,
                                   int64_t corrupt) {
  const Operands c("kg_transr.fwd", ent, "ent");
  const KgrIn k = kgr_check(c, ent, rel, mat, src, dst, ridx, neg, kind, corrupt);
  const auto g = c.guard();
  auto pos_s = torch::empty({k.B}, ent.options());
  auto neg_s = torch::empty({k.B, k.nneg}, ent.options());
  launch_ok(eh_kgr_fwd(ent.data_ptr<float>(), rel.data_ptr<float>(), mat.data_ptr<float>(), ent.size(0), rel.size(0),
                       src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(), ridx.data_ptr<int64_t>(),
                       neg.data_ptr<int64_t>(), k.B, static_cast<int>(k.K), static_cast<int>(k.E),
                       static_cast<int>(k.R), static_cast<int>(kind), static_cast<int>(corrupt),
                       pos_s.data_ptr<float>(), neg_s.data_ptr<float>(), cur_stream()),
            "kgr_fwd");
  return {pos_s, neg_s};
}

// adds the table gradients into dent / drel / dmat (zeroed by the caller); pos_s / neg_s are the
// forward's scores, gpos / gneg their upstream gradients
void kgr_bwd(torch::Tensor ent, torch::Tensor rel, torch::Tensor mat, torch::Tensor src, torch::Tensor dst,
             torch::Tensor ridx, torch::Tensor neg, int64_t kind, int64_t corrupt, torch::Tensor pos_s,
             torch::Tensor neg_s, torch::Tensor gpos, torch::Tensor gneg, torch::Tensor dent, torch::Tensor drel,
             torch::Tensor dmat) {
  const Operands c("kg_transr.bwd", ent, "ent");
  const KgrIn k = kgr_check(c, ent, rel, mat, src, dst, ridx, neg, kind, corrupt);
  c.f32(pos_s, "pos_s");
  c.f32(neg_s, "neg_s");
  c.f32(gpos, "gpos");
  c.f32(gneg, "gneg");
  c.f32(dent, "dent");
  c.f32(drel, "drel");
  c.f32(dmat, "dmat");
  TORCH_CHECK(pos_s.numel() == k.B && neg_s.numel() == k.B * k.nneg && gpos.numel() == k.B &&
                  gneg.numel() == k.B * k.nneg,
              "kg_transr.bwd: scores and score grads must be [B] and [B, K or 2K]");
  TORCH_CHECK(dent.sizes() == ent.sizes() && drel.sizes() == rel.sizes() && dmat.sizes() == mat.sizes(),
              "kg_transr.bwd: table grads must match the tables");
  const auto g = c.guard();
  launch_ok(eh_kgr_bwd(ent.data_ptr<float>(), rel.data_ptr<float>(), mat.data_ptr<float>(), ent.size(0), rel.size(0),
                       src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(), ridx.data_ptr<int64_t>(),
                       neg.data_ptr<int64_t>(), k.B, static_cast<int>(k.K), static_cast<int>(k.E),
                       static_cast<int>(k.R), static_cast<int>(kind), static_cast<int>(corrupt),
                       pos_s.data_ptr<float>(), neg_s.data_ptr<float>(), gpos.data_ptr<float>(),
                       gneg.data_ptr<float>(), dent.data_ptr<float>(), drel.data_ptr<float>(),
                       dmat.data_ptr<float>(), cur_stream()),
            "kgr_bwd");
}

}  // namespace

void register_kg_transr_ops(py::module& m) {
  m.def("fwd", &kgr_fwd, py::arg("ent"), py::arg("rel"), py::arg("mat"), py::arg("src"), py::arg("dst"),
        py::arg("ridx"), py::arg("neg"), py::arg("kind"), py::arg("corrupt"));
  m.def("bwd", &kgr_bwd, py::arg("ent"), py::arg("rel"), py::arg("mat"), py::arg("src"), py::arg("dst"),
        py::arg("ridx"), py::arg("neg"), py::arg("kind"), py::arg("corrupt"), py::arg("pos_s"), py::arg("neg_s"),
        py::arg("gpos"), py::arg("gneg"), py::arg("dent"), py::arg("drel"), py::arg("dmat"));
}
