// torch binding of the rank kernels of the projected KG models (kg_rank_proj.hip), registered on
// the submodule _hip_ops.kg_rank_proj.  Host-only; operands go through binding_util.h (rules
// R1-R3 there).  The outputs, the relation order and the tile table are made here, never inside
// a launcher.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

constexpr int64_t kTile = 64;            // queries per tile of kg_rank_proj.hip
constexpr int64_t kTargetBlocks = 1024;  // as ops/kg_rank_ops.py: a few resident blocks per CU

// (better [B], ties [B]) int64.  model 0 transh (proj_r = hyper), 1 transd (proj_e =
// entity_transfer, proj_r = relation_transfer), 2 transr (proj_r = mat [Nr, E * R]); table [N, E]
// holds exactly the candidates; given / true_idx in [0, N), rel in [0, Nr); side 0 head, 1 tail;
// kind 0 l1, 1 l2; splits 0: sized here from the number of tiles.
std::vector<torch::Tensor> rank_counts(int64_t model, torch::Tensor table, torch::Tensor rel_table,
                                       c10::optional<torch::Tensor> proj_e, torch::Tensor proj_r, torch::Tensor given,
                                       torch::Tensor true_idx, torch::Tensor rel, int64_t side, int64_t kind,
                                       c10::optional<torch::Tensor> filt_ptr, c10::optional<torch::Tensor> filt_idx,
                                       int64_t splits) {
  const Operands c("kg_rank_proj.rank_counts", table, "table");
  c.f32(table, "table");
  c.f32(rel_table, "rel_table");
  c.f32(proj_e, "proj_e");
  c.f32(proj_r, "proj_r");
  c.i64(given, "given");
  c.i64(true_idx, "true_idx");
  c.i64(rel, "rel");
  c.i64(filt_ptr, "filt_ptr");
  c.i32(filt_idx, "filt_idx");
  TORCH_CHECK(model >= 0 && model <= 2, "kg_rank_proj: model must be 0 (transh), 1 (transd) or 2 (transr)");
  TORCH_CHECK(kind >= 0 && kind <= 1, "kg_rank_proj: kind must be 0 (l1) or 1 (l2)");
  TORCH_CHECK(side >= 0 && side <= 1, "kg_rank_proj: side must be 0 (head) or 1 (tail)");
  TORCH_CHECK(table.dim() == 2 && rel_table.dim() == 2 && proj_r.dim() == 2 && table.size(0) >= 1 &&
                  rel_table.size(0) >= 1,
              "kg_rank_proj: table [N, E], rel_table [Nr, R] and proj_r must be non-empty matrices");
  const int64_t N = table.size(0), E = table.size(1), R = rel_table.size(1), Nr = rel_table.size(0);
  const int64_t dmax = eh_kg_rank_proj_max_dim();
  TORCH_CHECK(E >= 4 && E % 4 == 0 && E <= dmax && R >= 4 && R % 4 == 0 && R <= dmax,
              "kg_rank_proj: the kernels need E % 4 == 0, R % 4 == 0 and 4 <= E, R <= ", dmax, ", got E = ", E,
              ", R = ", R);
  TORCH_CHECK(model == 2 || E == R, "kg_rank_proj: transh / transd need E == R");
  TORCH_CHECK(proj_r.size(0) == Nr && proj_r.size(1) == (model == 2 ? E * R : E),
              "kg_rank_proj: proj_r must be [Nr, ", model == 2 ? "E * R" : "E", "]");
  TORCH_CHECK((model == 1) == proj_e.has_value(), "kg_rank_proj: proj_e (entity_transfer) comes with transd only");
  if (proj_e.has_value())
    TORCH_CHECK(proj_e->dim() == 2 && proj_e->size(0) == N && proj_e->size(1) == E,
                "kg_rank_proj: proj_e must be [N, E] like table");
  TORCH_CHECK(N <= INT32_MAX, "kg_rank_proj: N too large");
  const int64_t B = given.numel();
  TORCH_CHECK(B >= 1 && B <= INT32_MAX, "kg_rank_proj: given must hold 1 .. 2^31 - 1 queries");
  TORCH_CHECK(given.dim() == 1 && true_idx.dim() == 1 && rel.dim() == 1 && true_idx.numel() == B && rel.numel() == B,
              "kg_rank_proj: given, true_idx and rel must be [B]");
  TORCH_CHECK(filt_ptr.has_value() == filt_idx.has_value(),
              "kg_rank_proj: filt_ptr and filt_idx come together or not at all");
  TORCH_CHECK(splits >= 0 && splits <= eh_kg_rank_max_splits(), "kg_rank_proj: splits must be in [0, ",
              eh_kg_rank_max_splits(), "]");
  // the kernels read table rows with 16-byte loads
  for (const torch::Tensor* t : {&table, &rel_table, &proj_r, proj_e.has_value() ? &*proj_e : &table})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "kg_rank_proj: tables must be 16-byte aligned");
  const int64_t* fp = nullptr;
  const int32_t* fi = nullptr;
  int64_t nf = 0;
  if (filt_ptr.has_value()) {
    TORCH_CHECK(filt_ptr->dim() == 1 && filt_ptr->numel() == B + 1, "kg_rank_proj: filt_ptr must be [B + 1], got ",
                filt_ptr->numel(), " entries for B = ", B);
    TORCH_CHECK(filt_idx->dim() == 1, "kg_rank_proj: filt_idx must be one-dimensional");
    fp = filt_ptr->data_ptr<int64_t>();
    nf = filt_idx->numel();
    fi = nf > 0 ? filt_idx->data_ptr<int32_t>() : nullptr;
  }
  const auto g = c.guard();
  {
    // every id addresses a table row in the kernel: none may leave its table
    const auto mm = torch::stack({given.min(), given.max(), true_idx.min(), true_idx.max(), rel.min(), rel.max()}).cpu();
    const auto v = mm.accessor<int64_t, 1>();
    TORCH_CHECK(v[0] >= 0 && v[1] < N, "kg_rank_proj: given out of range [0, ", N, "): min ", v[0], ", max ", v[1]);
    TORCH_CHECK(v[2] >= 0 && v[3] < N, "kg_rank_proj: true_idx out of range [0, ", N, "): min ", v[2], ", max ",
                v[3]);
    TORCH_CHECK(v[4] >= 0 && v[5] < Nr, "kg_rank_proj: rel out of range [0, ", Nr, "): min ", v[4], ", max ", v[5]);
  }
  // the queries by relation, and one tile per run of at most 64 queries of one relation
  const auto order = rel.argsort(/*stable=*/true, /*dim=*/0, /*descending=*/false);
  const auto uc = torch::unique_consecutive(rel.index_select(0, order), /*return_inverse=*/false,
                                            /*return_counts=*/true);
  const torch::Tensor rels = std::get<0>(uc), counts = std::get<2>(uc);
  const auto per = torch::div(counts + (kTile - 1), kTile, "floor");
  const auto per_end = per.cumsum(0);
  const int64_t T = per_end[-1].item<int64_t>();  // the one host read of the tile table
  const auto iopt = rel.options();
  const auto seg = torch::repeat_interleave(torch::arange(rels.numel(), iopt), per, 0, T);
  const auto within = (torch::arange(T, iopt) - (per_end - per).index_select(0, seg)) * kTile;
  const auto first = (counts.cumsum(0) - counts).index_select(0, seg) + within;
  const auto cnt = (counts.index_select(0, seg) - within).clamp_max(kTile);
  const auto tiles = torch::stack({rels.index_select(0, seg), first, cnt}, 1).to(torch::kInt32).contiguous();
  if (splits == 0) {
    const int64_t ctiles = (N + kTile - 1) / kTile;
    splits = std::max<int64_t>(1, std::min<int64_t>({(kTargetBlocks + T - 1) / T, eh_kg_rank_max_splits(), ctiles}));
  }
  auto ts = torch::empty({B}, table.options());
  auto pb = torch::empty({B, splits}, iopt);
  auto pt = torch::empty({B, splits}, iopt);
  launch_ok(eh_kg_rank_proj(static_cast<int>(model), table.data_ptr<float>(), rel_table.data_ptr<float>(),
                            proj_e.has_value() ? proj_e->data_ptr<float>() : nullptr, proj_r.data_ptr<float>(), N,
                            static_cast<int>(E), static_cast<int>(R), given.data_ptr<int64_t>(),
                            true_idx.data_ptr<int64_t>(), order.data_ptr<int64_t>(), tiles.data_ptr<int32_t>(), T, B,
                            static_cast<int>(side), static_cast<int>(kind), fp, fi, nf, static_cast<int>(splits),
                            ts.data_ptr<float>(), pb.data_ptr<int64_t>(), pt.data_ptr<int64_t>(), cur_stream()),
            "kg_rank_proj");
  return {pb.sum(1), pt.sum(1)};
}

}  // namespace

void register_kg_rank_proj_ops(py::module& m) {
  m.def("rank_counts", &rank_counts, py::arg("model"), py::arg("table"), py::arg("rel_table"), py::arg("proj_e"),
        py::arg("proj_r"), py::arg("given"), py::arg("true_idx"), py::arg("rel"), py::arg("side"), py::arg("kind"),
        py::arg("filt_ptr") = py::none(), py::arg("filt_idx") = py::none(), py::arg("splits") = 0);
  m.attr("max_dim") = eh_kg_rank_proj_max_dim();
}
