// torch binding of the link-prediction rank kernels (kg_rank.hip).  Host-only; operands go
// through binding_util.h (rules R1-R3 there).  The outputs are allocated here, never inside a
// launcher.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

// (better [B], ties [B]) int64 of q [B, d] against cands [N, d]; kind 0 l1 / 1 l2 / 2 dot;
// filt_ptr [B + 1] int64 + filt_idx int32 (ascending inside a list) or both None
std::vector<torch::Tensor> kg_rank_counts(torch::Tensor q, torch::Tensor cands, torch::Tensor true_idx, int64_t kind,
                                          c10::optional<torch::Tensor> filt_ptr,
                                          c10::optional<torch::Tensor> filt_idx, int64_t splits) {
  const Operands c("kg_rank_counts", q, "q");
  c.f32(q, "q");
  c.f32(cands, "cands");
  c.i64(true_idx, "true_idx");
  c.i64(filt_ptr, "filt_ptr");
  c.i32(filt_idx, "filt_idx");
  TORCH_CHECK(kind >= 0 && kind <= 2, "kg_rank_counts: kind must be 0 (l1), 1 (l2) or 2 (dot)");
  TORCH_CHECK(q.dim() == 2 && cands.dim() == 2 && q.size(1) == cands.size(1) && q.size(1) >= 1,
              "kg_rank_counts: q [B, d] and cands [N, d] must share d >= 1");
  const int64_t B = q.size(0), N = cands.size(0);
  TORCH_CHECK(B >= 1 && N >= 1, "kg_rank_counts: empty q or cands");
  TORCH_CHECK(q.size(1) <= INT32_MAX && N <= INT32_MAX, "kg_rank_counts: d or N too large");
  TORCH_CHECK(true_idx.dim() == 1 && true_idx.numel() == B, "kg_rank_counts: true_idx must be [B]");
  TORCH_CHECK(filt_ptr.has_value() == filt_idx.has_value(),
              "kg_rank_counts: filt_ptr and filt_idx come together or not at all");
  TORCH_CHECK(splits >= 1 && splits <= eh_kg_rank_max_splits(), "kg_rank_counts: splits must be in [1, ",
              eh_kg_rank_max_splits(), "]");
  const int64_t* fp = nullptr;
  const int32_t* fi = nullptr;
  int64_t nf = 0;
  if (filt_ptr.has_value()) {
    TORCH_CHECK(filt_ptr->dim() == 1 && filt_ptr->numel() == B + 1, "kg_rank_counts: filt_ptr must be [B + 1], got ",
                filt_ptr->numel(), " entries for B = ", B);
    TORCH_CHECK(filt_idx->dim() == 1, "kg_rank_counts: filt_idx must be one-dimensional");
    fp = filt_ptr->data_ptr<int64_t>();
    nf = filt_idx->numel();
    fi = nf > 0 ? filt_idx->data_ptr<int32_t>() : nullptr;
  }
  const auto g = c.guard();
  {
    // a position outside cands has no score to rank against
    const auto mm = torch::stack({true_idx.min(), true_idx.max()}).cpu();
    const int64_t lo = mm[0].item<int64_t>(), hi = mm[1].item<int64_t>();
    TORCH_CHECK(lo >= 0 && hi < N, "kg_rank_counts: true_idx out of range [0, ", N, "): min ", lo, ", max ", hi);
  }
  auto ts = torch::empty({B}, q.options());
  auto pb = torch::empty({B, splits}, q.options().dtype(torch::kInt64));
  auto pt = torch::empty({B, splits}, q.options().dtype(torch::kInt64));
  launch_ok(eh_kg_rank_true(q.data_ptr<float>(), cands.data_ptr<float>(), true_idx.data_ptr<int64_t>(), B, N,
                            static_cast<int>(q.size(1)), static_cast<int>(kind), ts.data_ptr<float>(), cur_stream()),
            "kg_rank_true");
  launch_ok(eh_kg_rank_scan(q.data_ptr<float>(), cands.data_ptr<float>(), true_idx.data_ptr<int64_t>(),
                            ts.data_ptr<float>(), fp, fi, nf, B, N, static_cast<int>(q.size(1)), static_cast<int>(kind),
                            static_cast<int>(splits), pb.data_ptr<int64_t>(), pt.data_ptr<int64_t>(), cur_stream()),
            "kg_rank_scan");
  return {pb.sum(1), pt.sum(1)};
}

}  // namespace

void register_kg_rank_ops(py::module& m) {
  m.def("kg_rank_counts", &kg_rank_counts, py::arg("q"), py::arg("cands"), py::arg("true_idx"), py::arg("kind"),
        py::arg("filt_ptr") = py::none(), py::arg("filt_idx") = py::none(), py::arg("splits") = 1);
  m.attr("kg_rank_max_splits") = eh_kg_rank_max_splits();
}
