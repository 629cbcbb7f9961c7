// torch binding of the k-nearest-neighbour kernels (knn.hip).  Host-only; operands go through
// binding_util.h (rules R1-R3 there).  The outputs are allocated here, never inside a launcher.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

void check_k(int64_t k) {
  TORCH_CHECK(k >= 1 && k <= eh_knn_max_k(), "knn: k must be in [1, ", eh_knn_max_k(), "], got ", k);
}

// partial lists (dist [nq, S, k] fp32, row [nq, S, k] int64) of q [nq, d] against x [n, d]
std::vector<torch::Tensor> knn_flat_scan(torch::Tensor q, torch::Tensor x, torch::Tensor xn, int64_t k,
                                         int64_t splits) {
  const Operands c("knn_flat_scan", q, "q");
  c.f32(q, "q");
  c.f32(x, "x");
  c.f32(xn, "xn");
  TORCH_CHECK(q.dim() == 2 && x.dim() == 2 && q.size(1) == x.size(1) && q.size(1) >= 1,
              "knn_flat_scan: q [nq, d] and x [n, d] must share d >= 1");
  TORCH_CHECK(q.size(0) >= 1 && x.size(0) >= 1, "knn_flat_scan: empty q or x");
  TORCH_CHECK(xn.dim() == 1 && xn.numel() == x.size(0), "knn_flat_scan: xn must be [n]");
  TORCH_CHECK(q.size(1) <= INT32_MAX, "knn_flat_scan: d too large");
  check_k(k);
  TORCH_CHECK(splits >= 1 && splits <= eh_knn_max_splits(), "knn_flat_scan: splits must be in [1, ",
              eh_knn_max_splits(), "]");
  const auto g = c.guard();
  const int64_t nq = q.size(0);
  auto pd = torch::empty({nq, splits, k}, q.options());
  auto pr = torch::empty({nq, splits, k}, q.options().dtype(torch::kInt64));
  launch_ok(eh_knn_flat_scan(q.data_ptr<float>(), x.data_ptr<float>(), xn.data_ptr<float>(), nq, x.size(0),
                             static_cast<int>(q.size(1)), static_cast<int>(k), static_cast<int>(splits),
                             pd.data_ptr<float>(), pr.data_ptr<int64_t>(), cur_stream()),
            "knn_flat_scan");
  return {pd, pr};
}

// partial lists with S = nprobe over the CSR inverted lists
std::vector<torch::Tensor> knn_ivf_scan(torch::Tensor q, torch::Tensor xs, torch::Tensor xn, torch::Tensor list_ptr,
                                        torch::Tensor row_of, torch::Tensor probe, int64_t k) {
  const Operands c("knn_ivf_scan", q, "q");
  c.f32(q, "q");
  c.f32(xs, "xs");
  c.f32(xn, "xn");
  c.i64(list_ptr, "list_ptr");
  c.i64(row_of, "row_of");
  c.i64(probe, "probe");
  TORCH_CHECK(q.dim() == 2 && xs.dim() == 2 && q.size(1) == xs.size(1) && q.size(1) >= 1,
              "knn_ivf_scan: q [nq, d] and xs [n, d] must share d >= 1");
  TORCH_CHECK(q.size(1) <= INT32_MAX, "knn_ivf_scan: d too large");
  const int64_t nq = q.size(0), n = xs.size(0);
  TORCH_CHECK(nq >= 1, "knn_ivf_scan: empty q");
  TORCH_CHECK(xn.dim() == 1 && xn.numel() == n && row_of.dim() == 1 && row_of.numel() == n,
              "knn_ivf_scan: xn and row_of must be [n]");
  TORCH_CHECK(list_ptr.dim() == 1 && list_ptr.numel() >= 2, "knn_ivf_scan: list_ptr must be [ncent + 1]");
  TORCH_CHECK(probe.dim() == 2 && probe.size(0) == nq && probe.size(1) >= 1 && probe.size(1) <= eh_knn_max_splits(),
              "knn_ivf_scan: probe must be [nq, nprobe] with nprobe in [1, ", eh_knn_max_splits(), "]");
  check_k(k);
  const auto g = c.guard();
  const int64_t nprobe = probe.size(1);
  auto pd = torch::empty({nq, nprobe, k}, q.options());
  auto pr = torch::empty({nq, nprobe, k}, q.options().dtype(torch::kInt64));
  launch_ok(eh_knn_ivf_scan(q.data_ptr<float>(), xs.data_ptr<float>(), xn.data_ptr<float>(),
                            list_ptr.data_ptr<int64_t>(), row_of.data_ptr<int64_t>(), probe.data_ptr<int64_t>(), nq, n,
                            list_ptr.numel() - 1, static_cast<int>(nprobe), static_cast<int>(q.size(1)),
                            static_cast<int>(k), pd.data_ptr<float>(), pr.data_ptr<int64_t>(), cur_stream()),
            "knn_ivf_scan");
  return {pd, pr};
}

// D [nq, k] fp32 = max(score + qn, 0), I [nq, k] int64
std::vector<torch::Tensor> knn_merge(torch::Tensor pd, torch::Tensor pr, torch::Tensor qn) {
  const Operands c("knn_merge", pd, "dist");
  c.f32(pd, "dist");
  c.i64(pr, "row");
  c.f32(qn, "qn");
  TORCH_CHECK(pd.dim() == 3 && pr.sizes() == pd.sizes(), "knn_merge: dist and row must be [nq, S, k]");
  const int64_t nq = pd.size(0), S = pd.size(1), k = pd.size(2);
  TORCH_CHECK(nq >= 1 && k >= 1 && k <= INT32_MAX, "knn_merge: empty partials");
  TORCH_CHECK(S >= 1 && S <= eh_knn_max_splits(), "knn_merge: S must be in [1, ", eh_knn_max_splits(), "]");
  TORCH_CHECK(qn.dim() == 1 && qn.numel() == nq, "knn_merge: qn must be [nq]");
  const auto g = c.guard();
  auto D = torch::empty({nq, k}, pd.options());
  auto I = torch::empty({nq, k}, pr.options());
  launch_ok(eh_knn_merge(pd.data_ptr<float>(), pr.data_ptr<int64_t>(), qn.data_ptr<float>(), nq, static_cast<int>(S),
                         static_cast<int>(k), D.data_ptr<float>(), I.data_ptr<int64_t>(), cur_stream()),
            "knn_merge");
  return {D, I};
}

}  // namespace

void register_knn_ops(py::module& m) {
  m.def("knn_flat_scan", &knn_flat_scan, py::arg("q"), py::arg("x"), py::arg("xn"), py::arg("k"), py::arg("splits"));
  m.def("knn_ivf_scan", &knn_ivf_scan, py::arg("q"), py::arg("xs"), py::arg("xn"), py::arg("list_ptr"),
        py::arg("row_of"), py::arg("probe"), py::arg("k"));
  m.def("knn_merge", &knn_merge, py::arg("dist"), py::arg("row"), py::arg("qn"));
  m.attr("knn_max_k") = eh_knn_max_k();
  m.attr("knn_max_splits") = eh_knn_max_splits();
}
