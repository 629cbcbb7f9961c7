// torch binding of the list-grouped IVF search (knn_grouped.hip), on the submodule _hip_ops.knn_grouped.
// Host-only; operands go through binding_util.h (rules R1-R3 there).  Everything is allocated here, sized
// from nq, nprobe and ncent alone: nothing is read back from the device.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

// the inverted probe table of probe [nq, nprobe] over ncent lists, the work items, and the partials
// (dist / row [nq, nprobe, k], written so far only where an entry names no list):
// (qptr [ncent + 1], pairs [nq * nprobe], items [max_items, 2], n_items [1], dist, row)
std::vector<torch::Tensor> knn_grouped_invert(torch::Tensor probe, int64_t ncent, int64_t k) {
  const Operands c("knn_grouped_invert", probe, "probe");
  c.i64(probe, "probe");
  TORCH_CHECK(probe.dim() == 2 && probe.size(0) >= 1 && probe.size(1) >= 1 && probe.size(1) <= eh_knn_max_splits(),
              "knn_grouped_invert: probe must be [nq >= 1, nprobe] with nprobe in [1, ", eh_knn_max_splits(), "]");
  const int64_t nq = probe.size(0), nprobe = probe.size(1);
  TORCH_CHECK(nq <= INT32_MAX / nprobe, "knn_grouped_invert: nq * nprobe must be below 2^31, got ", nq, " x ", nprobe);
  TORCH_CHECK(ncent >= 1 && ncent < INT32_MAX, "knn_grouped_invert: ncent must be in [1, 2^31 - 1), got ", ncent);
  TORCH_CHECK(k >= 1 && k <= eh_knn_max_k(), "knn_grouped_invert: k must be in [1, ", eh_knn_max_k(), "], got ", k);
  const auto g = c.guard();
  const auto i32 = probe.options().dtype(torch::kInt32);
  const int64_t max_items = eh_knn_grouped_max_items(nq, static_cast<int>(nprobe), ncent);
  auto cnt = torch::zeros({ncent}, probe.options());
  auto qptr = torch::empty({ncent + 1}, i32);
  auto pairs = torch::empty({nq * nprobe}, i32);
  auto items = torch::empty({max_items, 2}, i32);
  auto n_items = torch::empty({1}, i32);
  auto pd = torch::empty({nq, nprobe, k}, probe.options().dtype(torch::kFloat32));
  auto pr = torch::empty({nq, nprobe, k}, probe.options());
  launch_ok(eh_knn_grouped_invert(probe.data_ptr<int64_t>(), nq, static_cast<int>(nprobe), ncent, static_cast<int>(k),
                                  cnt.data_ptr<int64_t>(), qptr.data_ptr<int32_t>(), pairs.data_ptr<int32_t>(),
                                  items.data_ptr<int32_t>(), n_items.data_ptr<int32_t>(), pd.data_ptr<float>(),
                                  pr.data_ptr<int64_t>(), cur_stream()),
            "knn_grouped_invert");
  return {qptr, pairs, items, n_items, pd, pr};
}

// scans every work item of an inverted probe table and writes its pairs' partials into dist / row, in
// place.  q and xs are both fp32 or both bf16 (read in place).
void knn_grouped_scan(torch::Tensor q, torch::Tensor xs, torch::Tensor xn, torch::Tensor list_ptr,
                      torch::Tensor row_of, torch::Tensor qptr, torch::Tensor pairs, torch::Tensor items,
                      torch::Tensor n_items, torch::Tensor pd, torch::Tensor pr) {
  const Operands c("knn_grouped_scan", q, "q");
  const bool bf = c.bf16_or_f32(xs, "xs");
  c.is(q, xs.scalar_type(), "q");
  c.f32(xn, "xn");
  c.i64(list_ptr, "list_ptr");
  c.i64(row_of, "row_of");
  c.i32(qptr, "qptr");
  c.i32(pairs, "pairs");
  c.i32(items, "items");
  c.i32(n_items, "n_items");
  c.f32(pd, "dist");
  c.i64(pr, "row");
  TORCH_CHECK(q.dim() == 2 && xs.dim() == 2 && q.size(1) == xs.size(1) && q.size(1) >= 1,
              "knn_grouped_scan: q [nq, d] and xs [n, d] must share d >= 1");
  TORCH_CHECK(q.size(1) <= INT32_MAX / 8, "knn_grouped_scan: d too large");
  const int64_t nq = q.size(0), n = xs.size(0);
  TORCH_CHECK(nq >= 1, "knn_grouped_scan: empty q");
  TORCH_CHECK(xn.dim() == 1 && xn.numel() == n && row_of.dim() == 1 && row_of.numel() == n,
              "knn_grouped_scan: xn and row_of must be [n]");
  TORCH_CHECK(list_ptr.dim() == 1 && list_ptr.numel() >= 2 && list_ptr.numel() <= INT32_MAX,
              "knn_grouped_scan: list_ptr must be [ncent + 1]");
  const int64_t ncent = list_ptr.numel() - 1;
  TORCH_CHECK(pd.dim() == 3 && pd.size(0) == nq && pr.sizes() == pd.sizes(),
              "knn_grouped_scan: dist and row must be [nq, nprobe, k]");
  const int64_t nprobe = pd.size(1), k = pd.size(2);
  TORCH_CHECK(nprobe >= 1 && nprobe <= eh_knn_max_splits() && nq <= INT32_MAX / nprobe,
              "knn_grouped_scan: nprobe must be in [1, ", eh_knn_max_splits(), "] and nq * nprobe below 2^31");
  TORCH_CHECK(k >= 1 && k <= eh_knn_max_k(), "knn_grouped_scan: k must be in [1, ", eh_knn_max_k(), "], got ", k);
  const int64_t max_items = eh_knn_grouped_max_items(nq, static_cast<int>(nprobe), ncent);
  TORCH_CHECK(qptr.numel() == ncent + 1 && pairs.numel() == nq * nprobe && items.numel() == 2 * max_items &&
                  n_items.numel() == 1,
              "knn_grouped_scan: qptr / pairs / items / n_items are not those of knn_grouped_invert for these sizes");
  const auto g = c.guard();
  launch_ok(eh_knn_grouped_scan(q.data_ptr(), xs.data_ptr(), bf ? 1 : 0, xn.data_ptr<float>(),
                                list_ptr.data_ptr<int64_t>(), row_of.data_ptr<int64_t>(), qptr.data_ptr<int32_t>(),
                                pairs.data_ptr<int32_t>(), items.data_ptr<int32_t>(), n_items.data_ptr<int32_t>(),
                                max_items, nq, n, ncent, static_cast<int>(nprobe), static_cast<int>(q.size(1)),
                                static_cast<int>(k), pd.data_ptr<float>(), pr.data_ptr<int64_t>(), cur_stream()),
            "knn_grouped_scan");
}

}  // namespace

void register_knn_grouped_ops(py::module& m) {
  m.def("invert", &knn_grouped_invert, py::arg("probe"), py::arg("ncent"), py::arg("k"));
  m.def("scan", &knn_grouped_scan, py::arg("q"), py::arg("xs"), py::arg("xn"), py::arg("list_ptr"), py::arg("row_of"),
        py::arg("qptr"), py::arg("pairs"), py::arg("items"), py::arg("n_items"), py::arg("dist"), py::arg("row"));
  m.attr("tq") = eh_knn_grouped_tq();
}
