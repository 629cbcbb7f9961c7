// torch binding of the node-row embedding-bag kernels (node_embed.hip).  Host-only; operands
// go through binding_util.h (rules R1-R3 there); nothing is allocated in the forward and
// nothing synchronises, so both ops capture into a hipGraph.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

struct Index {
  const int64_t* indptr = nullptr;
  const int64_t* values = nullptr;
  const int64_t* node_ids = nullptr;
  int64_t nnz = 0, num_rows = -1;
};

// mode 0 / 1: (indptr [N + 1], values [nnz]); mode 2: optional node_ids [N]
Index index_of(int64_t mode, const c10::optional<torch::Tensor>& indptr, const c10::optional<torch::Tensor>& values,
               const c10::optional<torch::Tensor>& node_ids, const Operands& c) {
  TORCH_CHECK(mode >= 0 && mode <= 2, "node_bag: mode must be 0 (bag_sum), 1 (bag_mean) or 2 (id)");
  Index ix;
  if (mode == 2) {
    if (node_ids.has_value()) {
      c.i64(*node_ids, "node_ids");
      ix.node_ids = node_ids->data_ptr<int64_t>();
      ix.num_rows = node_ids->numel();
    }
    return ix;
  }
  TORCH_CHECK(indptr.has_value() && values.has_value(), "node_bag: the bag modes need the CSR (indptr, values)");
  c.i64(*indptr, "indptr");
  c.i64(*values, "values");
  TORCH_CHECK(indptr->numel() >= 1, "node_bag: indptr must be [N + 1]");
  ix.indptr = indptr->data_ptr<int64_t>();
  ix.values = values->data_ptr<int64_t>();
  ix.nnz = values->numel();
  ix.num_rows = indptr->numel() - 1;
  return ix;
}

void node_bag_fwd(torch::Tensor rows, c10::optional<torch::Tensor> indptr, c10::optional<torch::Tensor> values,
                  c10::optional<torch::Tensor> node_ids, torch::Tensor table, torch::Tensor out, int64_t col,
                  int64_t mode, bool hash) {
  const Operands c("node_bag_fwd", table, "table");
  c.f32(table, "table");
  TORCH_CHECK(table.dim() == 2 && table.size(0) >= 1 && table.size(1) >= 1, "node_bag: table must be [V, D]");
  c.i64(rows, "rows");
  c.f32(out, "out");
  const int64_t n = rows.numel(), D = table.size(1);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == n && col >= 0 && col + D <= out.size(1),
              "node_bag: out must be [n, ld] with col + D <= ld");
  const Index ix = index_of(mode, indptr, values, node_ids, c);
  const auto g = c.guard();
  launch_ok(eh_node_bag_fwd(rows.data_ptr<int64_t>(), n, ix.indptr, ix.values, ix.nnz, ix.node_ids,
                                       ix.num_rows, table.data_ptr<float>(), table.size(0), static_cast<int>(D),
                                       out.data_ptr<float>(), out.size(1), col, static_cast<int>(mode), hash ? 1 : 0,
                                       cur_stream()),
            "node_bag_fwd");
}

// adds the table gradient of out[:, col : col + D] into dtable [V, D] (fp32, zeroed by the caller)
void node_bag_bwd_(torch::Tensor dtable, torch::Tensor rows, c10::optional<torch::Tensor> indptr,
                   c10::optional<torch::Tensor> values, c10::optional<torch::Tensor> node_ids, torch::Tensor dout,
                   int64_t col, int64_t mode, bool hash) {
  const Operands c("node_bag_bwd_", dtable, "dtable");
  c.f32(dtable, "dtable");
  TORCH_CHECK(dtable.dim() == 2 && dtable.size(0) >= 1 && dtable.size(1) >= 1, "node_bag: dtable must be [V, D]");
  c.i64(rows, "rows");
  c.f32(dout, "dout");
  const int64_t n = rows.numel(), D = dtable.size(1);
  TORCH_CHECK(dout.dim() == 2 && dout.size(0) == n && col >= 0 && col + D <= dout.size(1),
              "node_bag: dout must be [n, ld] with col + D <= ld");
  const Index ix = index_of(mode, indptr, values, node_ids, c);
  const auto g = c.guard();
  launch_ok(eh_node_bag_bwd(rows.data_ptr<int64_t>(), n, ix.indptr, ix.values, ix.nnz, ix.node_ids,
                                       ix.num_rows, dout.data_ptr<float>(), dout.size(1), col, dtable.size(0),
                                       static_cast<int>(D), dtable.data_ptr<float>(), static_cast<int>(mode),
                                       hash ? 1 : 0, cur_stream()),
            "node_bag_bwd");
}

}  // namespace

void register_node_embed_ops(py::module& m) {
  m.def("node_bag_fwd", &node_bag_fwd, py::arg("rows"), py::arg("indptr"), py::arg("values"), py::arg("node_ids"),
        py::arg("table"), py::arg("out"), py::arg("col"), py::arg("mode"), py::arg("hash"));
  m.def("node_bag_bwd_", &node_bag_bwd_, py::arg("dtable"), py::arg("rows"), py::arg("indptr"), py::arg("values"),
        py::arg("node_ids"), py::arg("dout"), py::arg("col"), py::arg("mode"), py::arg("hash"));
}
