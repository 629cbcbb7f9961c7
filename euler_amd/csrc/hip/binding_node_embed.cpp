// torch binding of the node-row embedding-bag kernels (node_embed.hip).  Host-only
// translation unit: every operand is validated (dtype, device, contiguity, the sizes the
// kernels index with) before a launch on torch's current stream; nothing is allocated in
// the forward and nothing synchronises, so both ops capture into a hipGraph.
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/extension.h>

#include "hip/launchers.h"

namespace py = pybind11;

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

void need(const torch::Tensor& t, c10::ScalarType st, const torch::Device& dev, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, "node_bag: ", name, " must be on the table's GPU");
  TORCH_CHECK(t.is_contiguous(), "node_bag: ", name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == st, "node_bag: ", name, " has the wrong dtype");
}

struct Index {
  const int64_t* indptr = nullptr;
  const int64_t* values = nullptr;
  const int64_t* node_ids = nullptr;
  int64_t nnz = 0, num_rows = -1;
};

// mode 0 / 1: (indptr [N + 1], values [nnz]); mode 2: optional node_ids [N]
Index index_of(int64_t mode, const c10::optional<torch::Tensor>& indptr, const c10::optional<torch::Tensor>& values,
               const c10::optional<torch::Tensor>& node_ids, const torch::Device& dev) {
  TORCH_CHECK(mode >= 0 && mode <= 2, "node_bag: mode must be 0 (bag_sum), 1 (bag_mean) or 2 (id)");
  Index ix;
  if (mode == 2) {
    if (node_ids.has_value()) {
      need(*node_ids, torch::kInt64, dev, "node_ids");
      ix.node_ids = node_ids->data_ptr<int64_t>();
      ix.num_rows = node_ids->numel();
    }
    return ix;
  }
  TORCH_CHECK(indptr.has_value() && values.has_value(), "node_bag: the bag modes need the CSR (indptr, values)");
  need(*indptr, torch::kInt64, dev, "indptr");
  need(*values, torch::kInt64, dev, "values");
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
  TORCH_CHECK(table.is_cuda() && table.dim() == 2 && table.is_contiguous() &&
                  table.scalar_type() == torch::kFloat32 && table.size(0) >= 1 && table.size(1) >= 1,
              "node_bag: table must be a contiguous fp32 [V, D] GPU tensor");
  const torch::Device dev = table.device();
  need(rows, torch::kInt64, dev, "rows");
  need(out, torch::kFloat32, dev, "out");
  const int64_t n = rows.numel(), D = table.size(1);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == n && col >= 0 && col + D <= out.size(1),
              "node_bag: out must be [n, ld] with col + D <= ld");
  const Index ix = index_of(mode, indptr, values, node_ids, dev);
  const c10::DeviceGuard g(dev);
  const hipError_t e = eh_node_bag_fwd(rows.data_ptr<int64_t>(), n, ix.indptr, ix.values, ix.nnz, ix.node_ids,
                                       ix.num_rows, table.data_ptr<float>(), table.size(0), static_cast<int>(D),
                                       out.data_ptr<float>(), out.size(1), col, static_cast<int>(mode), hash ? 1 : 0,
                                       stream());
  TORCH_CHECK(e == hipSuccess, "euler_amd HIP kernel 'node_bag_fwd' failed: ", hipGetErrorString(e));
}

// adds the table gradient of out[:, col : col + D] into dtable [V, D] (fp32, zeroed by the caller)
void node_bag_bwd_(torch::Tensor dtable, torch::Tensor rows, c10::optional<torch::Tensor> indptr,
                   c10::optional<torch::Tensor> values, c10::optional<torch::Tensor> node_ids, torch::Tensor dout,
                   int64_t col, int64_t mode, bool hash) {
  TORCH_CHECK(dtable.is_cuda() && dtable.dim() == 2 && dtable.is_contiguous() &&
                  dtable.scalar_type() == torch::kFloat32 && dtable.size(0) >= 1 && dtable.size(1) >= 1,
              "node_bag: dtable must be a contiguous fp32 [V, D] GPU tensor");
  const torch::Device dev = dtable.device();
  need(rows, torch::kInt64, dev, "rows");
  need(dout, torch::kFloat32, dev, "dout");
  const int64_t n = rows.numel(), D = dtable.size(1);
  TORCH_CHECK(dout.dim() == 2 && dout.size(0) == n && col >= 0 && col + D <= dout.size(1),
              "node_bag: dout must be [n, ld] with col + D <= ld");
  const Index ix = index_of(mode, indptr, values, node_ids, dev);
  const c10::DeviceGuard g(dev);
  const hipError_t e = eh_node_bag_bwd(rows.data_ptr<int64_t>(), n, ix.indptr, ix.values, ix.nnz, ix.node_ids,
                                       ix.num_rows, dout.data_ptr<float>(), dout.size(1), col, dtable.size(0),
                                       static_cast<int>(D), dtable.data_ptr<float>(), static_cast<int>(mode),
                                       hash ? 1 : 0, stream());
  TORCH_CHECK(e == hipSuccess, "euler_amd HIP kernel 'node_bag_bwd' failed: ", hipGetErrorString(e));
}

}  // namespace

void register_node_embed_ops(py::module& m) {
  m.def("node_bag_fwd", &node_bag_fwd, py::arg("rows"), py::arg("indptr"), py::arg("values"), py::arg("node_ids"),
        py::arg("table"), py::arg("out"), py::arg("col"), py::arg("mode"), py::arg("hash"));
  m.def("node_bag_bwd_", &node_bag_bwd_, py::arg("dtable"), py::arg("rows"), py::arg("indptr"), py::arg("values"),
        py::arg("node_ids"), py::arg("dout"), py::arg("col"), py::arg("mode"), py::arg("hash"));
}
