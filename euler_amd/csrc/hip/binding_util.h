// The one operand-validation layer of the torch bindings (binding*.cpp).  Host-only: torch,
// pybind11 and the HIP runtime API; no .hip file includes it.
//
// Rules every exported op and every plan constructor keeps (docs/DESIGN.md, "Binding rules"):
//   R1  every tensor operand is validated before any allocation or launch: a GPU tensor, on
//       the anchor's device, of the required dtype, contiguous, with the element count the
//       grid assumes;
//   R2  the launch runs under a DeviceGuard on the anchor's device, and the stream is read
//       after the guard is in place;
//   R3  a violation is a RuntimeError naming the op / plan and the operand / dict key (a dtype
//       mismatch also names the found and the expected dtype);
//   R4  per-step plan methods only launch.
#pragma once

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/extension.h>

#include <string>
#include <vector>

namespace py = pybind11;

// ----------------------------------------------------------------------------- registration
// binding_gnn.cpp: GAT / R-GCN / embedding-loss / unique kernels
void register_gnn_ops(py::module& m);
// binding_tree.cpp: fused GraphSAGE tree-step plan
void register_tree_ops(py::module& m);
// binding_gcn.cpp: fused GCN step plan
void register_gcn_ops(py::module& m);
// binding_graph_cls.cpp: fused graph-classification step plan
void register_graph_cls_ops(py::module& m);
// binding_node_embed.cpp: node rows -> embedding bags (sparse-feature / id inputs)
void register_node_embed_ops(py::module& m);
// binding_walk_shard.cpp: the hop kernels of random walks over the row-sharded graph
void register_walk_shard_ops(py::module& m);
// binding_knn.cpp: fused distance + top-k search (flat and IVF)
void register_knn_ops(py::module& m);
// binding_kg_rank.cpp: link-prediction rank counts (fused score + compare + filter scan)
void register_kg_rank_ops(py::module& m);
// binding_sage_csr.cpp: full-neighbourhood GraphSAGE layer over the graph's CSR (layer-wise inference)
void register_sage_csr_ops(py::module& m);
// binding_graph_build.cpp: edge list -> device CSR (DeviceGraph.from_edges)
void register_graph_build_ops(py::module& m);
// binding_frontier.cpp: row sets of frontier inference and the layer over a set's compact table
// (registered on the submodule _hip_ops.frontier)
void register_frontier_ops(py::module& m);

namespace euler_bind {

// ----------------------------------------------------------------------------- stream, launch result
// torch's current HIP stream on the current device: read it after the DeviceGuard (R2)
inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void launch_ok(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "euler_amd HIP kernel '", what, "' failed: ", hipGetErrorString(e));
}

// ----------------------------------------------------------------------------- per-call operand checker
// Built from the op's name and its anchor (with the anchor's operand name): the operand whose
// device the launch uses, which must be a GPU tensor.  Every operand, the anchor included, goes
// through one of the forms below before anything else happens; guard() then hands out the
// DeviceGuard.  The typed forms also take a c10::optional operand: an absent one passes.
class Operands {
 public:
  Operands(const char* op, const torch::Tensor& anchor, const char* anchor_name)
      : op_(op), dev_(anchor.device()) {
    placed(anchor, anchor_name);
  }
  // ops whose device is not an operand's (XgmiAr::run, synth_csr)
  Operands(const char* op, c10::Device dev) : op_(op), dev_(dev) {}

  // a contiguous GPU tensor on the anchor's device, any dtype
  void any(const torch::Tensor& t, const char* name) const {
    placed(t, name);
    TORCH_CHECK(t.is_contiguous(), op_, ": ", name, " must be contiguous");
  }
  void is(const torch::Tensor& t, c10::ScalarType st, const char* name) const {
    any(t, name);
    TORCH_CHECK(t.scalar_type() == st, op_, ": ", name, " has dtype ", t.scalar_type(), ", expected ", st);
  }
  // true: bfloat16, false: float32
  bool bf16_or_f32(const torch::Tensor& t, const char* name) const {
    any(t, name);
    return is_bf16(t, name);
  }
  // true: int64, false: int32
  bool i64_or_i32(const torch::Tensor& t, const char* name) const {
    any(t, name);
    TORCH_CHECK(t.scalar_type() == torch::kInt64 || t.scalar_type() == torch::kInt32, op_, ": ", name, " has dtype ",
                t.scalar_type(), ", expected ", torch::kInt64, " or ", torch::kInt32);
    return t.scalar_type() == torch::kInt64;
  }
  // The one exception to contiguity: a 2-D fp32 / bf16 matrix with unit inner stride and any
  // row stride (gemm's operands).  true: bfloat16
  bool strided_matrix(const torch::Tensor& t, const char* name) const {
    placed(t, name);
    TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, op_, ": ", name, " must be a 2-D matrix with unit inner stride");
    return is_bf16(t, name);
  }

  void is(const c10::optional<torch::Tensor>& t, c10::ScalarType st, const char* name) const {
    if (t.has_value()) is(*t, st, name);
  }
  template <typename T>
  void i32(const T& t, const char* name) const { is(t, torch::kInt32, name); }
  template <typename T>
  void i64(const T& t, const char* name) const { is(t, torch::kInt64, name); }
  template <typename T>
  void f32(const T& t, const char* name) const { is(t, torch::kFloat32, name); }
  template <typename T>
  void bf16(const T& t, const char* name) const { is(t, torch::kBFloat16, name); }

  // the launch's DeviceGuard (R2); take it after the checks, read the stream after it
  c10::DeviceGuard guard() const {
    TORCH_CHECK(dev_.is_cuda(), op_, ": launches need a GPU device, got ", dev_);
    return c10::DeviceGuard(dev_);
  }

 private:
  const char* op_;
  c10::Device dev_;

  void placed(const torch::Tensor& t, const char* name) const {
    TORCH_CHECK(t.is_cuda(), op_, ": ", name, " must be a GPU tensor, got one on ", t.device());
    TORCH_CHECK(t.device() == dev_, op_, ": ", name, " is on ", t.device(), ", the launch is on ", dev_);
  }
  bool is_bf16(const torch::Tensor& t, const char* name) const {
    TORCH_CHECK(t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kFloat32, op_, ": ", name,
                " has dtype ", t.scalar_type(), ", expected ", torch::kBFloat16, " or ", torch::kFloat32);
    return t.scalar_type() == torch::kBFloat16;
  }
};

// ----------------------------------------------------------------------------- plan dicts
// The dict a plan class is built from: typed access to its sizes and tensors, and the plan's
// own buffers.  The plan's device is fixed once, by the first tensor need() sees (or given up
// front); every later tensor must live there, and buffers are allocated there.  Hidden
// visibility, as for every type that holds a pybind11 object.
class __attribute__((visibility("hidden"))) PlanDict {
 public:
  PlanDict(py::dict d, const char* plan) : d_(d), plan_(plan) {}
  PlanDict(py::dict d, const char* plan, c10::Device dev) : d_(d), plan_(plan), dev_(dev) {
    TORCH_CHECK(dev_.is_cuda(), plan_, ": the plan's device must be a GPU, got ", dev_);
  }

  const char* name() const { return plan_; }
  c10::Device device() const { return dev_; }

  bool has(const char* k) const { return d_.contains(k) && !d_[k].is_none(); }
  // a required entry of any type
  py::object item(const char* k) const {
    TORCH_CHECK(has(k), plan_, ": missing '", k, "'");
    return d_[k];
  }
  int64_t geti(const char* k) const { return item(k).cast<int64_t>(); }
  double getf(const char* k) const { return item(k).cast<double>(); }
  std::vector<int64_t> getv(const char* k) const { return item(k).cast<std::vector<int64_t>>(); }
  torch::Tensor T(const char* k) const {
    TORCH_CHECK(has(k), plan_, ": missing tensor '", k, "'");
    return d_[k].cast<torch::Tensor>();
  }
  torch::Tensor T(const std::string& k) const { return T(k.c_str()); }

  // a contiguous tensor on the plan's GPU, any dtype
  void need_any(const torch::Tensor& t, const std::string& name) {
    TORCH_CHECK(t.is_cuda(), plan_, ": '", name, "' must be a GPU tensor, got one on ", t.device());
    if (!dev_.is_cuda()) dev_ = t.device();
    TORCH_CHECK(t.device() == dev_, plan_, ": '", name, "' is on ", t.device(), ", the plan is on ", dev_);
    TORCH_CHECK(t.is_contiguous(), plan_, ": '", name, "' must be contiguous");
  }
  // numel < 0: any element count
  void need(const torch::Tensor& t, c10::ScalarType st, int64_t numel, const std::string& name) {
    need_any(t, name);
    TORCH_CHECK(t.scalar_type() == st, plan_, ": '", name, "' has dtype ", t.scalar_type(), ", expected ", st);
    TORCH_CHECK(numel < 0 || t.numel() == numel, plan_, ": '", name, "' has ", t.numel(), " elements, expected ",
                numel);
  }
  // bfloat16 (true) or float32 (false)
  bool need_bf16_or_f32(const torch::Tensor& t, int64_t numel, const std::string& name) {
    const bool bf = t.scalar_type() == torch::kBFloat16;
    need(t, bf ? torch::kBFloat16 : torch::kFloat32, numel, name);
    return bf;
  }
  template <typename P>
  P* ptr(const std::string& k, c10::ScalarType st, int64_t numel) {
    torch::Tensor t = T(k);
    need(t, st, numel, k);
    return reinterpret_cast<P*>(t.data_ptr());
  }
  uint16_t* bf(const std::string& k, int64_t numel) { return ptr<uint16_t>(k, torch::kBFloat16, numel); }
  float* f32(const std::string& k, int64_t numel) { return ptr<float>(k, torch::kFloat32, numel); }
  int32_t* i32(const std::string& k, int64_t numel) { return ptr<int32_t>(k, torch::kInt32, numel); }

  // plan-owned buffers on the plan's device; the plan keeps them alive
  torch::Tensor zeros(int64_t n, c10::ScalarType st) { return own(torch::zeros({n}, options(st))); }
  torch::Tensor full(int64_t n, int64_t v, c10::ScalarType st) { return own(torch::full({n}, v, options(st))); }
  torch::Tensor empty(int64_t n, c10::ScalarType st) { return own(torch::empty({n}, options(st))); }
  template <typename P>
  P* zeros_ptr(int64_t n, c10::ScalarType st) { return reinterpret_cast<P*>(zeros(n, st).data_ptr()); }

 private:
  py::dict d_;
  const char* plan_;
  c10::Device dev_{c10::kCPU};
  std::vector<torch::Tensor> owned_;

  torch::TensorOptions options(c10::ScalarType st) const {
    TORCH_CHECK(dev_.is_cuda(), plan_, ": no tensor has fixed the plan's device yet");
    return torch::TensorOptions().dtype(st).device(dev_);
  }
  torch::Tensor own(torch::Tensor t) {
    owned_.push_back(t);
    return t;
  }
};

}  // namespace euler_bind
