// torch binding of the edge-list -> CSR kernels (graph_build.hip; DeviceGraph.from_edges).
// Host-only; operands go through binding_util.h (rules R1-R3 there).  Outputs and hipcub
// scratch are allocated here (torch's caching allocator), never inside a launcher.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

// every tensor operand of the graph build is one-dimensional
void flat(const Operands& c, const torch::Tensor& t, c10::ScalarType st, const char* name) {
  c.is(t, st, name);
  TORCH_CHECK(t.dim() == 1, "graph_build: ", name, " must be one-dimensional");
}

int is64(const Operands& c, const torch::Tensor& t, const char* name) {
  const bool i64 = c.i64_or_i32(t, name);
  TORCH_CHECK(t.dim() == 1, "graph_build: ", name, " must be one-dimensional");
  return i64 ? 1 : 0;
}

void check_layout(int64_t N, int64_t T, int64_t dst_bits) {
  TORCH_CHECK(N >= 1 && N < (int64_t{1} << 31), "graph_build: N must be in [1, 2^31)");
  TORCH_CHECK(T >= 1 && T <= 32, "graph_build: num_types must be in [1, 32]");
  TORCH_CHECK(dst_bits >= 1 && dst_bits <= 31 && ((N - 1) >> dst_bits) == 0, "graph_build: dst_bits too small for N");
  TORCH_CHECK(((N * T) >> (63 - dst_bits)) == 0, "graph_build: the packed key needs more than 63 bits");
}

void check_status(const Operands& c, const torch::Tensor& status) {
  flat(c, status, torch::kInt64, "status");
  TORCH_CHECK(status.numel() == 4, "graph_build: status must be int64 [4]");
}

// (keys int64 [E2], idx int32 [E2]), E2 = E or 2 E
std::vector<torch::Tensor> graph_build_pack(torch::Tensor src, torch::Tensor dst, c10::optional<torch::Tensor> weight,
                                            c10::optional<torch::Tensor> etype, c10::optional<torch::Tensor> ids,
                                            int64_t N, int64_t T, int64_t dst_bits, bool symmetric,
                                            torch::Tensor status) {
  const Operands c("graph_build_pack", src, "src");
  const int s64 = is64(c, src, "src"), d64 = is64(c, dst, "dst");
  const int64_t E = src.numel();
  TORCH_CHECK(dst.numel() == E, "graph_build_pack: src and dst differ in length");
  TORCH_CHECK(E >= 1 && E * (symmetric ? 2 : 1) < (int64_t{1} << 31), "graph_build_pack: edge count out of range");
  check_layout(N, T, dst_bits);
  check_status(c, status);
  const float* w = nullptr;
  const int32_t* et = nullptr;
  const int64_t* idp = nullptr;
  if (weight.has_value()) {
    flat(c, *weight, torch::kFloat32, "weight");
    TORCH_CHECK(weight->numel() == E, "graph_build_pack: weight must be [E]");
    w = weight->data_ptr<float>();
  }
  if (etype.has_value()) {
    flat(c, *etype, torch::kInt32, "edge_type");
    TORCH_CHECK(etype->numel() == E, "graph_build_pack: edge_type must be [E]");
    et = etype->data_ptr<int32_t>();
  }
  if (ids.has_value()) {
    flat(c, *ids, torch::kInt64, "ids");
    TORCH_CHECK(ids->numel() == N, "graph_build_pack: ids must be [N]");
    idp = ids->data_ptr<int64_t>();
  }
  const auto g = c.guard();
  const int64_t E2 = E * (symmetric ? 2 : 1);
  auto keys = torch::empty({E2}, src.options().dtype(torch::kInt64));
  auto idx = torch::empty({E2}, src.options().dtype(torch::kInt32));
  launch_ok(eh_gb_pack(src.data_ptr(), s64, dst.data_ptr(), d64, w, et, idp, N, static_cast<int>(T),
                       static_cast<int>(dst_bits), E, symmetric ? 1 : 0, keys.data_ptr<int64_t>(),
                       idx.data_ptr<int32_t>(), status.data_ptr<int64_t>(), cur_stream()),
            "edge_pack");
  return {keys, idx};
}

// stable radix sort of (keys, idx) over the bits [0, end_bit).  keys / idx are consumed: they
// and one new pair of the same size are the sort's ping-pong buffers, the pair that ends up
// holding the result is returned (12 B per edge beyond the input pair, not 24)
std::vector<torch::Tensor> graph_build_sort(torch::Tensor keys, torch::Tensor idx, int64_t end_bit) {
  const Operands c("graph_build_sort", keys, "keys");
  flat(c, keys, torch::kInt64, "keys");
  flat(c, idx, torch::kInt32, "idx");
  const int64_t n = keys.numel();
  TORCH_CHECK(idx.numel() == n && n >= 1 && n < (int64_t{1} << 31), "graph_build_sort: keys / idx must be [n], n < 2^31");
  TORCH_CHECK(end_bit >= 1 && end_bit <= 63, "graph_build_sort: end_bit must be in [1, 63]");
  const auto g = c.guard();
  auto ko = torch::empty_like(keys);
  auto io = torch::empty_like(idx);
  size_t bytes = 0;
  int in_b = 0;
  launch_ok(eh_gb_sort(keys.data_ptr<int64_t>(), ko.data_ptr<int64_t>(), idx.data_ptr<int32_t>(),
                       io.data_ptr<int32_t>(), n, static_cast<int>(end_bit), nullptr, &bytes, &in_b, cur_stream()),
            "edge_sort (size query)");
  auto temp = torch::empty({static_cast<int64_t>(bytes > 0 ? bytes : 1)}, keys.options().dtype(torch::kUInt8));
  launch_ok(eh_gb_sort(keys.data_ptr<int64_t>(), ko.data_ptr<int64_t>(), idx.data_ptr<int32_t>(),
                       io.data_ptr<int32_t>(), n, static_cast<int>(end_bit), temp.data_ptr(), &bytes, &in_b,
                       cur_stream()),
            "edge_sort");
  // the ping-pong pair that holds the result; the caller drops the other one
  return in_b ? std::vector<torch::Tensor>{ko, io} : std::vector<torch::Tensor>{keys, idx};
}

// incl int32 [n]: inclusive count of run heads; status[2] receives the number of runs
torch::Tensor graph_build_heads(torch::Tensor keys, torch::Tensor status) {
  const Operands c("graph_build_heads", keys, "keys");
  flat(c, keys, torch::kInt64, "keys");
  check_status(c, status);
  const int64_t n = keys.numel();
  TORCH_CHECK(n >= 1 && n < (int64_t{1} << 31), "graph_build_heads: n must be in [1, 2^31)");
  const auto g = c.guard();
  auto head = torch::empty({n}, keys.options().dtype(torch::kInt32));
  auto incl = torch::empty({n}, keys.options().dtype(torch::kInt32));
  size_t bytes = 0;
  launch_ok(eh_gb_heads(keys.data_ptr<int64_t>(), n, head.data_ptr<int32_t>(), incl.data_ptr<int32_t>(),
                        status.data_ptr<int64_t>(), nullptr, &bytes, cur_stream()),
            "edge_heads (size query)");
  auto temp = torch::empty({static_cast<int64_t>(bytes > 0 ? bytes : 1)}, keys.options().dtype(torch::kUInt8));
  launch_ok(eh_gb_heads(keys.data_ptr<int64_t>(), n, head.data_ptr<int32_t>(), incl.data_ptr<int32_t>(),
                        status.data_ptr<int64_t>(), temp.data_ptr(), &bytes, cur_stream()),
            "edge_heads");
  return incl;
}

// (ckeys int64 [nnz], cidx int32 [nnz], cw fp32 [nnz]) of the runs of equal sorted keys
std::vector<torch::Tensor> graph_build_compact(torch::Tensor keys, torch::Tensor idx, torch::Tensor incl,
                                               c10::optional<torch::Tensor> weight, int64_t E, int64_t nnz) {
  const Operands c("graph_build_compact", keys, "keys");
  flat(c, keys, torch::kInt64, "keys");
  flat(c, idx, torch::kInt32, "idx");
  flat(c, incl, torch::kInt32, "incl");
  const int64_t n = keys.numel();
  TORCH_CHECK(idx.numel() == n && incl.numel() == n && n >= 1, "graph_build_compact: keys / idx / incl must be [n]");
  TORCH_CHECK(nnz >= 1 && nnz <= n, "graph_build_compact: nnz must be in [1, n]");
  TORCH_CHECK(E >= 1 && (n == E || n == 2 * E), "graph_build_compact: n must be E or 2 E");
  const float* w = nullptr;
  if (weight.has_value()) {
    flat(c, *weight, torch::kFloat32, "weight");
    TORCH_CHECK(weight->numel() == E, "graph_build_compact: weight must be [E]");
    w = weight->data_ptr<float>();
  }
  const auto g = c.guard();
  auto ck = torch::empty({nnz}, keys.options());
  auto ci = torch::empty({nnz}, idx.options());
  auto cw = torch::empty({nnz}, keys.options().dtype(torch::kFloat32));
  launch_ok(eh_gb_compact(keys.data_ptr<int64_t>(), idx.data_ptr<int32_t>(), incl.data_ptr<int32_t>(), n, w, E, nnz,
                          ck.data_ptr<int64_t>(), ci.data_ptr<int32_t>(), cw.data_ptr<float>(), cur_stream()),
            "edge_compact");
  return {ck, ci, cw};
}

// (indptr int64 [N T + 1], nbr int32 [nnz], cumw fp32 [nnz]) of sorted keys.  perm given:
// slot i is input edge perm[i] (weight [E] or none = 1); perm absent: weight [nnz] per slot
std::vector<torch::Tensor> graph_build_csr(torch::Tensor keys, c10::optional<torch::Tensor> perm,
                                           c10::optional<torch::Tensor> weight, int64_t E, int64_t N, int64_t T,
                                           int64_t dst_bits) {
  const Operands c("graph_build_csr", keys, "keys");
  flat(c, keys, torch::kInt64, "keys");
  const int64_t nnz = keys.numel();
  check_layout(N, T, dst_bits);
  TORCH_CHECK(nnz < (int64_t{1} << 31), "graph_build_csr: nnz must be < 2^31");
  const float* w = nullptr;
  const int32_t* pp = nullptr;
  if (perm.has_value()) {
    flat(c, *perm, torch::kInt32, "perm");
    TORCH_CHECK(perm->numel() == nnz && E >= 0 && nnz <= 2 * E, "graph_build_csr: perm must be [nnz], nnz <= 2 E");
    pp = perm->data_ptr<int32_t>();
  }
  if (weight.has_value()) {
    flat(c, *weight, torch::kFloat32, "weight");
    TORCH_CHECK(weight->numel() == (pp ? E : nnz), "graph_build_csr: weight must be [E] with perm, [nnz] without");
    w = weight->data_ptr<float>();
  }
  TORCH_CHECK(pp != nullptr || w != nullptr || nnz == 0, "graph_build_csr: perm or per-slot weight required");
  const auto g = c.guard();
  auto indptr = torch::empty({N * T + 1}, keys.options());
  auto nbr = torch::empty({nnz}, keys.options().dtype(torch::kInt32));
  auto cumw = torch::empty({nnz}, keys.options().dtype(torch::kFloat32));
  launch_ok(eh_gb_csr(keys.data_ptr<int64_t>(), nnz, N, static_cast<int>(T), static_cast<int>(dst_bits), w, pp, E,
                      indptr.data_ptr<int64_t>(), nbr.data_ptr<int32_t>(), cumw.data_ptr<float>(), cur_stream()),
            "csr_bounds / seg_prefix");
  return {indptr, nbr, cumw};
}

}  // namespace

void register_graph_build_ops(py::module& m) {
  m.def("graph_build_pack", &graph_build_pack, py::arg("src"), py::arg("dst"), py::arg("weight"), py::arg("etype"),
        py::arg("ids"), py::arg("N"), py::arg("T"), py::arg("dst_bits"), py::arg("symmetric"), py::arg("status"));
  m.def("graph_build_sort", &graph_build_sort, py::arg("keys"), py::arg("idx"), py::arg("end_bit"));
  m.def("graph_build_heads", &graph_build_heads, py::arg("keys"), py::arg("status"));
  m.def("graph_build_compact", &graph_build_compact, py::arg("keys"), py::arg("idx"), py::arg("incl"),
        py::arg("weight"), py::arg("E"), py::arg("nnz"));
  m.def("graph_build_csr", &graph_build_csr, py::arg("keys"), py::arg("perm"), py::arg("weight"), py::arg("E"),
        py::arg("N"), py::arg("T"), py::arg("dst_bits"));
  m.attr("graph_build_short_len") = eh_gb_short_len();
  m.attr("graph_build_wave_len") = eh_gb_wave_len();
}
