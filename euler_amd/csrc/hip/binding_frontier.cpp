// torch binding of the frontier row sets (frontier.hip) and of the full-neighbourhood layer
// over a set's compact table (sage_csr.hip, eh_sage_csr_fwd_mapped).  Host-only; operands go
// through binding_util.h (rules R1-R3 there).  Exported on the submodule _hip_ops.frontier.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

void check_rows(int64_t N, const char* op) {
  TORCH_CHECK(N >= 1 && N < (int64_t{1} << 31), op, ": num_rows must be in [1, 2^31), got ", N);
}

// set_words int32 [ceil(N / 32), 2]: the set's rank bitmap
void check_words(const Operands& c, const torch::Tensor& words, int64_t N, const char* op) {
  c.i32(words, "set_words");
  TORCH_CHECK(words.dim() == 2 && words.size(0) == eh_frontier_words(N) && words.size(1) == 2, op,
              ": set_words must be [ceil(num_rows / 32) = ", eh_frontier_words(N), ", 2]");
}

void check_list(const Operands& c, const torch::Tensor& rows, const char* op) {
  c.i32(rows, "rows");
  TORCH_CHECK(rows.dim() == 1, op, ": rows must be one-dimensional");
}

// sets the bits of rows (entries outside [0, num_rows) are ignored)
void mark_rows(torch::Tensor set_words, torch::Tensor rows, int64_t num_rows) {
  const Operands c("mark_rows", set_words, "set_words");
  check_rows(num_rows, "mark_rows");
  check_words(c, set_words, num_rows, "mark_rows");
  check_list(c, rows, "mark_rows");
  const auto g = c.guard();
  if (rows.numel() == 0) return;
  launch_ok(eh_frontier_mark(set_words.data_ptr<int32_t>(), num_rows, rows.data_ptr<int32_t>(), rows.numel(),
                             cur_stream()),
            "mark_rows");
}

// sets the bits of the neighbours of rows over the masked segments of the CSR
void mark_neighbors(torch::Tensor set_words, torch::Tensor indptr, torch::Tensor nbr, int64_t num_types, int64_t mask,
                    torch::Tensor rows) {
  const Operands c("mark_neighbors", set_words, "set_words");
  c.i64(indptr, "indptr");
  c.i32(nbr, "nbr");
  TORCH_CHECK(num_types >= 1 && num_types <= 32, "mark_neighbors: 1 to 32 edge types, got ", num_types);
  TORCH_CHECK(mask >= 0 && mask <= 0xFFFFFFFFLL, "mark_neighbors: mask is a 32-bit edge-type set");
  TORCH_CHECK(indptr.dim() == 1 && indptr.numel() >= num_types + 1 && (indptr.numel() - 1) % num_types == 0,
              "mark_neighbors: indptr must be [N * T + 1]");
  const int64_t N = (indptr.numel() - 1) / num_types;
  check_rows(N, "mark_neighbors");
  check_words(c, set_words, N, "mark_neighbors");
  TORCH_CHECK(nbr.dim() == 1, "mark_neighbors: nbr must be [E]");
  check_list(c, rows, "mark_neighbors");
  const auto g = c.guard();
  if (rows.numel() == 0 || nbr.numel() == 0) return;
  launch_ok(eh_frontier_mark_neighbors(set_words.data_ptr<int32_t>(), indptr.data_ptr<int64_t>(),
                                       nbr.data_ptr<int32_t>(), N, nbr.numel(), static_cast<int>(num_types),
                                       static_cast<uint32_t>(mask), rows.data_ptr<int32_t>(), rows.numel(),
                                       cur_stream()),
            "mark_neighbors");
}

// fills the rank column of set_words; returns the set's size as a device scalar int32 [1]
torch::Tensor rank_words(torch::Tensor set_words, int64_t num_rows) {
  const Operands c("rank_words", set_words, "set_words");
  check_rows(num_rows, "rank_words");
  check_words(c, set_words, num_rows, "rank_words");
  const auto g = c.guard();
  auto opts = set_words.options();
  auto totals = torch::empty({eh_frontier_scan_blocks(num_rows)}, opts);
  auto count = torch::empty({1}, opts);
  launch_ok(eh_frontier_rank(set_words.data_ptr<int32_t>(), num_rows, totals.data_ptr<int32_t>(),
                             count.data_ptr<int32_t>(), cur_stream()),
            "rank_words");
  return count;
}

// the set's rows, ascending: int32 [count] (count as rank_words returned it)
torch::Tensor list_rows(torch::Tensor set_words, int64_t num_rows, int64_t count) {
  const Operands c("list_rows", set_words, "set_words");
  check_rows(num_rows, "list_rows");
  check_words(c, set_words, num_rows, "list_rows");
  TORCH_CHECK(count >= 0 && count <= num_rows, "list_rows: count must be in [0, num_rows], got ", count);
  const auto g = c.guard();
  auto list = torch::empty({count}, set_words.options());
  if (count == 0) return list;
  launch_ok(eh_frontier_list(set_words.data_ptr<int32_t>(), num_rows, count, list.data_ptr<int32_t>(), cur_stream()),
            "list_rows");
  return list;
}

// sage_csr_fwd (binding_sage_csr.cpp) with x [count, Dp] = the rows of a set in list order,
// addressed through set_words; missing int32 [1] counts the reads the set refused
torch::Tensor sage_csr_fwd_mapped(torch::Tensor indptr, torch::Tensor nbr, torch::Tensor cumw, int64_t num_types,
                                  int64_t mask, torch::Tensor x, torch::Tensor set_words, int64_t count,
                                  torch::Tensor missing, torch::Tensor W, c10::optional<torch::Tensor> rows,
                                  double nbr_scale, double self_scale, bool relu, bool out_fp32,
                                  c10::optional<torch::Tensor> out_opt) {
  const char* op = "sage_csr_fwd_mapped";
  const Operands c(op, x, "x");
  c.bf16_or_f32(x, "x");
  TORCH_CHECK(x.dim() == 2, op, ": x must be [count, Dp]");
  c.i64(indptr, "indptr");
  c.i32(nbr, "nbr");
  c.f32(cumw, "cumw");
  c.bf16(W, "W");
  c.i32(missing, "missing");
  TORCH_CHECK(missing.numel() == 1, op, ": missing must be int32 [1]");
  TORCH_CHECK(num_types >= 1 && num_types <= 32, op, ": 1 to 32 edge types, got ", num_types);
  TORCH_CHECK(mask >= 0 && mask <= 0xFFFFFFFFLL, op, ": mask is a 32-bit edge-type set");
  TORCH_CHECK(indptr.dim() == 1 && indptr.numel() >= num_types + 1 && (indptr.numel() - 1) % num_types == 0, op,
              ": indptr must be [N * T + 1]");
  const int64_t N = (indptr.numel() - 1) / num_types, Dp = x.size(1);
  check_rows(N, op);
  check_words(c, set_words, N, op);
  TORCH_CHECK(count >= 0 && count <= N && x.size(0) == count, op, ": x must have count = ", count, " rows (at most ", N,
              "), got ", x.size(0));
  TORCH_CHECK(nbr.dim() == 1 && cumw.dim() == 1 && nbr.numel() == cumw.numel(), op, ": nbr and cumw must be [E]");
  TORCH_CHECK(Dp >= 16 && Dp % 16 == 0 && Dp <= 512, op, ": Dp must be a multiple of 16 in [16, 512], got ", Dp);
  TORCH_CHECK(W.dim() == 2 && W.size(1) == 2 * Dp && W.size(0) >= 64 && W.size(0) % 64 == 0 && W.size(0) <= (1 << 20),
              op, ": W must be [Hp, 2 Dp] with Hp a multiple of 64");
  const int64_t Hp = W.size(0);
  const int32_t* rp = nullptr;
  int64_t M = N;
  if (rows.has_value()) {
    check_list(c, *rows, op);
    M = rows->numel();
    rp = M > 0 ? rows->data_ptr<int32_t>() : nullptr;
  }
  torch::Tensor out;
  if (out_opt.has_value()) {
    out = *out_opt;
    c.is(out, out_fp32 ? torch::kFloat32 : torch::kBFloat16, "out");
    TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == Hp, op, ": out must be [", M, ", ", Hp, "]");
  }
  const auto g = c.guard();
  if (!out_opt.has_value()) {
    out = torch::empty({M, Hp}, x.options().dtype(out_fp32 ? torch::kFloat32 : torch::kBFloat16));
  }
  if (M == 0) return out;
  launch_ok(eh_sage_csr_fwd_mapped(indptr.data_ptr<int64_t>(), nbr.numel() ? nbr.data_ptr<int32_t>() : nullptr,
                                   cumw.numel() ? cumw.data_ptr<float>() : nullptr, N, nbr.numel(),
                                   static_cast<int>(num_types), static_cast<uint32_t>(mask), x.data_ptr(),
                                   x.scalar_type() == torch::kFloat32 ? 1 : 0, static_cast<int>(Dp),
                                   set_words.data_ptr<int32_t>(), count, missing.data_ptr<int32_t>(), rp, M,
                                   W.data_ptr(), static_cast<int>(Hp), static_cast<float>(nbr_scale),
                                   static_cast<float>(self_scale), relu ? 1 : 0, out.data_ptr(), out_fp32 ? 1 : 0,
                                   cur_stream()),
            op);
  return out;
}

}  // namespace

void register_frontier_ops(py::module& m) {
  m.def("mark_rows", &mark_rows, py::arg("set_words"), py::arg("rows"), py::arg("num_rows"));
  m.def("mark_neighbors", &mark_neighbors, py::arg("set_words"), py::arg("indptr"), py::arg("nbr"),
        py::arg("num_types"), py::arg("mask"), py::arg("rows"));
  m.def("rank_words", &rank_words, py::arg("set_words"), py::arg("num_rows"));
  m.def("list_rows", &list_rows, py::arg("set_words"), py::arg("num_rows"), py::arg("count"));
  m.def("sage_csr_fwd_mapped", &sage_csr_fwd_mapped, py::arg("indptr"), py::arg("nbr"), py::arg("cumw"),
        py::arg("num_types"), py::arg("mask"), py::arg("x"), py::arg("set_words"), py::arg("count"),
        py::arg("missing"), py::arg("W"), py::arg("rows") = py::none(), py::arg("nbr_scale") = 1.0,
        py::arg("self_scale") = 0.0, py::arg("relu") = true, py::arg("out_fp32") = false,
        py::arg("out") = py::none());
}
