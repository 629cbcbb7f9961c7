// torch binding of the full-neighbourhood GCN-family layer and its degree counts (gcn_csr.hip).
// Host-only; operands go through binding_util.h (rules R1-R3 there).  The output is allocated
// here (or is the caller's table slice), never inside the launcher.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

void check_csr(const Operands& c, const char* op, const torch::Tensor& indptr, const torch::Tensor& nbr, int64_t N,
               int64_t num_types, int64_t mask) {
  c.i64(indptr, "indptr");
  c.i32(nbr, "nbr");
  TORCH_CHECK(num_types >= 1 && num_types <= 32, op, ": 1 to 32 edge types, got ", num_types);
  TORCH_CHECK(mask >= 0 && mask <= 0xFFFFFFFFLL, op, ": mask is a 32-bit edge-type set");
  TORCH_CHECK(N >= 0 && N < (int64_t{1} << 31), op, ": rows are int32, got N = ", N);
  TORCH_CHECK(indptr.dim() == 1 && indptr.numel() == N * num_types + 1, op, ": indptr must be [N * T + 1] = ",
              N * num_types + 1, " for ", N, " rows, got ", indptr.numel());
  TORCH_CHECK(nbr.dim() == 1, op, ": nbr must be [E]");
}

// out [M, Hp] = c[r] * act(bf16(a[r] * (sum_{masked edges of r} b[nbr] x[nbr] (+ b[r] x[r]))) @ W^T) for
// r = rows[m] (rows None: r = row_start + m, M = row_count; row_count < 0: every row from row_start)
torch::Tensor gcn_csr_fwd(torch::Tensor indptr, torch::Tensor nbr, int64_t num_types, int64_t mask, torch::Tensor x,
                          torch::Tensor W, torch::Tensor tgt_scale, c10::optional<torch::Tensor> src_scale,
                          c10::optional<torch::Tensor> out_scale, c10::optional<torch::Tensor> rows,
                          int64_t row_start, int64_t row_count, bool self_loop, bool relu, bool out_fp32,
                          c10::optional<torch::Tensor> out_opt) {
  const char* op = "gcn_csr_fwd";
  const Operands c(op, x, "x");
  c.bf16_or_f32(x, "x");
  TORCH_CHECK(x.dim() == 2, op, ": x must be [N, Dp]");
  const int64_t N = x.size(0), Dp = x.size(1);
  check_csr(c, op, indptr, nbr, N, num_types, mask);
  c.bf16(W, "W");
  c.f32(tgt_scale, "tgt_scale");
  c.f32(src_scale, "src_scale");
  c.f32(out_scale, "out_scale");
  TORCH_CHECK(Dp >= 16 && Dp % 16 == 0 && Dp <= 512, op, ": Dp must be a multiple of 16 in [16, 512], got ", Dp);
  TORCH_CHECK(W.dim() == 2 && W.size(1) == Dp && W.size(0) >= 64 && W.size(0) % 64 == 0 && W.size(0) <= (1 << 20),
              op, ": W must be [Hp, Dp = ", Dp, "] with Hp a multiple of 64");
  TORCH_CHECK(tgt_scale.numel() == N, op, ": tgt_scale must be [N = ", N, "], got ", tgt_scale.numel());
  TORCH_CHECK(!src_scale.has_value() || src_scale->numel() == N, op, ": src_scale must be [N = ", N, "]");
  TORCH_CHECK(!out_scale.has_value() || out_scale->numel() == N, op, ": out_scale must be [N = ", N, "]");
  const int64_t Hp = W.size(0);
  c.i32(rows, "rows");
  if (out_opt.has_value()) c.is(*out_opt, out_fp32 ? torch::kFloat32 : torch::kBFloat16, "out");
  const auto g = c.guard();  // before the range check of rows: its reduction is a launch too
  const int32_t* rp = nullptr;
  int64_t M;
  if (rows.has_value()) {
    TORCH_CHECK(rows->dim() == 1, op, ": rows must be one-dimensional");
    TORCH_CHECK(row_start == 0 && row_count < 0, op, ": a rows list and a row range exclude each other");
    M = rows->numel();
    if (M > 0) {  // the only host read of an operand's values (a blocking sync): a request's list, no hot loop
      const auto mm = rows->aminmax();
      const int64_t lo = std::get<0>(mm).item<int64_t>(), hi = std::get<1>(mm).item<int64_t>();
      TORCH_CHECK(lo >= 0 && hi < N, op, ": rows must lie in [0, ", N, "), got ", lo, " .. ", hi);
      rp = rows->data_ptr<int32_t>();
    }
  } else {
    M = row_count < 0 ? N - row_start : row_count;
    TORCH_CHECK(row_start >= 0 && M >= 0 && row_start + M <= N, op, ": the row range [", row_start, ", ",
                row_start + M, ") must lie in [0, ", N, "]");
  }
  torch::Tensor out;
  if (out_opt.has_value()) {  // the caller's slice of a layer table
    out = *out_opt;
    TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == Hp, op, ": out must be [", M, ", ", Hp, "]");
  }
  if (!out_opt.has_value()) {
    out = torch::empty({M, Hp}, x.options().dtype(out_fp32 ? torch::kFloat32 : torch::kBFloat16));
  }
  if (M == 0) return out;
  launch_ok(eh_gcn_csr_fwd(indptr.data_ptr<int64_t>(), nbr.numel() ? nbr.data_ptr<int32_t>() : nullptr, N,
                           nbr.numel(), static_cast<int>(num_types), static_cast<uint32_t>(mask), x.data_ptr(),
                           x.scalar_type() == torch::kFloat32 ? 1 : 0, static_cast<int>(Dp),
                           tgt_scale.data_ptr<float>(), src_scale.has_value() ? src_scale->data_ptr<float>() : nullptr,
                           out_scale.has_value() ? out_scale->data_ptr<float>() : nullptr, rp, row_start, M,
                           W.data_ptr(), static_cast<int>(Hp), self_loop ? 1 : 0, relu ? 1 : 0, out.data_ptr(),
                           out_fp32 ? 1 : 0, cur_stream()),
            op);
  return out;
}

// (deg_t [N], deg_s [N]) int32 of one edge-type mask over the CSR of N rows
std::vector<torch::Tensor> gcn_csr_degrees(torch::Tensor indptr, torch::Tensor nbr, int64_t num_rows,
                                           int64_t num_types, int64_t mask) {
  const char* op = "gcn_csr_degrees";
  const Operands c(op, indptr, "indptr");
  check_csr(c, op, indptr, nbr, num_rows, num_types, mask);
  const auto g = c.guard();
  auto deg_t = torch::zeros({num_rows}, indptr.options().dtype(torch::kInt32));
  auto deg_s = torch::zeros({num_rows}, indptr.options().dtype(torch::kInt32));
  if (num_rows == 0) return {deg_t, deg_s};
  launch_ok(eh_gcn_csr_degrees(indptr.data_ptr<int64_t>(), nbr.numel() ? nbr.data_ptr<int32_t>() : nullptr, num_rows,
                               nbr.numel(), static_cast<int>(num_types), static_cast<uint32_t>(mask),
                               deg_t.data_ptr<int32_t>(), deg_s.data_ptr<int32_t>(), cur_stream()),
            op);
  return {deg_t, deg_s};
}

}  // namespace

void register_gcn_csr_ops(py::module& m) {
  m.def("fwd", &gcn_csr_fwd, py::arg("indptr"), py::arg("nbr"), py::arg("num_types"), py::arg("mask"),
        py::arg("x"), py::arg("W"), py::arg("tgt_scale"), py::arg("src_scale") = py::none(),
        py::arg("out_scale") = py::none(), py::arg("rows") = py::none(), py::arg("row_start") = 0,
        py::arg("row_count") = -1, py::arg("self_loop") = true, py::arg("relu") = true, py::arg("out_fp32") = false,
        py::arg("out") = py::none());
  m.def("degrees", &gcn_csr_degrees, py::arg("indptr"), py::arg("nbr"), py::arg("num_rows"),
        py::arg("num_types"), py::arg("mask"));
  m.attr("tile_rows") = eh_gcn_csr_tile_rows();
}
