// torch binding of the full-neighbourhood GraphSAGE layer (sage_csr.hip).  Host-only; operands
// go through binding_util.h (rules R1-R3 there).  The output is allocated here (or is the
// caller's table slice), never inside the launcher.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

// out [M, Hp] = act([x[r] | nbr_scale * wmean_{masked edges of r} x + self_scale * x[r]] @ W^T) for
// r = rows[m] (rows None: r = m, M = N) on the CSR (indptr [N T + 1], nbr [E], cumw [E])
torch::Tensor sage_csr_fwd(torch::Tensor indptr, torch::Tensor nbr, torch::Tensor cumw, int64_t num_types,
                           int64_t mask, torch::Tensor x, torch::Tensor W, c10::optional<torch::Tensor> rows,
                           double nbr_scale, double self_scale, bool relu, bool out_fp32,
                           c10::optional<torch::Tensor> out_opt) {
  const Operands c("sage_csr_fwd", x, "x");
  c.bf16_or_f32(x, "x");
  TORCH_CHECK(x.dim() == 2, "sage_csr_fwd: x must be [N, Dp]");
  c.i64(indptr, "indptr");
  c.i32(nbr, "nbr");
  c.f32(cumw, "cumw");
  c.bf16(W, "W");
  const int64_t N = x.size(0), Dp = x.size(1);
  TORCH_CHECK(num_types >= 1 && num_types <= 32, "sage_csr_fwd: 1 to 32 edge types, got ", num_types);
  TORCH_CHECK(mask >= 0 && mask <= 0xFFFFFFFFLL, "sage_csr_fwd: mask is a 32-bit edge-type set");
  TORCH_CHECK(indptr.dim() == 1 && indptr.numel() == N * num_types + 1, "sage_csr_fwd: indptr must be [N * T + 1] = ",
              N * num_types + 1, " for the ", N, " rows of x, got ", indptr.numel());
  TORCH_CHECK(nbr.dim() == 1 && cumw.dim() == 1 && nbr.numel() == cumw.numel(),
              "sage_csr_fwd: nbr and cumw must be [E]");
  TORCH_CHECK(Dp >= 16 && Dp % 16 == 0 && Dp <= 512, "sage_csr_fwd: Dp must be a multiple of 16 in [16, 512], got ",
              Dp);
  TORCH_CHECK(W.dim() == 2 && W.size(1) == 2 * Dp && W.size(0) >= 64 && W.size(0) % 64 == 0 &&
                  W.size(0) <= (1 << 20),
              "sage_csr_fwd: W must be [Hp, 2 Dp] with Hp a multiple of 64");
  const int64_t Hp = W.size(0);
  const int32_t* rp = nullptr;
  int64_t M = N;
  if (rows.has_value()) {
    c.i32(*rows, "rows");
    TORCH_CHECK(rows->dim() == 1, "sage_csr_fwd: rows must be one-dimensional");
    M = rows->numel();
    rp = M > 0 ? rows->data_ptr<int32_t>() : nullptr;
  }
  torch::Tensor out;
  if (out_opt.has_value()) {  // the caller's slice of a layer table
    out = *out_opt;
    c.is(out, out_fp32 ? torch::kFloat32 : torch::kBFloat16, "out");
    TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == Hp, "sage_csr_fwd: out must be [", M, ", ", Hp,
                "]");
  }
  const auto g = c.guard();
  if (!out_opt.has_value()) {
    out = torch::empty({M, Hp}, x.options().dtype(out_fp32 ? torch::kFloat32 : torch::kBFloat16));
  }
  if (M == 0) return out;
  launch_ok(eh_sage_csr_fwd(indptr.data_ptr<int64_t>(), nbr.numel() ? nbr.data_ptr<int32_t>() : nullptr,
                            cumw.numel() ? cumw.data_ptr<float>() : nullptr, N, nbr.numel(),
                            static_cast<int>(num_types), static_cast<uint32_t>(mask), x.data_ptr(),
                            x.scalar_type() == torch::kFloat32 ? 1 : 0, static_cast<int>(Dp), rp, M, W.data_ptr(),
                            static_cast<int>(Hp), static_cast<float>(nbr_scale), static_cast<float>(self_scale),
                            relu ? 1 : 0, out.data_ptr(), out_fp32 ? 1 : 0, cur_stream()),
            "sage_csr_fwd");
  return out;
}

}  // namespace

void register_sage_csr_ops(py::module& m) {
  m.def("sage_csr_fwd", &sage_csr_fwd, py::arg("indptr"), py::arg("nbr"), py::arg("cumw"), py::arg("num_types"),
        py::arg("mask"), py::arg("x"), py::arg("W"), py::arg("rows") = py::none(), py::arg("nbr_scale") = 1.0,
        py::arg("self_scale") = 0.0, py::arg("relu") = true, py::arg("out_fp32") = false,
        py::arg("out") = py::none());
  m.attr("sage_csr_hub_degree") = eh_sage_csr_hub_degree();
}
