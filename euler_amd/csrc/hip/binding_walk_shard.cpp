// torch binding of the sharded random walk's hop kernels (walk_shard.hip).  Host-only;
// operands go through binding_util.h (rules R1-R3 there); launches go to torch's current HIP
// stream, so a walk records into a hipGraph.
#include "hip/binding_util.h"
#include "hip/launchers.h"

using namespace euler_bind;

namespace {

// the packed request space: R a multiple of W that covers the rows, and every key
// (W * n tickets) * R below 2^62
void check_keys(int64_t n, int64_t num_rows, int64_t R, int64_t W, int64_t ticket0) {
  TORCH_CHECK(W >= 1 && W <= 63 && R >= 1 && R % W == 0 && R >= num_rows && num_rows >= 0,
              "walk: R must be a multiple of W (1..63) covering num_rows");
  TORCH_CHECK(ticket0 >= 0 && n >= 0, "walk: negative ticket");
  TORCH_CHECK(ticket0 + n <= (int64_t{1} << 62) / R, "walk: ticket * R does not fit 62 bits");
}

// out [n, cols] int32 gets column 0 = starts; returns the hop-0 request keys [n] int64
torch::Tensor walk_keys(torch::Tensor starts, torch::Tensor out, int64_t num_rows, int64_t R, int64_t W,
                        int64_t ticket0) {
  const Operands c("walk_keys", starts, "starts");
  c.i32(starts, "starts");
  c.i32(out, "out");
  const int64_t n = starts.numel();
  TORCH_CHECK(out.dim() == 2 && out.size(0) == n && out.size(1) >= 1, "out must be [n, walk_len + 1]");
  check_keys(n, num_rows, R, W, ticket0);
  const auto g = c.guard();
  auto keys = torch::empty({n}, starts.options().dtype(torch::kInt64));
  launch_ok(eh_walk_keys(starts.data_ptr<int32_t>(), n, num_rows, R, ticket0, out.size(1), out.data_ptr<int32_t>(),
                         keys.data_ptr<int64_t>(), cur_stream()),
            "walk_keys");
  return keys;
}

// the owner's draw per received request [m] -> next global row int32 [m] (-1: none)
torch::Tensor walk_step_owner(torch::Tensor req, int64_t R, int64_t W, torch::Tensor indptr, torch::Tensor nbr,
                              torch::Tensor cumw, int64_t local_rows, int64_t num_types, int64_t mask, int64_t hop,
                              torch::Tensor rng, int64_t stream_id) {
  const Operands c("walk_step_owner", req, "req");
  c.i64(req, "req");
  c.i64(indptr, "indptr");
  c.i32(nbr, "nbr");
  c.f32(cumw, "cumw");
  c.i64(rng, "rng_state");
  TORCH_CHECK(rng.numel() == 2, "rng_state must have 2 elements");
  TORCH_CHECK(num_types >= 1 && num_types <= 32, "num_types must be in [1, 32]");
  TORCH_CHECK(local_rows >= 0 && indptr.numel() == local_rows * num_types + 1, "indptr size mismatch: ",
              indptr.numel(), " vs ", local_rows * num_types + 1);
  TORCH_CHECK(nbr.numel() == cumw.numel(), "nbr/cumw size mismatch");
  TORCH_CHECK(W >= 1 && W <= 63 && R >= 1 && R % W == 0, "walk: R must be a multiple of W (1..63)");
  // every row a key can name is below R, so its local row is below R / W
  TORCH_CHECK(hop >= 0 && hop < 1024, "walk: at most 1024 hops");
  const auto g = c.guard();
  auto ans = torch::empty({req.numel()}, req.options().dtype(torch::kInt32));
  launch_ok(eh_walk_step_owner(req.data_ptr<int64_t>(), req.numel(), R, static_cast<int>(W), indptr.data_ptr<int64_t>(),
                               nbr.data_ptr<int32_t>(), cumw.data_ptr<float>(), local_rows, static_cast<int>(num_types),
                               static_cast<uint32_t>(mask), static_cast<int>(hop), rng.data_ptr<int64_t>(),
                               static_cast<uint64_t>(stream_id), ans.data_ptr<int32_t>(), cur_stream()),
            "walk_step_owner");
  return ans;
}

// column `col` of out from the returned answers; returns the next hop's request keys [n]
torch::Tensor walk_unroute(torch::Tensor back, torch::Tensor pos, torch::Tensor out, int64_t col,
                           int64_t default_row, int64_t num_rows, int64_t R, int64_t W, int64_t ticket0) {
  const Operands c("walk_unroute", back, "back");
  c.i32(back, "back");
  c.i64(pos, "pos");
  c.i32(out, "out");
  const int64_t n = pos.numel();
  TORCH_CHECK(out.dim() == 2 && out.size(0) == n, "out must be [n, walk_len + 1]");
  TORCH_CHECK(col >= 1 && col < out.size(1), "walk_unroute: column out of range");
  TORCH_CHECK(default_row >= INT32_MIN && default_row <= INT32_MAX, "default row must fit int32");
  check_keys(n, num_rows, R, W, ticket0);
  const auto g = c.guard();
  auto keys = torch::empty({n}, pos.options());
  launch_ok(eh_walk_unroute(back.data_ptr<int32_t>(), back.numel(), pos.data_ptr<int64_t>(), n,
                            static_cast<int32_t>(default_row), num_rows, R, ticket0, out.size(1), col,
                            out.data_ptr<int32_t>(), keys.data_ptr<int64_t>(), cur_stream()),
            "walk_unroute");
  return keys;
}

}  // namespace

void register_walk_shard_ops(py::module& m) {
  m.def("walk_keys", &walk_keys, py::arg("starts"), py::arg("out"), py::arg("num_rows"), py::arg("R"), py::arg("W"),
        py::arg("ticket0"));
  m.def("walk_step_owner", &walk_step_owner, py::arg("req"), py::arg("R"), py::arg("W"), py::arg("indptr"),
        py::arg("nbr"), py::arg("cumw"), py::arg("local_rows"), py::arg("num_types"), py::arg("mask"),
        py::arg("hop"), py::arg("rng"), py::arg("stream_id"));
  m.def("walk_unroute", &walk_unroute, py::arg("back"), py::arg("pos"), py::arg("out"), py::arg("col"),
        py::arg("default_row"), py::arg("num_rows"), py::arg("R"), py::arg("W"), py::arg("ticket0"));
}
