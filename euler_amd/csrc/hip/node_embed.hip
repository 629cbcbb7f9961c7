// Node rows -> embedding rows, straight from the HBM-resident sparse feature CSR
// (graph/device_graph.py DeviceGraph.sparse) or the node id column: the input layer of the
// encoder models (utils/encoders.py ShallowEncoder) on the device path.
//
//   mode 0 bag_sum : out[i] = sum_j table[map(values[j])], j over the CSR segment of rows[i]
//   mode 1 bag_mean: the same sum, then one multiply by 1.0f / count
//   mode 2 id      : out[i] = table[map(v)], v = node_ids[rows[i]] (rows[i] when node_ids is null)
//
// An empty bag, a negative row and a row past the table are "a bag of the default id"
// V - 1 (the engine's default_values = max_id + 1 and its default node), mapped like any
// id.  map(v) = v when 0 <= v < V, else V - 1; with hash = 1 it is the multiplicative hash
// of utils/layers.py HashEmbedding (the multiply in uint64: it wraps like torch's int64).
//
// Forward: fixed shape, no host read, one launch.  The tables are small (they sit in L2),
// so the loop is latency-bound: a group of D / 4 lanes serves one bag with 16-byte table
// loads (D = 16: 4 lanes per bag, 16 bags per wave), four ids in flight per lane; the sum
// is taken in CSR order in fp32.  Widths that are no power-of-two multiple of 4 take one
// lane per (row, column).
//
// Backward: one lane per (row, column) adds dOut[i, col + d] (times 1 / count for the mean)
// to dTable[map(id), d] for every id of the bag with a no-return fp32 atomic: a
// wave-instruction adds whole contiguous row segments of D floats.  An addend of exactly
// 0.0f is skipped: the -1 padding of a capacity-padded hop set maps every padded row to
// row V - 1, and their (zero) gradients would otherwise all queue on one address.  The
// atomics arrive in any order, so dTable is not bit-reproducible from run to run.
#include "hip/common.h"
#include "hip/launchers.h"

namespace euler_hip {
namespace {

constexpr int kBagSum = 0, kBagMean = 1, kIdMode = 2;
constexpr int64_t kMaxBlocks = 2048;  // capped grid + grid-stride loop

struct NodeBagArgs {
  const int64_t* rows;
  int64_t n;
  const int64_t* indptr;  // [num_rows + 1] (bag modes)
  const int64_t* values;  // [nnz]
  int64_t nnz;
  const int64_t* node_ids;  // [num_rows] or null (id mode)
  int64_t num_rows;         // rows of the CSR / the id column; < 0: unbounded (ids = rows)
  int64_t V;
  int D;
  int64_t ld;
  int64_t col;
  int mode;
  int hash;
};

__device__ __forceinline__ int64_t map_id(int64_t v, int64_t V, int hash) {
  if (hash) {
    const uint64_t h = (static_cast<uint64_t>(v) * 0x9E3779B1ull) & 0x7FFFFFFFull;
    return static_cast<int64_t>(h % static_cast<uint64_t>(V));
  }
  return (v >= 0 && v < V) ? v : V - 1;
}

// the ids of output row i: [a, b) in `values` (bag modes, b > a) or the single id `one`
// (b == a): the id of the row in id mode, the default id otherwise
__device__ __forceinline__ void bag_of(const NodeBagArgs& p, int64_t i, int64_t& a, int64_t& b, int64_t& one) {
  const int64_t r = p.rows[i];
  a = b = 0;
  one = p.V - 1;
  const bool in = r >= 0 && (p.num_rows < 0 || r < p.num_rows);
  if (!in) return;
  if (p.mode == kIdMode) {
    one = p.node_ids ? p.node_ids[r] : r;
    return;
  }
  const int64_t s = p.indptr[r], e = p.indptr[r + 1];
  if (s >= 0 && e <= p.nnz && e > s) {
    a = s;
    b = e;
  }
}

// LP = D / 4 lanes per bag (a power of two <= 64), each lane 4 columns
__global__ __launch_bounds__(256) void node_bag_fwd_vec(NodeBagArgs p, const float* __restrict__ table,
                                                        float* __restrict__ out, int LP, int vec_store) {
  const int sub = threadIdx.x & (LP - 1);
  const int64_t group = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / LP;
  const int64_t ngroups = static_cast<int64_t>(gridDim.x) * blockDim.x / LP;
  const float4_t* __restrict__ t4 = reinterpret_cast<const float4_t*>(table);
  const int64_t D4 = p.D / 4;
  for (int64_t i = group; i < p.n; i += ngroups) {
    int64_t a, b, one;
    bag_of(p, i, a, b, one);
    float4_t acc;
    if (b == a) {
      acc = t4[map_id(one, p.V, p.hash) * D4 + sub];
    } else {
      acc = float4_t{0.f, 0.f, 0.f, 0.f};
      int64_t j = a;
      for (; j + 4 <= b; j += 4) {  // four rows in flight, added in CSR order
        const int64_t r0 = map_id(p.values[j], p.V, p.hash), r1 = map_id(p.values[j + 1], p.V, p.hash);
        const int64_t r2 = map_id(p.values[j + 2], p.V, p.hash), r3 = map_id(p.values[j + 3], p.V, p.hash);
        const float4_t v0 = t4[r0 * D4 + sub], v1 = t4[r1 * D4 + sub];
        const float4_t v2 = t4[r2 * D4 + sub], v3 = t4[r3 * D4 + sub];
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
      }
      for (; j < b; ++j) acc += t4[map_id(p.values[j], p.V, p.hash) * D4 + sub];
      if (p.mode == kBagMean) acc *= 1.0f / static_cast<float>(b - a);
    }
    float* o = out + i * p.ld + p.col + 4 * sub;
    if (vec_store) {
      *reinterpret_cast<float4_t*>(o) = acc;
    } else {
      o[0] = acc[0];
      o[1] = acc[1];
      o[2] = acc[2];
      o[3] = acc[3];
    }
  }
}

// any D: one lane per (row, column)
__global__ __launch_bounds__(256) void node_bag_fwd_col(NodeBagArgs p, const float* __restrict__ table,
                                                        float* __restrict__ out) {
  const int64_t D = p.D;
  grid_stride(p.n * D, [&](int64_t t) {
    const int64_t i = t / D;
    const int64_t d = t - i * D;
    int64_t a, b, one;
    bag_of(p, i, a, b, one);
    float acc;
    if (b == a) {
      acc = table[map_id(one, p.V, p.hash) * D + d];
    } else {
      acc = 0.f;
      int64_t j = a;
      for (; j + 4 <= b; j += 4) {
        const float v0 = table[map_id(p.values[j], p.V, p.hash) * D + d];
        const float v1 = table[map_id(p.values[j + 1], p.V, p.hash) * D + d];
        const float v2 = table[map_id(p.values[j + 2], p.V, p.hash) * D + d];
        const float v3 = table[map_id(p.values[j + 3], p.V, p.hash) * D + d];
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
      }
      for (; j < b; ++j) acc += table[map_id(p.values[j], p.V, p.hash) * D + d];
      if (p.mode == kBagMean) acc *= 1.0f / static_cast<float>(b - a);
    }
    out[i * p.ld + p.col + d] = acc;
  });
}

__global__ __launch_bounds__(256) void node_bag_bwd_col(NodeBagArgs p, const float* __restrict__ dout,
                                                        float* __restrict__ dtable) {
  const int64_t D = p.D;
  grid_stride(p.n * D, [&](int64_t t) {
    const int64_t i = t / D;
    const int64_t d = t - i * D;
    float g = dout[i * p.ld + p.col + d];
    if (g == 0.0f) return;  // padded rows: nothing to add (and no pile-up on row V - 1)
    int64_t a, b, one;
    bag_of(p, i, a, b, one);
    if (b == a) {
      atomicAdd(dtable + map_id(one, p.V, p.hash) * D + d, g);
      return;
    }
    if (p.mode == kBagMean) g *= 1.0f / static_cast<float>(b - a);
    for (int64_t j = a; j < b; ++j) atomicAdd(dtable + map_id(p.values[j], p.V, p.hash) * D + d, g);
  });
}

dim3 capped_grid(int64_t items) {
  const int64_t b = ceil_div(items, 256);
  return dim3(static_cast<uint32_t>(b < 1 ? 1 : (b < kMaxBlocks ? b : kMaxBlocks)));
}

bool fill_args(NodeBagArgs& p, const int64_t* rows, int64_t n, const int64_t* indptr, const int64_t* values,
               int64_t nnz, const int64_t* node_ids, int64_t num_rows, int64_t V, int D, int64_t ld, int64_t col,
               int mode, int hash) {
  if (rows == nullptr || n < 0 || V < 1 || D < 1 || col < 0 || col + D > ld) return false;
  if (mode != kBagSum && mode != kBagMean && mode != kIdMode) return false;
  if (mode != kIdMode && (indptr == nullptr || num_rows < 0 || nnz < 0 || (nnz > 0 && values == nullptr)))
    return false;
  if (mode == kIdMode && node_ids != nullptr && num_rows < 0) return false;
  p.rows = rows;
  p.n = n;
  p.indptr = indptr;
  p.values = values;
  p.nnz = nnz;
  p.node_ids = node_ids;
  p.num_rows = num_rows;
  p.V = V;
  p.D = D;
  p.ld = ld;
  p.col = col;
  p.mode = mode;
  p.hash = hash ? 1 : 0;
  return true;
}

}  // namespace
}  // namespace euler_hip

using namespace euler_hip;

extern "C" hipError_t eh_node_bag_fwd(const int64_t* rows, int64_t n, const int64_t* indptr, const int64_t* values,
                                      int64_t nnz, const int64_t* node_ids, int64_t num_rows, const float* table,
                                      int64_t V, int D, float* out, int64_t ld, int64_t col, int mode, int hash,
                                      hipStream_t s) {
  if (n == 0) return hipSuccess;  // nothing to launch (an empty tensor may have no storage)
  NodeBagArgs p;
  if (!fill_args(p, rows, n, indptr, values, nnz, node_ids, num_rows, V, D, ld, col, mode, hash) || !table || !out)
    return hipErrorInvalidValue;
  const int lp = D / 4;
  const bool vec = D % 4 == 0 && lp <= 64 && (lp & (lp - 1)) == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0;
  if (vec) {
    const int vec_store = (ld % 4 == 0 && col % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(node_bag_fwd_vec, capped_grid(n * lp), dim3(256), 0, s, p, table, out, lp, vec_store);
  } else {
    hipLaunchKernelGGL(node_bag_fwd_col, capped_grid(n * D), dim3(256), 0, s, p, table, out);
  }
  return hipGetLastError();
}

extern "C" hipError_t eh_node_bag_bwd(const int64_t* rows, int64_t n, const int64_t* indptr, const int64_t* values,
                                      int64_t nnz, const int64_t* node_ids, int64_t num_rows, const float* dout,
                                      int64_t ld, int64_t col, int64_t V, int D, float* dtable, int mode, int hash,
                                      hipStream_t s) {
  if (n == 0) return hipSuccess;
  NodeBagArgs p;
  if (!fill_args(p, rows, n, indptr, values, nnz, node_ids, num_rows, V, D, ld, col, mode, hash) || !dout || !dtable)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(node_bag_bwd_col, capped_grid(n * D), dim3(256), 0, s, p, dout, dtable);
  return hipGetLastError();
}
