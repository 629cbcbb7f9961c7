#!/usr/bin/env python3
"""Sparse-feature embedding lookup of a batch of graph rows, forward + backward: the fused
node-row kernels (``mp_ops.node_bag`` over the HBM CSR: csrc/hip/node_embed.hip) against the
composed path the engine-path layer runs (``SparseEmbedding.forward`` on a device
SparseTensor of the same bags: argsort, bincount, cumsum, one ``spmm_csr``, and in the
backward a row gather, a scale and ``index_add_rows_``).

The fused pair is timed as a hipGraph replay (fixed shapes, no host read).  The composed
path reads the bag count on the host (``torch.bincount``), so it cannot be captured and is
timed eagerly; building its SparseTensor (the host work of the engine path) is not timed.
Times are device-event times per forward + backward, alternating the two paths.  Prints
one JSON line.

    python benchmarks/bench_node_bag.py [--n 16384] [--mean-bag 9] [--dim 16] [--vocab 1433]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    import torch

    from euler_amd.ops import graph_api as G
    from euler_amd.ops.mp_ops import node_bag
    from euler_amd.utils.layers import SparseEmbedding

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=16384, help="rows per lookup")
    ap.add_argument("--graph-rows", dest="graph_rows", type=int, default=100000)
    ap.add_argument("--mean-bag", dest="mean_bag", type=int, default=9)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=1433)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_node_bag measures on a GPU; none is available")
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(a.seed)
    # bag lengths 1 .. 2 * mean - 1 (mean = mean_bag), ids uniform in the vocabulary
    lens = torch.randint(1, 2 * a.mean_bag, (a.graph_rows,), generator=g)
    indptr = torch.zeros(a.graph_rows + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(lens, 0)
    values = torch.randint(0, a.vocab, (int(indptr[-1]),), generator=g)
    rows = torch.randint(0, a.graph_rows, (a.n,), generator=g)
    layer = SparseEmbedding(a.vocab, a.dim).to(dev)  # vocab + 1 rows: the last is the default id
    with torch.no_grad():
        layer.weight.normal_(0.0, 0.1)
    dout = torch.randn(a.n, a.dim, generator=g).to(dev)
    # the composed path's input: the SparseTensor get_sparse_feature would return for these rows
    ln = lens[rows]
    bag = torch.repeat_interleave(torch.arange(a.n), ln)
    off = torch.arange(int(ln.sum())) - torch.repeat_interleave(torch.cumsum(ln, 0) - ln, ln)
    sp = G.SparseTensor(torch.stack([bag, off], 1).to(dev), values[indptr[rows][bag] + off].to(dev),
                        torch.tensor([a.n, int(ln.max())]))
    csr = (indptr.to(dev), values.to(dev))
    rows_d = rows.to(dev)

    def fused():
        layer.weight.grad = None
        node_bag(layer.weight, rows_d, csr, "bag_sum").backward(dout)

    def composed():
        layer.weight.grad = None
        layer(sp).backward(dout)

    fused()
    g_fused = layer.weight.grad.clone()
    composed()
    err = float((g_fused - layer.weight.grad).abs().max() / layer.weight.grad.abs().max())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):
            fused()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3 / a.iters  # us per forward + backward

    for fn in (graph.replay, composed, fused):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    res = {"fused_graph_us": [], "fused_eager_us": [], "composed_eager_us": []}
    for _ in range(a.rounds):
        res["fused_graph_us"].append(timed(graph.replay))
        res["composed_eager_us"].append(timed(composed))
        res["fused_eager_us"].append(timed(fused))
    med = {k: round(sorted(v)[len(v) // 2], 2) for k, v in res.items()}
    nnz = int(ln.sum())
    out = {"metric": "sparse-feature embedding lookup, forward + backward, us (median of %d rounds x %d)"
                     % (a.rounds, a.iters), "n": a.n, "nnz": nnz, "dim": a.dim, "vocab": a.vocab,
           "atomic_segment_bytes": 4 * a.dim, **med,
           "spread_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in res.items()},
           "grad_max_rel_diff": err,
           "speedup_graph_vs_composed": round(med["composed_eager_us"] / max(med["fused_graph_us"], 1e-9), 2)}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
