#!/usr/bin/env python3
"""Layer-wise full-graph inference of the fused GCN family (``euler_amd.models.gcn_infer``) on
one GPU.

The PPI-schema fused-GCN model (50-d features padded to 64, two conv layers of width 64, fc and
label width 121) on ``DeviceGraph.synthetic`` (default 10M nodes).  Three routes alternate in one
process, ``--reps`` timed repetitions each after one warm-up, ``torch.cuda.synchronize`` around
every timed region; medians and every repetition are reported:

  (i)   ``LayerwiseGcnInference`` over all nodes, fused (csrc/hip/gcn_csr.hip), cold cache;
  (ii)  every conv layer over all rows as ``impl="composed"`` on a prepared normalised CSR
        (``spmm_csr`` + ``gemm``; the CSR's build time is reported apart), next to the fused
        layer on the same operands: the per-layer A/B;
  (iii) ``GcnTrainer.infer_logits`` over a ``--block-ids`` subset in batches of ``--block-batch``
        ids: an exact block per batch, what users have without layer-wise inference (the rate
        ON THAT SUBSET).  The batches are first tried in a child process: if an exact-capacity
        block does not fit the HBM the JSON carries ``block_subset_error`` and the route is
        left out.

Prints one JSON line: ms per layer for both implementations, bytes per layer from shapes
((E + M) Dp bytes gathered + M Hp 2 written) and the achieved TB/s, nodes/s of (i) and (iii)
and their ratio.

    python benchmarks/bench_gcn_infer.py [--num-nodes 10000000] [--reps 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def main(argv=None):
    import torch

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--num-nodes", type=int, default=10_000_000)
    ap.add_argument("--avg-degree", type=float, default=10.0)
    ap.add_argument("--max-degree", type=int, default=2048)
    ap.add_argument("--feature-dim", type=int, default=50)
    ap.add_argument("--hidden-dim", type=int, default=64)
    ap.add_argument("--label-dim", type=int, default=121)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block-ids", type=int, default=65536)
    ap.add_argument("--block-batch", type=int, default=512)
    ap.add_argument("--skip-composed", action="store_true", help="time the fused route only (profiling runs)")
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--probe-block", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_gcn_infer measures on a GPU; none is available")
    if a.reps < 3:
        raise SystemExit("--reps must be at least 3")

    # Route (iii) builds an exact-capacity block per batch; on a heavy-tailed graph it may not fit
    # the HBM, and a failed batch leaves this process's allocator full.  So the batches are tried
    # in a child process first: if it fails, the error is reported and the route is left out.
    block_error = None
    if not a.skip_block and not a.probe_block:
        args = list(sys.argv[1:] if argv is None else argv) + ["--probe-block"]
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
        if r.returncode != 0:
            last = (r.stderr.strip().splitlines() or ["no message"])[-1]
            block_error = {"kind": "out of memory" if "OutOfMemoryError" in last else "error",
                           "block_batch": a.block_batch, "message": last.split(". See documentation")[0][:400]}
            a.skip_block = True

    from euler_amd import models as Z
    from euler_amd.dataset.synthetic import synthetic_features, synthetic_labels
    from euler_amd.estimator.device_trainers import materialize_without_engine
    from euler_amd.graph.device_graph import DeviceGraph
    from euler_amd.models.gcn_trainer import GcnTrainer
    from euler_amd.ops.gcn_csr_ops import gcn_composed_csr, gcn_csr_layer

    dev = torch.device("cuda", 0)
    N, L = a.num_nodes, a.layers
    g = DeviceGraph.synthetic(N, a.avg_degree, a.max_degree, seed=a.seed, device=dev)
    g.features = synthetic_features(N, a.feature_dim, a.seed + 1, dev, dtype=torch.bfloat16)
    g.labels = torch.nn.functional.one_hot(synthetic_labels(g.features, a.label_dim).long() % a.label_dim,
                                           a.label_dim).to(torch.bfloat16)  # multi-label [N, C] rows
    torch.manual_seed(a.seed)
    model = Z.SupervisedGNN("gcn", "full", [a.hidden_dim] * L + [a.label_dim], None, [["0"]] * L, ["f"],
                            [a.feature_dim], "l", a.label_dim, add_self_loops=True)
    materialize_without_engine(model)  # the lazy layers take their shapes on the host
    model = model.to(dev)
    tr = GcnTrainer(model, g, a.block_batch, [g._mask(None)] * L)
    if a.probe_block:
        ids = torch.randperm(N, generator=torch.Generator().manual_seed(a.seed))[:min(a.block_ids, N)].numpy()
        for s in range(0, (len(ids) // a.block_batch) * a.block_batch, a.block_batch):
            tr.infer_logits(ids[s:s + a.block_batch])  # a block's size follows its batch: every batch is tried
        torch.cuda.synchronize()
        return None
    lw = tr.layerwise()
    E = g.num_edges

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def stats(ts, prefix, rec):
        rec[prefix + "_ms"] = round(statistics.median(ts) * 1e3, 3)
        rec[prefix + "_ms_all"] = [round(t * 1e3, 3) for t in ts]

    res = {"bench": "gcn_infer", "num_nodes": N, "num_edges": E, "layers": L, "feature_dim": a.feature_dim,
           "hidden_dim": a.hidden_dim, "label_dim": a.label_dim, "reps": a.reps, "hbm_tb_s": HBM_TBS,
           "device": torch.cuda.get_device_name(0)}
    if block_error is not None:
        res["block_subset_error"] = block_error

    runs = {"layerwise_all": lambda: (lw.invalidate(), lw.logits())[1]}
    if not a.skip_block:
        n_ids = min(a.block_ids, N)
        ids = torch.randperm(N, generator=torch.Generator().manual_seed(a.seed))[:n_ids].numpy()
        n_block = (n_ids // a.block_batch) * a.block_batch  # whole batches: one flow shape

        def block_subset():  # every batch's block is dropped before the next one is built
            for s in range(0, n_block, a.block_batch):
                tr.infer_logits(ids[s:s + a.block_batch])

        runs["block_subset"] = block_subset
    times = {name: [] for name in runs}
    for rep in range(a.reps + 1):  # rep 0 warms up; the routes alternate
        for name, fn in runs.items():
            t, out = timed(fn)
            del out
            if rep:
                times[name].append(t)
    stats(times["layerwise_all"], "layerwise_all", res)
    res["layerwise_nodes_per_s"] = round(N / (res["layerwise_all_ms"] * 1e-3), 1)
    if "block_subset" in times:
        stats(times["block_subset"], "block_subset", res)
        res.update({"block_ids": n_block, "block_batch": a.block_batch,
                    "block_nodes_per_s_on_subset": round(n_block / (res["block_subset_ms"] * 1e-3), 1)})
        res["layerwise_over_block"] = round(res["layerwise_nodes_per_s"] / res["block_nodes_per_s_on_subset"], 1)
    torch.cuda.empty_cache()

    # (ii) the per-layer A/B on the same operands
    layers, x = [], lw.features
    for k in range(L):
        aa, bb = lw.scales[k]
        kw = dict(mask=lw.masks[L - 1 - k], tgt_scale=aa, src_scale=bb if k == 0 else None,
                  out_scale=lw.scales[k + 1][1] if k < L - 1 else None, self_loop=True)
        W = lw.conv_weights[k]
        runs = {"fused": lambda: gcn_csr_layer(g, x, W, impl="fused", **kw)}
        rec = {"layer": k, "Dp": x.shape[1], "Hp": W.shape[0],
               "bytes": (E + N) * x.shape[1] * x.element_size() + N * W.shape[0] * 2}
        if not a.skip_composed:
            t, prep = timed(lambda: gcn_composed_csr(g, kw["mask"], None, aa, kw["src_scale"], True))
            rec["composed_csr_build_s"] = round(t, 3)
            runs["composed"] = lambda: gcn_csr_layer(g, x, W, impl="composed", prepared=prep, **kw)
        times = {name: [] for name in runs}
        out = None
        for rep in range(a.reps + 1):
            for name, fn in runs.items():
                t, y = timed(fn)
                if rep:
                    times[name].append(t)
                if name == "fused":
                    out = y
                del y
        for name, ts in times.items():
            stats(ts, name, rec)
            rec[name + "_tb_s"] = round(rec["bytes"] / (rec[name + "_ms"] * 1e-3) / 1e12, 3)
            rec[name + "_hbm_frac"] = round(rec[name + "_tb_s"] / HBM_TBS, 3)
        if "composed_ms" in rec:
            rec["fused_over_composed"] = round(rec["composed_ms"] / rec["fused_ms"], 3)
        layers.append(rec)
        x, prep = out, None
        torch.cuda.empty_cache()
    res["conv_layers"] = layers
    if not a.skip_composed:
        res["fused_over_composed"] = round(sum(r["composed_ms"] for r in layers) / sum(r["fused_ms"] for r in layers), 3)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
