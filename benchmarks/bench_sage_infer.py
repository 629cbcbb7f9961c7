#!/usr/bin/env python3
"""Layer-wise full-graph GraphSAGE inference (``euler_amd.models.sage_infer``) on one GPU.

The headline model of ``bench.py`` (128-d bf16 features, conv widths 256, fanouts 25,10) on
``DeviceGraph.synthetic`` (default 10M nodes; ``--num-nodes 100000000`` for the headline
graph).  Every conv layer is run over ALL rows, ``fused`` (csrc/hip/sage_csr.hip, one launch)
and ``composed`` (CSR SpMM + concat + MFMA GEMM on a prepared normalised CSR, whose build
time is reported apart) alternating in one process, ``--reps`` timed repetitions each after
one warm-up, ``torch.cuda.synchronize`` around every timed region; medians are reported.

Prints one JSON line: ms per layer and nodes/s (rows over the sum of the conv layers) for
both implementations, the end-to-end time of ``LayerwiseSageInference.embed()`` over every
row with either implementation (conv layers in row chunks + fc; the composed one builds its
CSR per chunk and layer there), the sampled ``SageTrainer.infer_embed`` rate on a
``--sampled-ids`` subset (the rate ON THAT SUBSET, in batches of ``--sampled-batch`` ids),
bytes per layer from shapes ((E + M) Dp bytes gathered + M Hp 2 written) and the achieved
TB/s of the fused layer against the 6.3 TB/s achievable HBM rate.

    python benchmarks/bench_sage_infer.py [--num-nodes 10000000] [--reps 3]

``--frontier-ids 1024,65536,1048576`` measures frontier inference instead (``mode="frontier"``,
nothing of the above runs): for every id count, on a random id subset, the frontier call and
the all-rows call from a cold cache (``invalidate()`` first: the cost after a training step)
alternate in one process, ``--reps`` repetitions each after one warm-up.  Per id count the JSON
line holds the medians and every repetition, the set sizes, the time of building the sets (mark
+ rank + list) against the time of the layers on a prepared plan, and the bytes gathered by
shape ((edges of the targets + targets) Dp bytes per layer).  The counts are a sweep: the
``crossover`` entry names the last count at which the frontier call wins and the first at which
it does not, with the largest set's share of the graph at both — the figure behind
``frontier_max_fraction`` (which the benchmark itself sets to 1: no fallback hides a time).
"""
import argparse
import json
import os
import statistics
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
    ap.add_argument("--feature-dim", type=int, default=128)
    ap.add_argument("--hidden-dim", type=int, default=256)
    ap.add_argument("--label-dim", type=int, default=64)
    ap.add_argument("--fanouts", default="25,10")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sampled-ids", type=int, default=65536)
    ap.add_argument("--sampled-batch", type=int, default=8192)
    ap.add_argument("--skip-composed", action="store_true", help="time the fused layers only (profiling runs)")
    ap.add_argument("--skip-sampled", action="store_true")
    ap.add_argument("--frontier-ids", default="", help="comma-separated id counts: measure frontier inference "
                    "against the cold all-rows call at each (module docstring)")
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sage_infer measures on a GPU; none is available")
    if a.reps < 3:
        raise SystemExit("--reps must be at least 3")

    from euler_amd.dataset.synthetic import synthetic_features, synthetic_labels
    from euler_amd.graph.device_graph import DeviceGraph
    from euler_amd.models.sage_trainer import SageTrainer
    from euler_amd.ops.sage_csr_ops import composed_csr, expected_scales, sage_csr_layer

    dev = torch.device("cuda", 0)
    fanouts = [int(f) for f in a.fanouts.split(",")]
    L, N = len(fanouts), a.num_nodes
    g = DeviceGraph.synthetic(N, a.avg_degree, a.max_degree, seed=a.seed, device=dev)
    feats = synthetic_features(N, a.feature_dim, a.seed + 1, dev, dtype=torch.bfloat16)
    labels = synthetic_labels(feats, a.label_dim)
    tr = SageTrainer(g, 1024, fanouts, [a.hidden_dim] * (L + 1), a.label_dim, features=feats, labels=labels,
                     init_seed=a.seed, keep_samples=False)
    lw = tr.layerwise()
    E = g.num_edges

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    if a.frontier_ids:
        res = frontier_bench(a, g, tr, lw, timed)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))
        return res

    prep = None
    prep_s = None
    if not a.skip_composed:
        # no self loops: nbr_scale = 1, self_scale = 0 for every hop, one CSR serves all layers
        prep_s, prep = timed(lambda: composed_csr(g, tr.masks[0], None, 1.0, 0.0))

    layers = []
    x = tr.features
    for k in range(L):
        hop = L - 1 - k
        ns, ss = expected_scales(fanouts[hop], tr.include_self)
        W = lw.conv_weights[k]
        kw = dict(mask=tr.masks[hop], nbr_scale=ns, self_scale=ss, relu=True, out_dtype=torch.bfloat16)
        runs = {"fused": lambda: sage_csr_layer(g, x, W, impl="fused", **kw)}
        if prep is not None:
            runs["composed"] = lambda: sage_csr_layer(g, x, W, impl="composed", prepared=prep, **kw)
        times = {name: [] for name in runs}
        out = None
        for rep in range(a.reps + 1):  # rep 0 warms up; the implementations alternate
            for name, fn in runs.items():
                t, y = timed(fn)
                if rep:
                    times[name].append(t)
                if name == "fused":
                    out = y
                del y
        Dp, Hp = x.shape[1], W.shape[0]
        nbytes = (E + N) * Dp * x.element_size() + N * Hp * 2
        rec = {"layer": k, "Dp": Dp, "Hp": Hp, "bytes": nbytes}
        for name, ts in times.items():
            ms = statistics.median(ts) * 1e3
            rec[name + "_ms"] = round(ms, 3)
            rec[name + "_ms_all"] = [round(t * 1e3, 3) for t in ts]
            rec[name + "_tb_s"] = round(nbytes / (ms * 1e-3) / 1e12, 3)
            rec[name + "_hbm_frac"] = round(nbytes / (ms * 1e-3) / 1e12 / HBM_TBS, 3)
        layers.append(rec)
        x = out
    del x, out, prep
    torch.cuda.empty_cache()

    res = {"bench": "sage_infer", "num_nodes": N, "num_edges": E, "fanouts": fanouts, "feature_dim": a.feature_dim,
           "hidden_dim": a.hidden_dim, "reps": a.reps, "hbm_tb_s": HBM_TBS, "layers": layers,
           "composed_csr_build_s": None if prep_s is None else round(prep_s, 3)}
    for name in ("fused", "composed"):
        if name + "_ms" in layers[0]:
            total = sum(r[name + "_ms"] for r in layers) * 1e-3
            res[name + "_nodes_per_s"] = round(N / total, 1)
    if "composed_nodes_per_s" in res:
        res["fused_over_composed"] = round(res["fused_nodes_per_s"] / res["composed_nodes_per_s"], 3)

    # the whole model through LayerwiseSageInference (row chunks, fc), as infer() runs it; the
    # composed implementation builds its normalised CSR per chunk and layer there
    from euler_amd.models.sage_infer import LayerwiseSageInference

    for name in ("fused", "composed"):
        if name == "composed" and a.skip_composed:
            continue
        m = lw if name == "fused" else LayerwiseSageInference(
            g, tr.features, lw.conv_weights, fanouts, tr.masks, tr.include_self, fc=lw.fc, out_fc=lw.out_fc,
            embed_dim=tr.E, logits_dim=tr.C, impl="composed")
        ts = []
        for rep in range(a.reps + 1):
            m.invalidate()
            t, emb = timed(lambda: m.embed())
            del emb
            if rep:
                ts.append(t)
        t = statistics.median(ts)
        res[name + "_end_to_end_embed_s"] = round(t, 4)
        res[name + "_end_to_end_nodes_per_s"] = round(N / t, 1)
        del m
        torch.cuda.empty_cache()

    if not a.skip_sampled:
        n_ids = min(a.sampled_ids, N)
        ids = torch.randperm(N, generator=torch.Generator().manual_seed(a.seed))[:n_ids].numpy()
        tr.infer_embed(ids[: a.sampled_batch])  # warm-up
        t, _ = timed(lambda: [tr.infer_embed(ids[s:s + a.sampled_batch]) for s in range(0, n_ids, a.sampled_batch)])
        res["sampled_ids"] = n_ids
        res["sampled_batch"] = a.sampled_batch
        res["sampled_nodes_per_s_on_subset"] = round(n_ids / t, 1)
        res["fused_over_sampled"] = round(res["fused_nodes_per_s"] / res["sampled_nodes_per_s_on_subset"], 1)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    return res


def masked_edges(g, rows, mask):
    """edges of the valid rows over the masked (row, type) segments, from indptr"""
    import torch

    r = rows.long()
    r = r[(r >= 0) & (r < g.num_rows)]
    n = 0
    for t in range(g.num_types):
        if (mask >> t) & 1:
            n += int((g.indptr[r * g.num_types + t + 1] - g.indptr[r * g.num_types + t]).sum())
    return n


def frontier_bench(a, g, tr, lw, timed):
    import torch

    from euler_amd.models.sage_infer import FrontierPlan

    N, L = g.num_rows, lw.L
    if L < 2:
        raise SystemExit("--frontier-ids needs at least two hops: a 1-hop model has no all-rows pass to avoid")
    counts = [int(c) for c in a.frontier_ids.split(",")]
    lw.frontier_max_fraction = 1.0  # measure the frontier path at every count: the sweep finds the crossover
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(a.seed))
    widths = [tr.features.shape[1]] + [w.shape[0] for w in lw.conv_weights]
    esz = tr.features.element_size()
    points = []
    for n_ids in counts:
        rows = perm[: min(n_ids, N)].to(g.device)
        runs = {
            "frontier": lambda: lw.embed(rows, mode="frontier"),
            "all_rows_cold": lambda: (lw.invalidate(), lw.embed(rows))[1],
            "sets": lambda: FrontierPlan(lw, rows),
        }
        times = {name: [] for name in runs}
        times["layers"] = []
        for rep in range(a.reps + 1):  # rep 0 warms up; the calls alternate
            for name, fn in runs.items():
                t, out = timed(fn)
                if rep:
                    times[name].append(t)
                if name == "sets":
                    t, y = timed(lambda: lw.embed(rows, mode="frontier", plan=out))
                    if rep:
                        times["layers"].append(t)
                    del y
                del out
        plan = FrontierPlan(lw, rows)
        # targets of layer k: the list of I_{k+1}; of the last layer: the request
        targets = [s.rows for s in plan.sets] + [rows]
        gathered = [(masked_edges(g, targets[k], lw.masks[L - 1 - k]) + int(targets[k].numel())) * widths[k] * esz
                    for k in range(L)]
        all_rows = [(g.num_edges + N) * widths[k] * esz for k in range(L - 1)] + [gathered[-1]]
        rec = {"ids": int(rows.numel()), "set_sizes": plan.sizes,
               "largest_set_fraction": round(max(plan.sizes) / N, 4),
               "gathered_bytes": gathered, "all_rows_gathered_bytes": all_rows,
               "gather_work_ratio": round(sum(gathered) / sum(all_rows), 4)}
        for name, ts in times.items():
            rec[name + "_ms"] = round(statistics.median(ts) * 1e3, 3)
            rec[name + "_ms_all"] = [round(t * 1e3, 3) for t in ts]
        rec["frontier_over_all_rows_cold"] = round(rec["frontier_ms"] / rec["all_rows_cold_ms"], 4)
        points.append(rec)
        del plan, targets
        torch.cuda.empty_cache()
    wins = [p for p in points if p["frontier_ms"] < p["all_rows_cold_ms"]]
    loses = [p for p in points if p["frontier_ms"] >= p["all_rows_cold_ms"]]
    cross = {"last_win": None, "first_loss": None}
    if wins:
        w = max(wins, key=lambda p: p["ids"])
        cross["last_win"] = {"ids": w["ids"], "largest_set_fraction": w["largest_set_fraction"]}
    if loses:
        lo = min(loses, key=lambda p: p["ids"])
        cross["first_loss"] = {"ids": lo["ids"], "largest_set_fraction": lo["largest_set_fraction"]}
    return {"bench": "sage_infer_frontier", "num_nodes": N, "num_edges": g.num_edges, "fanouts": list(lw.fanouts),
            "feature_dim": a.feature_dim, "hidden_dim": a.hidden_dim, "reps": a.reps, "points": points,
            "crossover": cross}


if __name__ == "__main__":
    main()
