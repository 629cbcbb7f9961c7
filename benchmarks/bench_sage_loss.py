#!/usr/bin/env python3
"""Cost of the softmax head: the fused GraphSAGE training step (``SageTrainer``) with
``loss="sigmoid"`` next to ``loss="softmax"`` on one GPU.

BASELINE config-2 shapes (``bench.py --num-nodes 10000000``): 10M-node synthetic graph, 128-d
bf16 features, int16 class-id labels over 64 classes, fanouts 25,10, conv / fc widths 256, 1024
roots per step, Adam.  Both trainers are built in one process on their own copy of the graph
(the same seed: the same graph, each with its own sample stream) and one shared feature table;
their steps are captured into hipGraphs as in ``bench.py`` and ``--reps`` timed repetitions of
``--steps`` steps each alternate (sigmoid, softmax, sigmoid, ...) after a warm-up,
``torch.cuda.synchronize`` around every timed region.

Prints one JSON line: every repetition's us per step for both losses, the medians, and their
ratio (softmax / sigmoid).  Only the head launch differs between the two steps; its share of
the step comes from a kernel table (``rocprofv3 --kernel-trace --stats`` over this script).

    python benchmarks/bench_sage_loss.py [--num-nodes 10000000] [--steps 2000] [--reps 5]
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


def main(argv=None):
    import torch

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--num-nodes", type=int, default=10_000_000)
    ap.add_argument("--avg-degree", type=float, default=10.0)
    ap.add_argument("--max-degree", type=int, default=1024)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--fanouts", default="25,10")
    ap.add_argument("--feature-dim", type=int, default=128)
    ap.add_argument("--hidden-dim", type=int, default=256)
    ap.add_argument("--label-dim", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps-per-graph", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sage_loss measures on a GPU; none is available")

    from euler_amd.dataset.synthetic import synthetic_features, synthetic_labels
    from euler_amd.graph.device_graph import DeviceGraph
    from euler_amd.models.sage_trainer import SageTrainer

    dev = torch.device("cuda", 0)
    fanouts = [int(x) for x in a.fanouts.split(",")]
    feats = synthetic_features(a.num_nodes, a.feature_dim, a.seed + 1, dev)
    labels = synthetic_labels(feats, a.label_dim)  # int16 class ids
    trainers = {}
    for loss in ("sigmoid", "softmax"):
        g = DeviceGraph.synthetic(a.num_nodes, a.avg_degree, a.max_degree, seed=a.seed, device=dev)
        g.manual_seed(a.seed * 7919)
        tr = SageTrainer(g, a.batch_size, fanouts, [a.hidden_dim] * (len(fanouts) + 1), a.label_dim, features=feats,
                         labels=labels, init_seed=a.seed, keep_samples=False, loss=loss)
        spg = max(1, a.steps_per_graph)
        tr.capture(steps=spg, extra_sizes=(a.warmup % spg, a.steps % spg))
        tr.replay_steps(a.warmup)
        trainers[loss] = tr
    torch.cuda.synchronize()

    us = {k: [] for k in trainers}
    for _ in range(a.reps):
        for loss, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.replay_steps(a.steps)
            torch.cuda.synchronize()
            us[loss].append((time.perf_counter() - t0) * 1e6 / a.steps)
    for tr in trainers.values():
        tr._check_fuse()
    med = {k: statistics.median(v) for k, v in us.items()}
    out = {"metric": "us per captured SageTrainer step, loss=softmax against loss=sigmoid",
           "us_per_step": {k: [round(x, 3) for x in v] for k, v in us.items()},
           "median_us": {k: round(v, 3) for k, v in med.items()},
           "ratio_softmax_over_sigmoid": round(med["softmax"] / med["sigmoid"], 4),
           "loss_last": {k: round(float(tr.loss.item()), 4) for k, tr in trainers.items()},
           "metric_last": {k: {tr.metric_name: round(tr.metric(), 4)} for k, tr in trainers.items()},
           "config": {"num_nodes": a.num_nodes, "fanouts": fanouts, "batch_size": a.batch_size,
                      "feature_dim": a.feature_dim, "hidden_dim": a.hidden_dim, "label_dim": a.label_dim,
                      "labels": "int16 class ids", "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
                      "steps_per_graph": a.steps_per_graph}}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
