#!/usr/bin/env python3
"""Train on a graph given as an edge list -- no graph engine, no Euler JSON, no converter.

Writes a small planted-community graph as an ``.npz`` (arrays ``src``, ``dst``, ``weight``,
``node_ids``, ``features``, ``labels``), then trains ``SupervisedGraphSage`` and ``DeepWalk``
on it through ``NodeEstimator(device_graph=True)``: ``edge_list_factory`` hands the estimator
a ``DeviceGraph.from_edges`` graph built on the training device, and evaluate / infer read an
id file and map its ids with ``graph.rows_of``.

    python examples/train_from_edge_list.py [--device cuda|cpu] [--nodes 4000] [--steps 200]
"""
import argparse
import logging
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from euler_amd import models as Z  # noqa: E402
from euler_amd.estimator import NodeEstimator  # noqa: E402
from euler_amd.graph import edge_list_factory  # noqa: E402


def planted_communities(n, classes, feature_dim, degree, seed=0):
    """edge-list arrays of a planted-community graph: raw int64 ids with gaps, ``degree`` out
    edges per node (90 % inside the node's class), features around the class mean, one-hot
    labels; edges in random order"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, classes, n)
    ids = np.arange(n, dtype=np.int64) * 7 + 1000
    members = [np.flatnonzero(cls == c) for c in range(classes)]
    src = np.repeat(np.arange(n), degree)
    own = np.array([members[c][rng.integers(0, len(members[c]))] for c in cls[src]])
    dst = np.where(rng.random(n * degree) < 0.9, own, rng.integers(0, n, n * degree))
    p = rng.permutation(n * degree)
    means = rng.standard_normal((classes, feature_dim)).astype(np.float32)
    return {"src": ids[src[p]], "dst": ids[dst[p]],
            "weight": (0.5 + rng.random(n * degree)).astype(np.float32), "node_ids": ids,
            "features": (means[cls] + 0.5 * rng.standard_normal((n, feature_dim))).astype(np.float32),
            "labels": np.eye(classes, dtype=np.float32)[cls]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--nodes", type=int, default=4000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--feature_dim", type=int, default=16)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--work_dir", default=None)
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    work = args.work_dir or tempfile.mkdtemp(prefix="edge_list_")
    os.makedirs(work, exist_ok=True)

    arrays = planted_communities(args.nodes, args.classes, args.feature_dim, degree=8)
    path = os.path.join(work, "graph.npz")
    np.savez(path, **arrays)
    id_file = os.path.join(work, "eval_ids.txt")
    with open(id_file, "w") as f:
        f.write("\n".join(str(int(i)) for i in arrays["node_ids"][::5]) + "\n")

    def params(name, **kw):
        p = {"model_dir": os.path.join(work, name), "infer_dir": os.path.join(work, name, "infer"),
             "batch_size": args.batch_size, "total_step": args.steps, "optimizer": "adam", "learning_rate": 0.01,
             "log_steps": max(1, args.steps // 5), "train_node_type": -1, "device": args.device, "seed": 1,
             "id_file": id_file, "device_graph": True}
        p.update(kw)
        return p

    # supervised GraphSAGE on the raw ids: the factory compacts them, rows_of maps the id file
    torch.manual_seed(0)
    sage = Z.SupervisedGraphSage([32, 32, args.classes], [5, 5], [[0], [0]], "feature", args.feature_dim, "label",
                                 args.classes, max_id=int(arrays["node_ids"].max()))
    est = NodeEstimator(sage, params("graphsage", device_graph_factory=edge_list_factory(path, symmetric=True)))
    print("SupervisedGraphSage train:", est.train())
    print("SupervisedGraphSage evaluate:", est.evaluate())
    ids, emb = est.infer()
    print("SupervisedGraphSage infer: %d embeddings of width %d" % (emb.shape[0], emb.shape[1]))

    # DeepWalk keeps one embedding row per id, so its ids are the rows 0 .. n - 1
    rows = {k: np.searchsorted(arrays["node_ids"], arrays[k]) for k in ("src", "dst")}
    rows["weight"] = arrays["weight"]
    torch.manual_seed(0)
    walk = Z.DeepWalk(-1, -1, args.nodes - 1, 32, walk_len=3, num_negs=5)
    est = NodeEstimator(walk, params("deepwalk", learning_rate=0.05, device_graph_factory=edge_list_factory(
        rows, num_nodes=args.nodes, symmetric=True)))
    print("DeepWalk train:", est.train())
    print("outputs under", work)


if __name__ == "__main__":
    main()
