#!/usr/bin/env python3
"""TransH / TransD / TransR training throughput under ``EdgeEstimator(device_graph=True)``: the
fused projected score kernels (csrc/hip/kg_proj.hip kgp_fwd / kgp_bwd; ``--models transr``:
csrc/hip/kg_transr.hip kgr_fwd / kgr_bwd) against the torch composition of the same model
(``EULER_AMD_KG_PROJ_FUSED=0``), alternating in one process.

The run is ``benchmarks/bench_gcn.py --model M --dataset fb15k`` (the README's TransE estimator
row: batch 512, 5 negatives, dim 32) with the device path only and a longer window: the rate
is the estimator's own over the last log interval (a quarter of ``--steps``), which ends in a
device synchronise.  Prints one JSON line: per model and route the rates of every repetition,
their median, and the median time per step.

    python benchmarks/bench_kg_proj.py [--models transh,transd] [--routes fused,torch] [--reps 3] [--dim 32]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmarks import bench_gcn  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="transh,transd")
    ap.add_argument("--routes", default="fused,torch", help="fused: kg_proj.hip / kg_transr.hip; torch: EULER_AMD_KG_PROJ_FUSED=0")
    ap.add_argument("--reps", type=int, default=3, help="repetitions of every (model, route), routes alternating")
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--batch-size", dest="batch_size", type=int, default=512)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--num-negs", dest="num_negs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_kg_proj measures on a GPU; none is available")
    work = tempfile.mkdtemp(prefix="bench_kg_proj_")
    out = {"bench": "kg_proj", "dataset": "fb15k", "batch_size": a.batch_size, "dim": a.dim, "num_negs": a.num_negs,
           "steps": a.steps, "window_steps": max(a.steps // 4, 1), "reps": a.reps, "models": {}}
    for model in a.models.split(","):
        rates = {r: [] for r in a.routes.split(",")}
        for rep in range(a.reps + 1):  # repetition 0 warms up both routes (code objects, the dataset files)
            for route in rates:
                os.environ["EULER_AMD_KG_PROJ_FUSED"] = "1" if route == "fused" else "0"
                args = argparse.Namespace(
                    model=model, dataset="fb15k", batch_size=a.batch_size, steps=a.steps, engine_steps=0, lr=0.01,
                    device="cuda", seed=a.seed, hidden_dim=32, scale=1.0, loss="sigmoid",
                    common="--dim,%d,--num_negs,%d" % (a.dim, a.num_negs), extra="")
                res = bench_gcn.run("device", args, os.path.join(work, "%s_%s_%d" % (model, route, rep)))
                print("[bench_kg_proj] %s %s rep %d: %s" % (model, route, rep, res), file=sys.stderr, flush=True)
                if rep > 0:
                    rates[route].append(res["samples_per_sec"])
        out["models"][model] = {
            r: {"triples_per_sec": v, "median_triples_per_sec": round(statistics.median(v), 1),
                "median_us_per_step": round(a.batch_size / statistics.median(v) * 1e6, 2)}
            for r, v in rates.items() if v}  # --reps 0: one untimed run per route (for a kernel trace)
        if "fused" in out["models"][model] and "torch" in out["models"][model]:
            m = out["models"][model]
            m["fused_over_torch"] = round(m["fused"]["median_triples_per_sec"] / m["torch"]["median_triples_per_sec"], 3)
    os.environ.pop("EULER_AMD_KG_PROJ_FUSED", None)
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
