#!/usr/bin/env python3
"""Graph-classification inference throughput under ``GraphEstimator(device_graph=True)`` on the
MUTAG-shaped synthetic set (188 graphs of 10-27 nodes): ``infer_logits`` of ``--requests`` graph
indices (the set's graphs in a seeded random order, repeated), three routes alternating in one
process:

* ``packed``         the forward-only pack kernel (csrc/hip/graph_cls_infer.hip), default packing;
* ``one_per_block``  the same kernel with one graph per block (``EULER_AMD_GRAPH_INFER_PACK=1``);
* ``generic``        ``GraphTrainer.infer_logits`` on the GPU (the model's own modules over
                     ``DeviceFullFlow`` blocks, chunks of ``--batch-size`` graphs).

A repetition times whole calls (host packing and upload included) with the host clock over a
window of at least ``--window`` seconds that ends in a device synchronise; repetition 0 warms up
every route.  Prints one JSON line: per model and route the graphs/s of every repetition, their
median and the median time per call.

    python benchmarks/bench_graph_infer.py [--models gin,graphgcn] [--routes packed,one_per_block,generic]
    python benchmarks/bench_graph_infer.py --margins   # CPU: fp32 against float64 forward (the tests' bound)
"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def trainer(model, device, work, batch, fused=True, seed=5):
    """the estimator's device trainer of ``model`` with seeded random weights"""
    import torch

    from euler_amd.tools import runner

    train_eps = model == "gin_eps"
    os.environ["EULER_AMD_GRAPH_FUSED"] = "1" if fused else "0"
    a = runner.parse_args(["--model_dir", os.path.join(work, model + device), "--batch_size", str(batch),
                           "--total_step", "1", "--device", device, "--seed", "1", "--device_graph"],
                          model="gin" if train_eps else model)
    torch.manual_seed(0)
    _, est = runner.build(a)
    if train_eps:
        for conv in est.model.gnn.convs:
            del conv._buffers["eps"]
            conv.eps = torch.nn.Parameter(torch.tensor([0.25]))
    tr = est._device_graph_trainer(est.get_train_from_input(est.train_input_fn(), est.params))
    os.environ.pop("EULER_AMD_GRAPH_FUSED", None)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in tr.flat.params:
            p.copy_((torch.randn(p.shape, generator=gen) * 0.3).to(p.device))
    return tr


def margins(work):
    """max|a - b| / max|b| of the CPU fp32 forward against the float64 one (outputs rounded to
    fp32) on the request lists of tests/test_graph_cls_infer.py"""
    import torch

    rel = lambda x, y: float((x.double() - y.double()).abs().max() / y.double().abs().max())  # noqa: E731
    out = {"measure": "max|fp32 - fp64| / max|fp64|, generic CPU GraphTrainer", "cases": {}}
    for model in ("gin", "gin_eps", "graphgcn"):
        tr = trainer(model, "cpu", work, 16)
        for case, idx in (("single", [5]), ("packs", list(range(14)) + [3])):
            idx = torch.tensor(idx)
            emb, (_, logits, _) = tr.infer_embed(idx), tr.infer_logits(idx)
            m32, m64 = tr.model, copy.deepcopy(tr.model).double()
            tr.model, tr.gnn = m64, m64.gnn
            emb64, (_, logits64, _) = tr.infer_embed(idx), tr.infer_logits(idx)
            tr.model, tr.gnn = m32, m32.gnn
            out["cases"]["%s/%s" % (model, case)] = {"emb": rel(emb, emb64), "logits": rel(logits, logits64)}
    for k in ("emb", "logits"):
        worst = max(c[k] for c in out["cases"].values())
        out[k] = {"max_fp32_vs_fp64": worst, "tolerance_8x_floor_1e-6": max(8 * worst, 1e-6)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="gin,graphgcn")
    ap.add_argument("--routes", default="packed,one_per_block,generic")
    ap.add_argument("--reps", type=int, default=3, help="timed repetitions of every (model, route), routes alternating")
    ap.add_argument("--requests", type=int, default=4096, help="graph indices per infer_logits call")
    ap.add_argument("--batch-size", dest="batch_size", type=int, default=64, help="the trainers' B (generic chunk)")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds of calls per repetition")
    ap.add_argument("--margins", action="store_true")
    a = ap.parse_args(argv)
    import torch

    work = tempfile.mkdtemp(prefix="bench_graph_infer_")
    if a.margins:
        out = margins(work)
        print(json.dumps(out), flush=True)
        return out
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph_infer measures on a GPU; none is available")
    out = {"bench": "graph_infer", "dataset": "mutag (synthetic)", "requests": a.requests, "batch_size": a.batch_size,
           "reps": a.reps, "window_s": a.window, "models": {}}
    for model in a.models.split(","):
        fused = trainer(model, "cuda", work, a.batch_size)
        assert type(fused).__name__ == "GraphClsTrainer", type(fused)
        routes = {r: (trainer(model, "cuda", work, a.batch_size, fused=False) if r == "generic" else fused)
                  for r in a.routes.split(",")}
        G = int(fused.onehot.shape[0])
        idx = torch.randint(0, G, (a.requests,), generator=torch.Generator().manual_seed(3))
        rates, packs = {r: [] for r in routes}, {}
        for rep in range(a.reps + 1):  # repetition 0 warms up every route
            for route, tr in routes.items():
                os.environ.pop("EULER_AMD_GRAPH_INFER_PACK", None)
                if route == "one_per_block":
                    os.environ["EULER_AMD_GRAPH_INFER_PACK"] = "1"
                tr.infer_logits(idx)
                torch.cuda.synchronize()
                if tr is fused:
                    packs[route] = int(tr.plan.infer_packs)
                calls, t0 = 0, time.perf_counter()
                while True:
                    tr.infer_logits(idx)
                    calls += 1
                    if calls >= 3 and time.perf_counter() - t0 >= (a.window if rep else 0.0):
                        break
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print("[bench_graph_infer] %s %s rep %d: %d calls in %.4f s" % (model, route, rep, calls, dt),
                      file=sys.stderr, flush=True)
                if rep:
                    rates[route].append(a.requests * calls / dt)
        os.environ.pop("EULER_AMD_GRAPH_INFER_PACK", None)
        m = {r: {"graphs_per_sec": [round(x, 1) for x in v], "median_graphs_per_sec": round(statistics.median(v), 1),
                 "median_us_per_call": round(a.requests / statistics.median(v) * 1e6, 2)} for r, v in rates.items() if v}
        for r, n in packs.items():
            if r in m:
                m[r]["packs"] = n
        m["rows_per_pack"] = int(fused.plan.infer_rows)
        m["lds_bytes"] = int(fused.plan.infer_lds_bytes)
        out["models"][model] = m
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
