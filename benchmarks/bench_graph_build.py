#!/usr/bin/env python3
"""Edge list -> HBM graph (``DeviceGraph.from_edges``): build time and peak memory of three
routes on one GPU, A/B/C in one process, alternating, ``--reps`` repetitions each.

* ``kernels`` -- ``DeviceGraph.from_edges`` as it stands (gfx950 kernels, hipcub radix sort);
* ``torch``   -- the CPU twin's torch composition on the same GPU tensors
  (``ops/graph_build_ops.py`` ``impl="torch"``: ``torch.sort`` on the packed key,
  ``unique_consecutive``, ``cumsum``), then the ``DeviceGraph`` constructor;
* ``host``    -- the route a user had before: ``numpy.lexsort`` of host copies of the arrays
  (the copies are not timed), then ``DeviceGraph.from_csr``.

Edges (int64 ids, ids are rows), fp32 weights and edge types are generated on the device in
random order.  Per route: build seconds (median and every repetition,
``torch.cuda.synchronize`` around the timed region), edges/s, and
``torch.cuda.max_memory_allocated`` during the build over what was allocated before it
(inputs), as peak bytes per input edge.  Prints one JSON line.

    python benchmarks/bench_graph_build.py [--nodes 10000000] [--edges 100000000] [--types 1]
        [--symmetric] [--duplicates keep|sum] [--routes kernels,torch,host] [--reps 3]
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
    import numpy as np
    import torch

    from euler_amd.graph.device_graph import DeviceGraph
    from euler_amd.ops import graph_build_ops as gb

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--edges", type=int, default=100_000_000)
    ap.add_argument("--types", type=int, default=1)
    ap.add_argument("--symmetric", action="store_true")
    ap.add_argument("--duplicates", choices=["keep", "sum"], default="keep")
    ap.add_argument("--routes", default="kernels,torch,host")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    routes = [r for r in args.routes.split(",") if r]
    for r in routes:
        if r not in ("kernels", "torch", "host"):
            ap.error(f"unknown route {r!r}")
    dev = torch.device(args.device)
    on_gpu = dev.type == "cuda"
    N, E, T = args.nodes, args.edges, args.types

    gen = torch.Generator(device=dev).manual_seed(args.seed)
    src = torch.randint(0, N, (E,), generator=gen, device=dev)
    dst = torch.randint(0, N, (E,), generator=gen, device=dev)
    w = torch.rand(E, generator=gen, device=dev) + 0.5
    et = torch.randint(0, T, (E,), generator=gen, device=dev, dtype=torch.int32) if T > 1 else None
    host = None
    if "host" in routes:
        host = (src.cpu().numpy(), dst.cpu().numpy(), w.cpu().numpy(), None if et is None else et.cpu().numpy())

    def sync():
        if on_gpu:
            torch.cuda.synchronize(dev)

    def kernels():
        return DeviceGraph.from_edges(src, dst, w, et, num_types=T, num_nodes=N, symmetric=args.symmetric,
                                      duplicates=args.duplicates, device=dev)

    def composed():
        indptr, nbr, cumw, _ = gb.build_csr(src, dst, w, et, None, num_rows=N, num_types=T,
                                            symmetric=args.symmetric, duplicates=args.duplicates, impl="torch")
        return DeviceGraph(indptr, nbr, cumw, T, device=dev)

    def host_route():
        s, d, ww, t = host
        if args.symmetric:
            s, d, ww = np.concatenate([s, d]), np.concatenate([d, s]), np.concatenate([ww, ww])
            t = None if t is None else np.concatenate([t, t])
        seg = s if t is None else s * T + t
        order = np.lexsort((d, seg))  # stable: equal (segment, dst) keep their input order
        seg, d, ww = seg[order], d[order], ww[order]
        if args.duplicates == "sum":
            head = np.ones(len(seg), bool)
            head[1:] = (seg[1:] != seg[:-1]) | (d[1:] != d[:-1])
            starts = np.flatnonzero(head)
            ww = np.add.reduceat(ww.astype(np.float64), starts).astype(np.float32)
            seg, d = seg[starts], d[starts]
        indptr = np.searchsorted(seg, np.arange(N * T + 1))
        return DeviceGraph.from_csr(indptr, d, ww, T, device=dev)

    if on_gpu:  # load the code objects of both device routes before anything is timed
        m = min(E, 1 << 16)
        ws, wd = src[:m] % min(N, 1 << 12), dst[:m] % min(N, 1 << 12)
        for impl in (None, "torch"):
            gb.build_csr(ws, wd, w[:m], None, None, num_rows=min(N, 1 << 12), symmetric=args.symmetric,
                         duplicates=args.duplicates, impl=impl)
        sync()

    fns = {"kernels": kernels, "torch": composed, "host": host_route}
    secs = {r: [] for r in routes}
    peaks = {r: [] for r in routes}
    errors = {}
    nnz = None
    for _ in range(args.reps):
        for r in routes:  # alternating
            if r in errors:
                continue
            sync()
            base = 0
            if on_gpu:
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
            t0 = time.perf_counter()
            try:
                g = fns[r]()
            except (RuntimeError, MemoryError) as e:  # e.g. out of memory: recorded, not hidden
                errors[r] = "%s: %s" % (type(e).__name__, str(e).split("\n")[0][:200])
                continue
            sync()
            secs[r].append(time.perf_counter() - t0)
            if on_gpu:
                peaks[r].append(torch.cuda.max_memory_allocated(dev) - base)
            nnz = g.num_edges if nnz is None else nnz
            assert g.num_edges == nnz, "the routes disagree on the number of CSR entries"
            del g

    out = {"metric": "edge list -> DeviceGraph build (seconds, lower is better)", "nodes": N, "edges": E, "types": T,
           "symmetric": bool(args.symmetric), "duplicates": args.duplicates, "nnz": nnz, "reps": args.reps,
           "device": torch.cuda.get_device_name(dev) if on_gpu else "cpu",
           "input_bytes_per_edge": 8 + 8 + 4 + (4 if et is not None else 0), "routes": {}}
    for r in routes:
        if not secs[r]:
            out["routes"][r] = {"error": errors.get(r, "not run")}
            continue
        med = statistics.median(secs[r])
        res = {"build_s": round(med, 4), "build_s_all": [round(x, 4) for x in secs[r]],
               "edges_per_s": round(E / med, 1)}
        if peaks[r]:
            res["peak_bytes_over_inputs"] = int(max(peaks[r]))
            res["peak_bytes_per_edge"] = round(max(peaks[r]) / max(E, 1), 2)
        if r in errors:
            res["error"] = errors[r]
        out["routes"][r] = res
    if on_gpu:
        out["total_hbm_gib"] = round(torch.cuda.get_device_properties(dev).total_memory / 2 ** 30, 1)
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
