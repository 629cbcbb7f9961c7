#!/usr/bin/env python3
"""kNN retrieval (``euler_amd.tools.knn``): index build and search on one GPU.

Seeded clustered synthetic embeddings (``--n`` rows around 1024 Gaussian centres), queries
drawn the same way.  Prints one JSON line: build seconds, search ms (median of 3 after a
warm-up search, ``torch.cuda.synchronize`` around the timed region), queries/s, peak bytes
allocated during a search over what was allocated before it, and for ``ivfflat`` recall@k
against the flat index of the same implementation.

``--impl kernel`` is the tool as it stands (fused distance + top-k kernels on GPU tensors);
``--impl torch`` asks for the torch composition (``use_kernels=False`` where the tool knows
the argument) and touches nothing but ``build_index`` / ``search``, so with ``--tool-file``
pointing at another checkout's ``euler_amd/tools/knn.py`` the same script times that one.

``--dtype bf16`` compares the two table dtypes of this tree instead: the embeddings are rounded
to bf16 so that both routes see the same numbers, one index of ``--index`` is built per dtype
(the IVF ones share their centroids), and the fp32 and bf16 searches are timed alternating in one
process, ``--reps`` repetitions of ``--iters`` searches each.  It prints one JSON line with, per
route, the median and the spread of the time per search, the peak bytes allocated during a
search, the bytes the index holds, and how far the two results agree.

``--index ivfflat --ivf-schedule query|list`` picks the IVF search schedule of the plain run.
``--ivf-schedule both`` compares the two schedules instead: one IVF index of ``--dtype`` (here the
table's dtype) is built and searched through both schedules alternating in one process, ``--reps``
repetitions of a warm-up search and ``--iters`` timed searches each, for every query count in
``--nqs``.  It prints one JSON line per query count with, per schedule, the median and the spread
of the time per search, and the time of its stages (probe selection, inversion, scan, merge; each
synchronised, summed over the query chunks), and how far the two results agree.

    python benchmarks/bench_knn.py [--n 1000000] [--d 128] [--nq 1024] [--k 10]
        [--index flat|ivfflat] [--impl kernel|torch] [--tool-file PATH]
        [--dtype fp32|bf16] [--reps 5] [--iters 10] [--ivf-schedule query|list|both] [--nqs 1024,16384]
"""
import argparse
import importlib.util
import inspect
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _clustered(n, d, centres, gen, dev, torch):
    out = torch.empty(n, d, device=dev)
    for s in range(0, n, 1 << 20):  # in slabs: no second [n, d] temporary
        m = min(1 << 20, n - s)
        which = torch.randint(0, centres.shape[0], (m,), generator=gen, device=dev)
        out[s:s + m] = centres[which] + torch.randn(m, d, generator=gen, device=dev)
    return out


def _compare_dtypes(a, knn, x, q, torch, np):
    """fp32 and bf16 indexes over the same bf16-representable values, searched alternating"""
    xb = x.to(torch.bfloat16)
    q = q.to(torch.bfloat16).float()
    x = None  # the fp32 route's table is made from the rounded values below
    routes = {}
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        table = xb.float() if name == "fp32" else xb
        if a.index == "flat":
            idx = knn.FlatIndex(a.d, device="cuda", dtype=dt)
        else:
            idx = knn.IVFFlatIndex(a.d, int(4 * a.n ** 0.5), nprobe=10, device="cuda", dtype=dt)
            if routes:
                idx.cent, idx.ncent = routes["fp32"]["index"].cent, routes["fp32"]["index"].ncent
            else:
                g = torch.Generator(device="cpu").manual_seed(1234)
                keep = torch.randperm(a.n, generator=g)[:256 * idx.ncent].sort().values.cuda()
                idx.train(table[keep] if keep.numel() < a.n else table)
        idx.add(table)
        torch.cuda.synchronize()
        held = sum(t.numel() * t.element_size() for t in (idx.xb, getattr(idx, "xs", None)) if t is not None)
        routes[name] = {"index": idx, "build_s": time.perf_counter() - t0, "index_bytes": held,
                        "build_peak_bytes": torch.cuda.max_memory_allocated() - before, "ms": []}
        del table
    for r in routes.values():
        r["out"] = r["index"].search(q, a.k)  # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        r["index"].search(q, a.k)
        torch.cuda.synchronize()
        r["peak"] = torch.cuda.max_memory_allocated() - before
    for _ in range(a.reps):
        for r in routes.values():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                r["index"].search(q, a.k)
            torch.cuda.synchronize()
            r["ms"].append((time.perf_counter() - t0) * 1e3 / a.iters)
    (D0, I0), (D1, I1) = routes["fp32"]["out"], routes["bf16"]["out"]
    fin = np.isfinite(D0) & np.isfinite(D1)
    res = {"bench": "knn_dtypes", "index": a.index, "n": a.n, "d": a.d, "nq": a.nq, "k": a.k, "reps": a.reps,
           "iters": a.iters, "same_rows": round(float((I0 == I1).mean()), 6),
           "max_abs_dist_diff": float(np.abs(D0[fin] - D1[fin]).max()) if fin.any() else 0.0,
           "device": torch.cuda.get_device_name(0)}
    for name, r in routes.items():
        ms = statistics.median(r["ms"])
        res[name] = {"search_ms": round(ms, 3), "search_ms_min": round(min(r["ms"]), 3),
                     "search_ms_max": round(max(r["ms"]), 3), "search_ms_all": [round(t, 3) for t in r["ms"]],
                     "queries_per_s": round(a.nq / (ms * 1e-3), 1), "search_peak_bytes": int(r["peak"]),
                     "index_bytes": int(r["index_bytes"]), "build_s": round(r["build_s"], 4),
                     "build_peak_bytes": int(r["build_peak_bytes"])}
    res["bf16_over_fp32_time"] = round(res["bf16"]["search_ms"] / res["fp32"]["search_ms"], 4)
    print(json.dumps(res))
    return res


def _stages(idx, q, k, torch):
    """ms per stage of one search of an IVF index, as IVFFlatIndex.search composes it"""
    from euler_amd.ops import knn_ops
    from euler_amd.ops._native import hip

    t = {"probe": 0.0, "invert": 0.0, "scan": 0.0, "merge": 0.0}

    def timed(name, f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        t[name] += (time.perf_counter() - t0) * 1e3
        return out

    bf = idx.dtype == torch.bfloat16
    q = q.to(torch.bfloat16).contiguous() if bf else q.float().contiguous()
    nprobe, ncent = min(idx.nprobe, idx.ncent), idx.list_ptr.numel() - 1
    chunk = 65536 if idx.schedule == "list" else 1024
    for s in range(0, q.shape[0], chunk):
        qq = q[s:s + chunk]
        probe = timed("probe", lambda: knn_ops.flat_topk(qq.float(), idx.cent, nprobe)[1])
        if idx.schedule == "list":
            table = timed("invert", lambda: hip().knn_grouped.invert(probe, ncent, k))
            pd, pr = table[4], table[5]
            timed("scan", lambda: hip().knn_grouped.scan(qq, idx.xs, idx.xns, idx.list_ptr, idx.row_of, *table))
        else:
            scan = hip().knn_bf16.ivf_scan if bf else hip().knn_ivf_scan
            pd, pr = timed("scan", lambda: scan(qq, idx.xs, idx.xns, idx.list_ptr, idx.row_of, probe, k))
        timed("merge", lambda: hip().knn_merge(pd, pr, (qq.float() * qq.float()).sum(1)))
    return {n: round(v, 3) for n, v in t.items()}


def _compare_schedules(a, knn, x, torch, np, centres, gen):
    """one IVF index searched through the "query" and the "list" schedule, alternating"""
    import copy

    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    t0 = time.perf_counter()
    base = knn.build_index(x.to(dt) if dt == torch.bfloat16 else x, "ivfflat", device="cuda",
                           max_points_per_centroid=256, dtype=dt)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    routes = {}
    for name in ("query", "list"):
        routes[name] = copy.copy(base)  # the same tensors, another schedule
        routes[name].schedule = name
    out = []
    for nq in [int(v) for v in a.nqs.split(",")]:
        q = _clustered(nq, a.d, centres, gen, x.device, torch)
        ms = {name: [] for name in routes}
        got = {}
        for _ in range(a.reps):
            for name, idx in routes.items():
                got[name] = idx.search(q, a.k)  # warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    idx.search(q, a.k)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
        res = {"bench": "knn_ivf_schedules", "dtype": a.dtype, "n": a.n, "d": a.d, "nq": nq, "k": a.k,
               "ncent": base.ncent, "nprobe": base.nprobe, "reps": a.reps, "iters": a.iters,
               "build_s": round(build_s, 3),
               "same_rows": round(float((got["query"][1] == got["list"][1]).mean()), 6),
               "max_abs_dist_diff": float(np.nan_to_num(np.abs(got["query"][0] - got["list"][0]), posinf=0.0).max()),
               "device": torch.cuda.get_device_name(0)}
        for name, idx in routes.items():
            med = statistics.median(ms[name])
            res[name] = {"search_ms": round(med, 3), "search_ms_min": round(min(ms[name]), 3),
                         "search_ms_max": round(max(ms[name]), 3), "search_ms_all": [round(v, 3) for v in ms[name]],
                         "queries_per_s": round(nq / (med * 1e-3), 1), "stages_ms": _stages(idx, q, a.k, torch)}
        res["list_over_query_time"] = round(res["list"]["search_ms"] / res["query"]["search_ms"], 4)
        print(json.dumps(res), flush=True)
        out.append(res)
    return out


def main(argv=None):
    import numpy as np
    import torch

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--index", choices=["flat", "ivfflat"], default="flat")
    ap.add_argument("--impl", choices=["kernel", "torch"], default="kernel")
    ap.add_argument("--tool-file", dest="tool_file", default=None,
                    help="load build_index from this knn.py instead of euler_amd.tools.knn")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32",
                    help="bf16: time the fp32 and the bf16 table of this tree against each other")
    ap.add_argument("--reps", type=int, default=5, help="--dtype bf16: repetitions per route, alternating")
    ap.add_argument("--iters", type=int, default=10, help="--dtype bf16: searches per repetition")
    ap.add_argument("--ivf-schedule", dest="ivf_schedule", choices=["query", "list", "both"], default="query",
                    help="IVF search schedule; both: time the two against each other on a --dtype table")
    ap.add_argument("--nqs", default=None, help="--ivf-schedule both: comma-separated query counts (default: --nq)")
    a = ap.parse_args(argv)
    a.nqs = a.nqs or str(a.nq)
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn measures on a GPU; none is available")
    if a.tool_file:
        spec = importlib.util.spec_from_file_location("knn_under_test", a.tool_file)
        knn = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(knn)
    else:
        from euler_amd.tools import knn
    has_switch = "use_kernels" in inspect.signature(knn.build_index).parameters
    if a.impl == "kernel" and not has_switch:
        raise SystemExit("this knn.py has no fused kernels (--impl torch times it)")

    if a.ivf_schedule != "query" and "schedule" not in inspect.signature(knn.build_index).parameters:
        raise SystemExit("this knn.py has no IVF schedules (--ivf-schedule query times it)")

    def build(kind):
        kw = {}
        if has_switch:
            kw["use_kernels"] = None if a.impl == "kernel" else False
        if a.ivf_schedule != "query":
            kw["schedule"] = a.ivf_schedule
        return knn.build_index(x, kind, device="cuda", **kw)

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    centres = torch.randn(1024, a.d, generator=gen, device=dev) * 4.0
    x = _clustered(a.n, a.d, centres, gen, dev, torch)
    if a.ivf_schedule == "both":
        if a.tool_file or a.impl != "kernel" or a.index != "ivfflat":
            raise SystemExit("--ivf-schedule both compares the IVF kernels of this tree (--index ivfflat, --impl kernel)")
        return _compare_schedules(a, knn, x, torch, np, centres, gen)
    q = _clustered(a.nq, a.d, centres, gen, dev, torch)
    if a.dtype == "bf16":
        if a.tool_file or a.impl != "kernel":
            raise SystemExit("--dtype bf16 compares the kernels of this tree (no --tool-file, --impl kernel)")
        return _compare_dtypes(a, knn, x, q, torch, np)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = build(a.index)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0

    index.search(q, a.k)  # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D, I = index.search(q, a.k)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    peak = torch.cuda.max_memory_allocated() - before
    ms = statistics.median(times) * 1e3
    res = {"bench": "knn", "index": a.index, "impl": a.impl, "tool_file": bool(a.tool_file), "ivf_schedule": a.ivf_schedule,
           "n": a.n, "d": a.d,
           "nq": a.nq, "k": a.k, "build_s": round(build_s, 4), "search_ms": round(ms, 3),
           "search_ms_all": [round(t * 1e3, 3) for t in times], "queries_per_s": round(a.nq / (ms * 1e-3), 1),
           "search_peak_bytes": int(peak), "device": torch.cuda.get_device_name(0)}
    if a.index == "ivfflat":
        del index
        _, J = build("flat").search(q, a.k)
        res["recall_at_k"] = round(float(np.mean([len(set(r) & set(t)) / float(a.k) for r, t in zip(I, J)])), 4)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
