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

    python benchmarks/bench_knn.py [--n 1000000] [--d 128] [--nq 1024] [--k 10]
        [--index flat|ivfflat] [--impl kernel|torch] [--tool-file PATH]
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
    a = ap.parse_args(argv)
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

    def build(kind):
        if has_switch:
            return knn.build_index(x, kind, device="cuda", use_kernels=None if a.impl == "kernel" else False)
        return knn.build_index(x, kind, device="cuda")

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    centres = torch.randn(1024, a.d, generator=gen, device=dev) * 4.0
    x = _clustered(a.n, a.d, centres, gen, dev, torch)
    q = _clustered(a.nq, a.d, centres, gen, dev, torch)

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
    res = {"bench": "knn", "index": a.index, "impl": a.impl, "tool_file": bool(a.tool_file), "n": a.n, "d": a.d,
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
