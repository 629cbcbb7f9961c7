#!/usr/bin/env python3
"""Knowledge-graph link prediction (``euler_amd.models.kg_eval``) at the FB15k shape on one GPU.

14,951 entities, 1,345 relations, D = 100 and 59,071 test triples (the size of FB15k's test
split).  The tables are seeded random rows and the test triples are uniform draws; the dataset
itself is not needed.  The filter is synthetic as well: every test query gets a list of known
answers whose length is drawn from a heavy-tailed distribution (``1 + floor(Pareto(1.2))``,
capped at 2,000: most queries have one or two known answers, a few have hundreds, as in a real
split; ``--filter-alpha`` changes the tail).

For each score kind (``l1``: TransE, ``l2``: TransE(l1=False), ``dot``: DistMult) it times

* ``rank_triples`` on both sides, filtered, and on the tail side, raw: the fused rank kernel;
* for ``l1`` / ``l2`` the composition the kernel replaces, ``dataset.synthetic.tail_ranks``
  (tail side, raw; a [chunk, N] ``torch.cdist`` matrix per chunk), imported unchanged.

``--models transh,transd,transr`` measures the projected models instead: ``rank_triples`` on both
sides, filtered, on the fused route (``kg_rank_ops.rank_counts_proj``: the projection inside the
scan kernel) and on the per-relation loop it replaces (``EULER_AMD_KG_RANK_PROJ_FUSED=0``),
alternating in one process, ``--repeat`` passes each after a warm-up pass of each route.  The test
relations are drawn with Zipf frequencies (``p(r) ~ 1 / (r + 1)``): a few relations hold thousands
of queries, most a handful, as in FB15k's test split.  TransR runs at ``--dim`` and at
``--transr-dim`` (entity and relation dimension alike).  Reports medians and ranges, the share of
equal ranks between the routes and the number of single-relation query tiles with their mean fill.

Each figure is the median of ``--repeat`` passes after a warm-up pass, with
``torch.cuda.synchronize`` around the timed region; peak bytes are what a pass allocates over
what was allocated before it.  Prints one JSON line.

    python benchmarks/bench_kg_rank.py [--entities 14951] [--relations 1345] [--dim 100]
        [--triples 59071] [--batch 4096] [--repeat 3] [--kinds l1 l2 dot]
        [--models transh,transd,transr] [--transr-dim 32]
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


def _timed(fn, repeat, torch):
    fn()  # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    times, out = [], None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    peak = torch.cuda.max_memory_allocated() - before
    return statistics.median(times) * 1e3, [round(t * 1e3, 3) for t in times], int(peak), out


def _ab(model, triples, known, batch, repeat, torch, kg_eval):
    """fused route and per-relation loop, alternating; ms per pass"""
    def run(fused):
        os.environ["EULER_AMD_KG_RANK_PROJ_FUSED"] = "1" if fused else "0"
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = kg_eval.rank_triples(model, *triples, known=known, batch=batch)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out
        finally:
            os.environ.pop("EULER_AMD_KG_RANK_PROJ_FUSED", None)

    ranks = {f: run(f)[1] for f in (True, False)}  # warm-up of both routes
    ms = {True: [], False: []}
    for _ in range(repeat):
        for f in (True, False):
            ms[f].append(run(f)[0])
    same = torch.cat([ranks[True][s] == ranks[False][s] for s in ("head", "tail")]).double().mean()
    diff = max(int((ranks[True][s] - ranks[False][s]).abs().max()) for s in ("head", "tail"))

    def stats(v):
        return {"ms": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                "ms_all": [round(t, 3) for t in v]}

    return {"fused": stats(ms[True]), "per_relation_loop": stats(ms[False]),
            "speedup": round(statistics.median(ms[False]) / statistics.median(ms[True]), 2),
            "ranks_equal_fraction": round(float(same), 6), "max_rank_difference": diff}


def _bench_models(a, torch, res, dev, gen):
    from euler_amd import models as Z
    from euler_amd.models import kg_eval

    n, N, R = a.triples, a.entities, a.relations
    src = torch.randint(0, N, (n,), generator=gen, device=dev)
    dst = torch.randint(0, N, (n,), generator=gen, device=dev)
    freq = 1.0 / torch.arange(1, R + 1, device=dev, dtype=torch.float64)
    rel = torch.multinomial(freq, n, replacement=True, generator=gen)
    known = kg_eval.KnownTriples(src, rel, dst, N, device=dev)
    tiles = fill = 0
    for s0 in range(0, n, a.batch):  # the single-relation query tiles of every batch
        cnt = torch.unique(rel[s0:s0 + a.batch], return_counts=True)[1]
        tiles += int(((cnt + 63) // 64).sum())
        fill += int(cnt.sum())
    res.update(relation_frequencies="zipf", distinct_test_relations=int(torch.unique(rel).numel()),
               query_tiles_per_side=tiles, mean_tile_fill=round(fill / tiles / 64, 4), models={})
    for name in a.models.split(","):
        for dim in ([a.dim, a.transr_dim] if name == "transr" else [a.dim]):
            torch.manual_seed(a.seed)
            cls = {"transh": Z.TransH, "transd": Z.TransD, "transr": Z.TransR}[name]
            model = cls(-1, [0], N - 1, R - 1, dim, dim).to(dev)
            res["models"]["%s_d%d" % (name, dim)] = _ab(model, (src, rel, dst), known, a.batch, a.repeat, torch,
                                                         kg_eval)


def main(argv=None):
    import torch

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--entities", type=int, default=14951)
    ap.add_argument("--relations", type=int, default=1345)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--triples", type=int, default=59071)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--kinds", nargs="+", default=["l1", "l2", "dot"], choices=["l1", "l2", "dot"])
    ap.add_argument("--filter-alpha", dest="alpha", type=float, default=1.2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--models", default="", help="transh,transd,transr: the projected models, fused route vs loop")
    ap.add_argument("--transr-dim", dest="transr_dim", type=int, default=32)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_kg_rank measures on a GPU; none is available")
    from euler_amd import models as Z
    from euler_amd.dataset.synthetic import tail_ranks
    from euler_amd.models import kg_eval

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    if a.models:
        res = {"bench": "kg_rank_proj", "entities": a.entities, "relations": a.relations, "dim": a.dim,
               "triples": a.triples, "batch": a.batch, "repeat": a.repeat, "sides": "head + tail, filtered",
               "device": torch.cuda.get_device_name(0)}
        _bench_models(a, torch, res, dev, gen)
        print(json.dumps(res))
        return res
    n, N, R = a.triples, a.entities, a.relations
    src = torch.randint(0, N, (n,), generator=gen, device=dev)
    rel = torch.randint(0, R, (n,), generator=gen, device=dev)
    dst = torch.randint(0, N, (n,), generator=gen, device=dev)
    # known triples: the test triples plus, per test query and side, len - 1 other answers
    u = torch.rand(n, generator=gen, device=dev).clamp_min(1e-9)
    lens = (u ** (-1.0 / a.alpha)).floor().clamp(1, 2000).long()
    extra = lens - 1
    who = torch.repeat_interleave(torch.arange(n, device=dev), extra)
    other = torch.randint(0, N, (int(extra.sum()),), generator=gen, device=dev)
    known = kg_eval.KnownTriples(torch.cat([src, src[who], other]), torch.cat([rel, rel[who], rel[who]]),
                                 torch.cat([dst, other, dst[who]]), N, device=dev)
    res = {"bench": "kg_rank", "entities": N, "relations": R, "dim": a.dim, "triples": n, "batch": a.batch,
           "known_triples": len(known), "filter_len_mean": round(float(lens.double().mean()), 2),
           "filter_len_max": int(lens.max()), "device": torch.cuda.get_device_name(0), "kinds": {}}

    for kind in a.kinds:
        torch.manual_seed(a.seed)
        args = (-1, [0], N - 1, R - 1, a.dim, a.dim)
        model = (Z.DistMult(*args) if kind == "dot" else Z.TransE(*args, l1=kind == "l1")).to(dev)
        out = {}
        ms, all_ms, peak, _ = _timed(lambda: kg_eval.rank_triples(model, src, rel, dst, known=known, batch=a.batch),
                                     a.repeat, torch)
        out["both_sides_filtered"] = {"ms": round(ms, 3), "ms_all": all_ms, "queries_per_s": round(2 * n / ms * 1e3, 1),
                                      "peak_bytes": peak}
        ms, all_ms, peak, ranks = _timed(lambda: kg_eval.rank_triples(model, src, rel, dst, sides=("tail",),
                                                                      batch=a.batch), a.repeat, torch)
        out["tail_raw"] = {"ms": round(ms, 3), "ms_all": all_ms, "queries_per_s": round(n / ms * 1e3, 1),
                           "peak_bytes": peak}
        if kind != "dot":
            ent = model.entity_encoder.weight.detach()[:N]
            rtab = model.relation_encoder.weight.detach()
            ms, all_ms, peak, comp = _timed(lambda: tail_ranks(ent, rtab, src, rel, dst, normalize=True, kind=kind),
                                            a.repeat, torch)
            out["tail_raw_composition"] = {"ms": round(ms, 3), "ms_all": all_ms,
                                           "queries_per_s": round(n / ms * 1e3, 1), "peak_bytes": peak,
                                           "ranks_equal_fraction":
                                               round(float((comp == ranks["tail"]).double().mean()), 6),
                                           "max_rank_difference": int((comp - ranks["tail"]).abs().max())}
        res["kinds"][kind] = out
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
