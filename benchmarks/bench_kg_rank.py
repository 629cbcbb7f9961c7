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

Each figure is the median of ``--repeat`` passes after a warm-up pass, with
``torch.cuda.synchronize`` around the timed region; peak bytes are what a pass allocates over
what was allocated before it.  Prints one JSON line.

    python benchmarks/bench_kg_rank.py [--entities 14951] [--relations 1345] [--dim 100]
        [--triples 59071] [--batch 4096] [--repeat 3] [--kinds l1 l2 dot]
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
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_kg_rank measures on a GPU; none is available")
    from euler_amd import models as Z
    from euler_amd.dataset.synthetic import tail_ranks
    from euler_amd.models import kg_eval

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(a.seed)
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
