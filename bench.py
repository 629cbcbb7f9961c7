#!/usr/bin/env python3
"""Headline benchmark: GraphSAGE 2-hop training throughput (samples/sec, whole node).

BASELINE.json metric: "train samples/sec (whole node), GraphSAGE 2-hop on 100M-node
synthetic graph".  Config (defaults): 100M-node power-law synthetic graph (avg degree
10, ~1B weighted edges), 128-d bf16 node features, 64 classes, supervised GraphSAGE
(reference examples/graphsage: SAGEConv x2 + fc + out_fc, sigmoid CE, Adam), fanouts
[25, 10], 1024 roots per GPU per step (weak scaling), hidden 256.

The step is the framework's training path, euler_amd.models.sage_trainer.SageTrainer
(the same class NodeEstimator(device_graph=True) drives on loaded datasets): roots +
2 hops of neighbour sampling on the GPU, forward, backward, optimizer — four gfx950
launches captured in one hipGraph.  One process per GPU (torchrun): every rank holds
the whole graph + feature table in its own HBM with its own sample stream; the flat
gradient (fp32 by default, as the reference's synchronous gradient sync; --grad-reduce-dtype
bf16 halves the bytes) is all-reduced inside the captured step by the two-shot xGMI
peer-memory all-reduce (parallel/xgmi.py: every rank reads its peers' staged gradients
directly over the point-to-point links, two cross-GPU barriers instead of a ring's 2 (W-1)
hops) or by RCCL: with 2+ ranks the xGMI kernel's self-test runs on every rank, then both
are timed on the gradient buffer at start-up and the faster one is used (--grad-sync
xgmi / rccl forces one; the JSON config records the timings and the choice).  Nothing is skipped inside the timed
region.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full] [...]

A plain run sets up, warms up, times exactly --steps steps and prints one JSON line
(`ms_per_step` = milliseconds per timed step).  `--dump-outputs DIR` also writes the last timed
step's results as .npy files; `--full` is where anything beyond the headline figure belongs.

`--gpus N` without torchrun starts N ranks on this node itself (parallel/launch.py); under
torchrun it must equal WORLD_SIZE.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# dmabuf IPC is the only mode the MI355X host driver supports: RCCL and the xGMI all-reduce's
# peer mappings fail without it.  Set before anything can initialise HIP, so a torchrun launch
# behaves like the self-spawned one (parallel/launch.py sets it for its children too).
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--num-nodes", type=int, default=100_000_000)
    p.add_argument("--avg-degree", type=float, default=10.0)
    p.add_argument("--max-degree", type=int, default=1024)
    p.add_argument("--batch-size", type=int, default=1024, help="roots per GPU per step")
    p.add_argument("--fanouts", type=str, default="25,10")
    p.add_argument("--feature-dim", type=int, default=128)
    p.add_argument("--feature-dtype", choices=["bf16", "fp32"], default="bf16",
                   help="storage dtype of the HBM feature table (GEMMs are bf16 MFMA either way)")
    p.add_argument("--hidden-dim", type=int, default=256)
    p.add_argument("--label-dim", type=int, default=64)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--no-graph", action="store_true", help="eager steps instead of hipGraph replay")
    p.add_argument("--log", action="store_true")
    p.add_argument("--grad-reduce-dtype", choices=["bf16", "fp32"], default="fp32",
                   help="dtype of the data-parallel gradient all-reduce (bf16: half the bytes on xGMI, "
                        "summed in bf16 by RCCL)")
    p.add_argument("--grad-buckets", type=int, choices=[1, 2], default=1,
                   help="data-parallel gradient buckets: 1 = one all-reduce after the reduce (one stream); "
                        "2 = the head-layer bucket's reduce + all-reduce overlap the routed dW on a side stream")
    p.add_argument("--shard-features", action="store_true",
                   help="row-shard the feature table over the ranks (row r on rank r %% world); every step's "
                        "sampled rows come over an all-to-all (graph/sharded_features.py). Needs the process "
                        "group: torchrun, or --force-dist with one rank")
    p.add_argument("--steps-per-graph", type=int, default=32,
                   help="complete training steps captured per hipGraph (replays amortise the per-launch gap; "
                        "the timed region still runs exactly --steps steps)")
    p.add_argument("--force-dist", action="store_true",
                   help="take the multi-GPU code path (process group, all-reduce in the step) even with one rank")
    p.add_argument("--grad-sync", choices=["auto", "xgmi", "rccl", "tune"], default="auto",
                   help="data-parallel gradient all-reduce: auto = with 2+ ranks, the xGMI two-shot kernel's "
                        "self-test, then xGMI and RCCL timed on the gradient buffer and the faster kept; tune = "
                        "the same with one rank too")
    p.add_argument("--shared-gpu", action="store_true",
                   help="rehearsal: every rank on cuda:0 with a gloo process group (xGMI all-reduce only; "
                        "checks the multi-rank step on a one-GPU box)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step left with the caller of the training "
                        "path (loss, flat fp32 parameters, optimizer slots) as DIR/<name>.npy (float32); the same "
                        "arguments give the same inputs, so two builds can be compared output for output")
    p.add_argument("--full", action="store_true",
                   help="everything beyond the headline figure (extra measurements, comparisons, per-kernel numbers); "
                        "a plain run sets up, warms up, times --steps steps and prints the result line. The headline "
                        "run has no such extras today, so --full runs the same steps")
    return p.parse_args(argv)


def dump_outputs(tr, path):
    """What a caller of SageTrainer.step() holds after the last timed step: the step's loss, the
    flat fp32 parameters (trainer layout, logical_params() unpacks them) and the optimizer's two
    slots.  The fused single-process optimizer launch consumes the split-K gradient partials
    without storing the reduced gradient, so there is no gradient array to write."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    torch.cuda.synchronize()
    cap = 4 * 1024 * 1024  # elements per array: 16 MB each, under 64 MB in all
    for name, t in (("loss", tr.loss), ("params", tr.flat), ("adam_m", tr.m), ("adam_v", tr.v)):
        a = t.detach().to(torch.float32).cpu().numpy().reshape(-1)
        if a.size > cap:  # a fixed sample of a larger array (the same elements in every run)
            a = a[np.sort(np.random.default_rng(0).choice(a.size, cap, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


def _cpu_baseline():
    """BASELINE.md publishes no reference number; its prescribed comparison point is the
    reference-equivalent CPU path measured on the MI355X host (euler_amd/tools/cpu_baseline.py,
    result committed in profiles/cpu_baseline.json)."""
    path = os.path.join(ROOT, "profiles", "cpu_baseline.json")
    try:
        with open(path) as f:
            b = json.loads(f.readline())
        if "value_node_linear" in b:
            # whole node: the measured per-GPU host share scaled linearly to every core (an
            # upper bound for the CPU path, so vs_baseline is conservative)
            note = (f"profiles/cpu_baseline.json: reference-equivalent CPU path, {b['value']} samples/s on "
                    f"{b.get('threads')} host threads, linearly scaled to all {b['node_cores']} node cores: "
                    f"{b['value_node_linear']} samples/s ({b['config']['num_nodes']} nodes)")
            return float(b["value_node_linear"]), note
        note = (f"profiles/cpu_baseline.json: reference-equivalent CPU path, {b['value']} samples/s "
                f"({b.get('threads')} host threads, {b['config']['num_nodes']} nodes)")
        return float(b["value"]), note
    except (OSError, ValueError, KeyError):
        return None, None


def log(*a):
    print("[bench]", *a, file=sys.stderr, flush=True)


def main(argv=None):
    args = parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        # plain `python bench.py --gpus N`: start N ranks here (one process per GPU) before
        # anything touches the GPU; rank 0's JSON line is this process's stdout
        from euler_amd.parallel.launch import spawn_local

        return spawn_local(args.gpus, list(sys.argv[1:] if argv is None else argv), script=os.path.abspath(__file__))
    if env_world is not None and int(env_world) != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} disagrees with WORLD_SIZE={env_world} (torchrun --nproc-per-node)")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist_on = world > 1 or args.force_dist or args.shared_gpu
    if args.shared_gpu:
        local_rank = 0
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if args.shared_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (run through gpurun on an MI355X)")
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    from euler_amd.graph.device_graph import DeviceGraph
    from euler_amd.dataset.synthetic import synthetic_features, synthetic_labels
    from euler_amd.models.sage_trainer import SageTrainer

    fanouts = [int(x) for x in args.fanouts.split(",")]
    B = args.batch_size
    t0 = time.time()
    graph = DeviceGraph.synthetic(args.num_nodes, args.avg_degree, args.max_degree, seed=args.seed, device=dev)
    graph.manual_seed(args.seed * 7919 + rank)  # different root/neighbor draws per rank
    fdt = torch.bfloat16 if args.feature_dtype == "bf16" else torch.float32
    feats = synthetic_features(args.num_nodes, args.feature_dim, args.seed + 1, dev, dtype=fdt)
    labels = synthetic_labels(feats, args.label_dim)
    torch.cuda.synchronize()
    if rank == 0:
        log(f"graph: {graph.num_rows} nodes, {graph.num_edges} edges, csr {graph.nbytes()/2**30:.2f} GiB, "
            f"features {feats.numel()*feats.element_size()/2**30:.2f} GiB ({args.feature_dtype}), "
            f"build {time.time()-t0:.1f}s")

    dims = [args.hidden_dim] * (len(fanouts) + 1)  # reference run_graphsage: [hidden] * (layers + 1)
    fshard = None
    if args.shard_features:
        if not dist_on:
            raise SystemExit("--shard-features needs the process group (torchrun, or --force-dist with one rank)")
        from euler_amd.graph.sharded_features import ShardedFeatures

        fshard = ShardedFeatures(feats[rank::world].contiguous(), args.num_nodes, force_comm=True)
        feats = None  # this rank keeps its shard only
        torch.cuda.empty_cache()
    tr = SageTrainer(graph, B, fanouts, dims, args.label_dim, features=feats, labels=labels, learning_rate=args.lr,
                     init_seed=args.seed, keep_samples=False, grad_buckets=args.grad_buckets, feature_shard=fshard)
    xar = None
    sync_name = None
    sync_info = {}
    grad_sync = None
    if dist_on:
        from euler_amd.parallel.xgmi import make_grad_sync

        dist.broadcast(tr.flat, 0)
        tr.refresh_shadows()
        tr.set_grad_sync_dtype(args.grad_reduce_dtype)
        gbuf = tr.grad if getattr(tr, "grad16", None) is None else tr.grad16
        kind = "xgmi" if args.shared_gpu else args.grad_sync
        grad_sync, sync_name, sync_info = make_grad_sync(gbuf, kind, rebind=tr.use_grad_buffer)
        xar = sync_info.pop("xar")
        if rank == 0 and sync_info:
            log(f"gradient all-reduce: {sync_name} ({sync_info})")

    def timed_run(grad_sync):
        use_graph = not args.no_graph
        if use_graph:
            ok = True
            try:
                spg = max(1, args.steps_per_graph)
                # remainder graphs for the warm-up and timed counts: every step of the timed
                # region still runs, in as few replays as possible
                tr.capture(grad_sync, steps=spg, extra_sizes=(args.warmup % spg, args.steps % spg))
            except RuntimeError as e:  # e.g. a collective the runtime cannot capture
                ok = False
                log(f"rank {rank}: step capture failed ({e}); running eager steps")
            if dist_on:  # every rank takes the same path (captured collectives never ran)
                flag = torch.tensor([0 if ok else 1], dtype=torch.int32, device=dev)
                dist.all_reduce(flag)
                ok = int(flag.item()) == 0
            if not ok:
                tr._graph_exec = None
                use_graph = False

        if use_graph:
            def run_steps(n):
                tr.replay_steps(n)
        else:
            def run_steps(n):
                for _ in range(n):
                    tr.step(grad_sync)

        run_steps(args.warmup)
        torch.cuda.synchronize()
        first_loss = float(tr.loss.item())

        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        t_start = time.perf_counter()
        done = 0
        while done < args.steps:
            n = min(args.steps - done, 48 if args.log else args.steps)
            run_steps(n)
            done += n
            if args.log and rank == 0:
                torch.cuda.synchronize()
                log(f"step {done} loss {float(tr.loss.item()):.4f}")
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        elapsed = time.perf_counter() - t_start
        el = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        if dist_on:
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
        return float(el.item()), first_loss, use_graph

    elapsed, first_loss, use_graph = timed_run(grad_sync)
    if xar is not None:
        # a cross-GPU wait that timed out (lost peer) leaves a wrong sum behind, never a hang:
        # every rank agrees and the measurement is repeated over RCCL
        flag = torch.tensor([xar.error()], dtype=torch.int32, device=dev if not args.shared_gpu else "cpu")
        dist.all_reduce(flag)
        if int(flag.item()) != 0 and not args.shared_gpu:
            log("xGMI all-reduce timed out on some rank during the run; re-measuring over RCCL")
            torch.cuda.synchronize()
            tr.release_graphs()
            sync_name = "rccl (xgmi timed out)"
            elapsed, first_loss, use_graph = timed_run(make_grad_sync(gbuf, "rccl")[0])
        elif int(flag.item()) != 0:
            raise SystemExit("xGMI all-reduce timed out")
    last_loss = float(tr.loss.item())
    if fshard is not None:
        fshard.check_overflow()
    ms = elapsed * 1000.0 / max(args.steps, 1)
    value = world * B * args.steps / elapsed
    base_value, base_note = _cpu_baseline()
    if rank == 0 and args.dump_outputs:
        dump_outputs(tr, args.dump_outputs)
    if rank == 0:
        log(f"loss after warmup {first_loss:.4f} -> after timed steps {last_loss:.4f}")
        out = {
            # the BASELINE.json metric on its 100M-node config; other sizes (BASELINE config 2:
            # --num-nodes 10000000) say so in the name and carry no vs_baseline
            "metric": "train samples/sec (whole node), GraphSAGE 2-hop on %s synthetic graph" % (
                "100M-node" if args.num_nodes == 100_000_000 else "%gM-node" % (args.num_nodes / 1e6)),
            "value": round(value, 1),
            "unit": "samples/s",
            # a --shared-gpu rehearsal runs every rank on one physical GPU: n_gpus counts the
            # devices, "ranks" the processes, and the number is no whole-node result
            "n_gpus": 1 if args.shared_gpu else world,
            "ranks": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": (round(value / base_value, 2) if base_value and args.num_nodes == 100_000_000
                            and not args.shared_gpu else None),
            # the CPU comparison point is measured on the 16 host threads a job may use and
            # scaled linearly to the node's cores (profiles/cpu_baseline.json)
            "vs_baseline_kind": ("extrapolated CPU baseline (16 measured host threads scaled linearly to all node "
                                 "cores)" if base_note and "linearly scaled" in base_note else "measured CPU baseline"),
            "dtype": "bf16",
            "data": "synthetic (power-law random graph + random-normal features, random-init weights)",
            "config": {
                "model": "GraphSAGE supervised (2x SAGEConv mean + fc + out_fc, sigmoid CE, Adam)",
                "global_batch": B * world,
                "seq_len": None,
                "parallelism": f"dp{world}",
                "num_nodes": args.num_nodes,
                "num_edges": graph.num_edges,
                "fanouts": fanouts,
                "feature_dim": args.feature_dim,
                "feature_dtype": args.feature_dtype,
                "hidden_dim": args.hidden_dim,
                "label_dim": args.label_dim,
                "hipgraph": use_graph,
                "steps_per_graph": args.steps_per_graph if use_graph else None,
                "feature_sharding": (f"row-sharded over {world} rank(s), per-step all-to-all of the sampled rows"
                                     if fshard is not None else None),
                "grad_sync": (f"{sync_name} all-reduce ({args.grad_reduce_dtype} gradient, {args.grad_buckets} "
                              f"bucket(s)) in the captured step" if dist_on else None),
                "grad_sync_choice": sync_info or None,
                "shared_gpu_rehearsal": bool(args.shared_gpu) or None,
                "impl": "euler_amd.models.sage_trainer.SageTrainer (4 fused gfx950 launches per step)",
                "loss_first_last": [round(first_loss, 4), round(last_loss, 4)],
                "baseline": base_note,
            },
        }
        print(json.dumps(out), flush=True)
    if dist_on:
        # a live graph holding captured collectives keeps the communicator busy: drop it first
        torch.cuda.synchronize()
        tr.release_graphs()
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
