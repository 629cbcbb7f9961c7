"""Random walks on the row-sharded device graph (graph/sharded_graph.py
ShardedDeviceGraph.random_walk, csrc/hip/walk_shard.hip; reference
tf_euler/kernels/random_walk_op.cc:172-291 over euler/core/kernels/remote_op.cc:60-146) and
the skip-gram walk models trained on it (estimator/device_trainers.py build_sharded_trainer,
models/deepwalk_step.py).

CPU (gloo, the composed path): every step of every walk is a real neighbour of the previous
row in the whole graph, ended walkers write the default, one-step frequencies follow the
edge weights, node2vec bias is refused; NodeEstimator(device_graph_sharded=True) trains
DeepWalk on 2 ranks holding half of the graph each; an overflow seen by one rank raises on
both in the same step.

GPU: on a one-rank RCCL group the fused hop kernels reproduce the whole-graph walk kernel
bit for bit (the oracle of the shared draw function, the request packing and the unroute);
the walk records into a hipGraph and is redrawn every replay; two processes sharing the
GPU walk across both shards."""
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_parallel import _free_port, _init, _run  # noqa: E402

N, T = 300, 2


def _graph(n=N, seed=0, device="cpu"):
    """300 rows, 2 edge types, row 7 without out-edges (tests/test_sharded_graph.py _graph)"""
    from euler_amd.graph.device_graph import DeviceGraph

    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 9, (n * T,), generator=g)
    deg[7 * T: 7 * T + T] = 0
    indptr = torch.zeros(n * T + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(deg, 0)
    E = int(indptr[-1])
    nbr = torch.randint(0, n, (E,), generator=g)
    w = torch.rand(E, generator=g) + 0.1
    nw = torch.rand(n, generator=g).numpy() + 0.05
    dg = DeviceGraph.from_csr(indptr.numpy(), nbr.numpy(), w.numpy(), T, node_weights=nw, seed=5, device=device)
    return dg, indptr, nbr, w, nw


def _starts(n, seed):
    s = torch.randint(0, N, (n,), generator=torch.Generator().manual_seed(seed))
    s[3], s[10], s[11] = 7, -1, 7
    return s


def _walks_ok(walks, starts, indptr, nbr, types, default):
    """every step a neighbour of the previous row over ``types`` in the whole graph; a walker
    without a row to step from (< 0, >= N, no such edge) writes ``default`` — and goes on
    from it when ``default`` is itself a row"""
    walks = walks.cpu().long()
    if not torch.equal(walks[:, 0], starts.cpu().long()):
        return False
    for row in walks.tolist():
        for a, b in zip(row[:-1], row[1:]):
            cand = set()
            if 0 <= a < N:
                for t in types:
                    cand |= set(nbr[int(indptr[a * T + t]): int(indptr[a * T + t + 1])].tolist())
            if (b not in cand) if cand else (b != default):
                return False
    return True


def _hot_row(indptr):
    return int(torch.argmax(indptr[2::2] - indptr[1::2]))  # the row with the most type-1 edges


def _one_step_tv(sg, indptr, nbr, w, device="cpu"):
    """TV distance of 60,096 one-step draws from the hot row to its type-1 edge weights (192
    walkers a time: all of them go to one owner, and capacity(192) = 192 for 2..4 ranks)"""
    hot = _hot_row(indptr)
    assert sg.capacity(192) == 192
    draws = []
    for _ in range(313):
        sg.advance()
        if device == "cpu":
            sg.reseed_cpu()
        draws.append(sg.random_walk(torch.full((192,), hot, device=device), 1, edge_types=[1])[:, 1])
    d = torch.cat(draws).long().cpu()
    assert bool((d >= 0).all())
    cnt = torch.zeros(N).index_add_(0, d, torch.ones(d.numel()))
    a, b = int(indptr[hot * T + 1]), int(indptr[hot * T + 2])
    exp = torch.zeros(N).index_add_(0, nbr[a:b], w[a:b])
    return float((cnt / cnt.sum() - exp / exp.sum()).abs().sum() / 2)


# ----------------------------------------------------------------------------------- CPU
def test_one_rank_without_comm_is_the_local_walk_cpu():
    from euler_amd.graph.sharded_graph import ShardedDeviceGraph

    g, *_ = _graph()
    sg = ShardedDeviceGraph.from_full(g)
    starts = _starts(200, 1)
    sg.manual_seed(9)
    a = sg.random_walk(starts, 4)
    sg.manual_seed(9)
    b = sg.local.random_walk(starts, 4)
    assert a.shape == (200, 5) and torch.equal(a, b)


def _worker_walks(rank, world, port, q):
    try:
        _init(rank, world, port)
        from euler_amd.graph.sharded_graph import ShardedDeviceGraph

        g, indptr, nbr, w, nw = _graph()
        sg = ShardedDeviceGraph.from_full(g, node_weights=nw)
        starts = _starts(400, rank)
        ok = True
        for default in (-1, N):
            sg.advance()
            sg.reseed_cpu()
            walks = sg.random_walk(starts, 4, edge_types=[1], default=default)
            ok &= walks.shape == (400, 5) and walks.dtype == torch.int32
            ok &= _walks_ok(walks, starts, indptr, nbr, [1], default)
            ok &= bool((walks[10, 1:] == default).all()) and bool((walks[3, 1:] == default).all())
            ok &= bool((walks[:, 1] != default).sum() > 300)  # the walkers do move
        tv = _one_step_tv(sg, indptr, nbr, w)
        ok &= tv < 0.03
        sg.check_overflow()
        try:
            sg.random_walk(starts, 2, p=2.0)
            ok = False
        except ValueError as e:
            ok &= "node2vec" in str(e)
        q.put((rank, "walks", bool(ok), tv))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "error", traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharded_walks_support_defaults_and_frequencies(world):
    res = _run(_worker_walks, world=world)
    assert not [r for r in res if r[1] == "error"], res
    assert len(res) == world and all(r[2] for r in res), res


def _deepwalk_estimator(data_dir, model_dir, total, sharded_kind=True, graph=None):
    import euler_amd as ea
    from euler_amd import models as Z
    from euler_amd.estimator import NodeEstimator

    if graph is None:
        from euler_amd.dataset import get_dataset

        ds = get_dataset("cora", data_dir=data_dir, scale=0.08)
        ds.load_graph()
        max_id = ds.max_node_id
        tnt = ds.train_node_type[0] if isinstance(ds.train_node_type, list) else ds.train_node_type
        et = ["train"]
    else:
        max_id, tnt, et = graph, -1, ["0", "1"]
    ea.set_seed(3)
    torch.manual_seed(0)
    m = Z.DeepWalk(tnt, et, max_id, 8, walk_len=3, num_negs=3, sharded=True)
    est = NodeEstimator(m, {"model_dir": model_dir, "batch_size": 32, "total_step": total, "optimizer": "adam",
                            "learning_rate": 0.05, "log_steps": 10, "train_node_type": tnt, "device": "cpu",
                            "device_graph": True, "device_graph_sharded": sharded_kind, "seed": 11})
    return m, est


def _record_losses():
    from euler_amd.models.deepwalk_step import DeepWalkEstimatorTrainer as D

    losses, orig = [], D._one

    def rec(self):
        out = orig(self)
        losses.append(float(out))
        return out

    D._one = rec
    return losses


def _worker_estimator(rank, world, port, q, data_dir, model_dir, out_dir, total):
    """DeepWalk(sharded=True) under NodeEstimator(device_graph_sharded=True): trains to
    ``total`` (or only restores the per-rank shard checkpoint) and dumps this rank's rows"""
    try:
        _init(rank, world, port)
        losses = _record_losses()
        m, est = _deepwalk_estimator(data_dir, model_dir, total)
        est.train()
        tr = est.device_trainer
        g = tr.graph
        ok = tr.device_trainer_kind == ("sharded_skipgram_walks" if world > 1 else "skipgram_walks")
        if world > 1:
            ok &= g.world == world and g.local.num_rows == len(range(rank, g.num_rows, world))
            ok &= len(losses) == total and all(math.isfinite(x) for x in losses)
            ok &= sum(losses[-10:]) < sum(losses[:10])
            g.check_overflow()
        rows = tr._half_rows()
        keep = rows < tr.num
        t = tr.inner.table
        dump = {key: {"rows": rows[keep].clone(), "weight": t.weight[h * tr._offw: (h + 1) * tr._offw][keep].clone()}
                for h, key in enumerate(tr._keys)}
        torch.save(dump, os.path.join(out_dir, "w%d_r%d.pt" % (world, rank)))
        q.put((rank, "estimator", bool(ok), losses[:3], losses[-3:]))
        if dist.is_initialized():
            dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "error", traceback.format_exc()))


def test_estimator_trains_deepwalk_on_the_sharded_graph_and_reshards(tmp_path):
    out = tmp_path / "dump"
    out.mkdir()
    args = (str(tmp_path / "cora"), str(tmp_path / "ckpt"), str(out), 40)
    res = _run(_worker_estimator, *args, world=2)
    assert not [r for r in res if r[1] == "error"], res
    assert len(res) == 2 and all(r[2] for r in res), res
    # the checkpoint written by 2 ranks restores under 1 rank (the one-rank fallback)
    res = _run(_worker_estimator, *args, world=1)
    assert not [r for r in res if r[1] == "error"], res
    assert len(res) == 1 and res[0][2], res
    one = torch.load(out / "w1_r0.pt", weights_only=True)
    for r in range(2):
        part = torch.load(out / ("w2_r%d.pt" % r), weights_only=True)
        for key, d in part.items():
            full = torch.zeros_like(one[key]["weight"])
            full[one[key]["rows"]] = one[key]["weight"]
            assert torch.equal(full[d["rows"]], d["weight"]), (r, key)


def _worker_engine_shard_estimator(rank, world, port, q, data, tmp):
    """device_graph_sharded="engine_shards": each rank's engine holds half of the partitions,
    the graph's rows are not in id order (the trainer maps them through ``row_ids``)"""
    try:
        _init(rank, world, port)
        from euler_amd.ops.base import initialize_graph

        initialize_graph({"mode": "local", "data_path": data, "shard_idx": rank, "shard_num": world})
        losses = _record_losses()
        m, est = _deepwalk_estimator(None, os.path.join(tmp, "ck"), 40, "engine_shards", graph=2999)
        est.train()
        tr = est.device_trainer
        g = tr.graph
        ok = tr.device_trainer_kind == "sharded_skipgram_walks" and g.ids is None and g.local.num_rows < 3000
        ok &= all(math.isfinite(x) for x in losses) and sum(losses[-10:]) < sum(losses[:10])
        # the row map sends every graph row to its node id, padding rows and the walk's pad
        # to the model's pad row
        rid = g.row_ids.cpu()
        rm = tr.inner.row_map.cpu()
        ok &= rm.numel() == g.num_rows + 1 and int(rm[-1]) == 3000
        ok &= torch.equal(rm[:-1], torch.where(rid >= 0, rid, torch.full_like(rid, 3000)))
        # pairs are (id, id of a neighbour): check against this rank's engine where it owns the id
        src, pos, _ = tr.inner.sample()
        ok &= bool(((src >= 0) & (src <= 3000) & (pos >= 0) & (pos <= 3000)).all())
        g.check_overflow()
        q.put((rank, "engine_shard_walks", bool(ok), losses[:3], losses[-3:]))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "error", traceback.format_exc()))


def test_estimator_deepwalk_on_per_rank_engine_shards(tmp_path):
    import euler_amd as ea

    data = str(tmp_path / "g")
    e = ea.synthetic_graph(3000, 6.0, 64, node_types=1, edge_types=2, feature_dim=8, label_dim=4, seed=3,
                           make_current=False)
    e.save(data, partitions=4, threads=4)
    res = _run(_worker_engine_shard_estimator, data, str(tmp_path))
    assert not [r for r in res if r[1] == "error"], res
    assert len(res) == 2 and all(r[2] for r in res), res


def _worker_refusals(rank, world, port, q, data_dir, tmp):
    try:
        _init(rank, world, port)
        from euler_amd import models as Z
        from euler_amd.dataset import get_dataset
        from euler_amd.estimator import NodeEstimator
        from euler_amd.estimator.device_trainers import NoDeviceTrainer, build_sharded_trainer, sharded_supported

        ds = get_dataset("cora", data_dir=data_dir, scale=0.08)
        ds.load_graph()
        n2v = Z.Node2Vec("train", ["train"], ds.max_node_id, 8, walk_len=3, num_negs=3, walk_p=0.5)
        line1 = Z.Line("train", ["train"], ds.max_node_id, 8, num_negs=3, order=1)
        line2 = Z.Line("train", ["train"], ds.max_node_id, 8, num_negs=3, order=2)
        ok = sharded_supported(line2) and sharded_supported(n2v) and not sharded_supported(line1)
        msgs = []
        for m in (n2v, line1):
            est = NodeEstimator(m, {"model_dir": os.path.join(tmp, "ck"), "batch_size": 32, "device": "cpu",
                                    "device_graph": True, "device_graph_sharded": True})
            try:
                build_sharded_trainer(est, m, None)
                ok = False
            except NoDeviceTrainer as e:
                msgs.append(str(e))
        ok &= len(msgs) == 2 and "node2vec" in msgs[0] and "first-order LINE" in msgs[1]
        q.put((rank, "refusals", bool(ok), msgs))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "error", traceback.format_exc()))


def test_sharded_trainer_refuses_node2vec_bias_and_first_order_line(tmp_path):
    res = _run(_worker_refusals, str(tmp_path / "cora"), str(tmp_path))
    assert not [r for r in res if r[1] == "error"], res
    assert len(res) == 2 and all(r[2] for r in res), res


def _worker_overflow(rank, world, port, q):
    """rank 0 walks 512 rows of ONE owner: more than the owner's capacity(512) = 448 slots,
    so rank 0's graph flag is set and rank 1's is not; the trainer's periodic check (every 2
    steps) raises on both ranks in step 2"""
    try:
        _init(rank, world, port)
        from euler_amd.graph.sharded_graph import ShardedDeviceGraph
        from euler_amd.models.deepwalk_step import DeepWalkTrainer

        g, indptr, nbr, w, nw = _graph()
        sg = ShardedDeviceGraph.from_full(g, node_weights=nw)
        tr = DeepWalkTrainer(sg, N, dim=8, walk_len=2, num_negs=2, batch_size=64, static=True, seed=5,
                             overflow_check_every=2)
        starts = torch.arange(512) % 140 * 2 if rank == 0 else _starts(512, 1)
        assert sg.capacity(512) == 448
        sg.advance()
        sg.reseed_cpu()
        walks = sg.random_walk(starts, 1)
        own = int(sg.overflow.item())
        ended = int((walks[:, 1] == -1).sum())
        raised_at = None
        for _ in range(4):
            try:
                tr.step()
            except RuntimeError as e:
                raised_at = (tr.steps_done, "graph" in str(e))
                break
        ok = own == (1 if rank == 0 else 0) and raised_at == (2, True) and int(tr.table.overflow.item()) == 0
        ok &= ended >= 512 - 448 if rank == 0 else ended < 40
        q.put((rank, "overflow", bool(ok), own, raised_at, ended))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "error", traceback.format_exc()))


def test_walk_overflow_on_one_rank_raises_on_every_rank_in_the_same_step():
    res = _run(_worker_overflow)
    assert not [r for r in res if r[1] == "error"], res
    assert len(res) == 2 and all(r[2] for r in res), res


# ----------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_fused_hops_equal_the_whole_graph_walk_kernel_bitwise():
    """one-rank RCCL group, force_comm: request packing, route, all-to-all, the owner's draw
    and the unroute reproduce ``random_walk_kernel`` on the same rng state, bit for bit"""
    from euler_amd.graph.sharded_graph import ShardedDeviceGraph

    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        g, indptr, nbr, w, nw = _graph(device="cuda")
        sg = ShardedDeviceGraph.from_full(g, force_comm=True, node_weights=nw)
        assert sg.comm and sg.world == 1
        starts = _starts(600, 2)  # two full 256-thread blocks and a partial one
        starts[20] = N + 5
        starts = starts.cuda()
        for types in ([1], None):
            for default in (-1, N):
                sg.advance()
                a = sg.random_walk(starts, 5, edge_types=types, default=default)
                b = sg.local.random_walk(starts, 5, edge_types=types, default=default)
                assert a.dtype == torch.int32 and a.shape == (600, 6)
                assert torch.equal(a, b), (types, default)
                assert _walks_ok(a, starts, indptr, nbr, [1] if types else [0, 1], default)
                assert bool((a[20, 1:] == default).all()) and bool((a[10, 1:] == default).all())
        # the torch composition of the same hops draws valid walks too
        c = sg._random_walk_composed(starts, 5, [1], -1)
        assert _walks_ok(c, starts, indptr, nbr, [1], -1)
        sg.check_overflow()
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_deepwalk_step_captures_over_rccl_and_redraws_walks():
    from euler_amd.graph.sharded_graph import ShardedDeviceGraph
    from euler_amd.models.deepwalk_step import DeepWalkTrainer

    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    tr = None
    try:
        g, indptr, nbr, w, nw = _graph(device="cuda")
        sg = ShardedDeviceGraph.from_full(g, force_comm=True, node_weights=nw)
        tr = DeepWalkTrainer(sg, N, dim=32, walk_len=3, batch_size=256, lr=0.05, seed=5, static=True,
                             force_comm=True)
        seen = []
        walk = sg.random_walk

        def keep(*a, **k):
            seen.append(walk(*a, **k))
            return seen[-1]

        sg.random_walk = keep
        tr.capture(warm=2)
        captured = seen[-1]  # the walks tensor of the recorded step
        first = float(tr.warm_loss)
        losses, draws = [], []
        for _ in range(20):
            tr.step()
            losses.append(tr.loss.clone())
            draws.append(captured.clone())
        torch.cuda.synchronize()
        losses = [float(x) for x in losses]
        assert all(math.isfinite(x) for x in losses) and sum(losses[-5:]) / 5 < first, (first, losses)
        assert int(sg.overflow.item()) == 0
        tr.check_overflow()
        assert not torch.equal(draws[0], draws[1]) and not torch.equal(draws[-2], draws[-1])
        assert _walks_ok(draws[-1], draws[-1][:, 0], indptr, nbr, [0, 1], N)
    finally:
        if tr is not None:
            tr.release()  # a graph holding RCCL work blocks destroy_process_group
        dist.destroy_process_group()


def _worker_shared_gpu(rank, world, port, q):
    """2 processes sharing the GPU (gloo, the all-to-alls staged through host memory): the
    fused hop kernels across two shards"""
    try:
        os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                           "WORLD_SIZE": str(world), "LOCAL_RANK": "0"})
        from euler_amd.graph.sharded_graph import ShardedDeviceGraph
        from euler_amd.parallel import dp

        dp.init_distributed(backend="gloo", device=torch.device("cuda", 0))
        g, indptr, nbr, w, nw = _graph(device="cuda")
        sg = ShardedDeviceGraph.from_full(g, node_weights=nw)
        starts = _starts(512, 10 + rank).cuda()
        ok = sg.world == 2 and sg.local.num_rows == N // 2
        runs = []
        for _ in range(2):
            sg.manual_seed(21 + rank)
            sg.advance()
            runs.append(sg.random_walk(starts, 4, edge_types=[1]))
        ok &= torch.equal(runs[0], runs[1])
        ok &= _walks_ok(runs[0], starts, indptr, nbr, [1], -1)
        ok &= bool((runs[0][10, 1:] == -1).all()) and bool((runs[0][3, 1:] == -1).all())
        sg.advance()
        ok &= _walks_ok(sg.random_walk(starts, 4, default=N), starts, indptr, nbr, [0, 1], N)
        tv = _one_step_tv(sg, indptr, nbr, w, device="cuda")
        ok &= tv < 0.03
        sg.check_overflow()
        q.put((rank, "shared_gpu_walks", bool(ok), tv))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "error", traceback.format_exc()))


@pytest.mark.gpu
def test_fused_hops_two_ranks_share_the_gpu():
    res = _run(_worker_shared_gpu)
    assert not [r for r in res if r[1] == "error"], res
    assert len(res) == 2 and all(r[2] for r in res), res
