"""EdgeEstimator.rank_evaluate() under 2 CPU ranks over gloo: each rank ranks its share of the
id file and the sums are all-reduced before the division, so every rank returns the metrics
of the whole file (the same code path runs over RCCL on GPUs)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _estimator(data_dir, model_dir):
    import euler_amd as ea
    from euler_amd import models as Z
    from euler_amd.dataset import get_dataset
    from euler_amd.estimator import EdgeEstimator

    ds = get_dataset("fb15k", data_dir=data_dir, scale=0.01)
    ds.load_graph()
    ea.set_seed(3)
    torch.manual_seed(0)  # no checkpoint: every process builds the same tables
    m = Z.TransE("train", "train", ds.max_node_id, ds.max_edge_id, 16, 16, num_negs=4)
    return EdgeEstimator(m, {"model_dir": model_dir, "batch_size": 16, "device": "cpu", "train_edge_type": "train",
                             "id_file": ds.edge_id_file, "rank_filter_edge_types": list(ds.all_edge_type)})


def _worker(rank, world, port, q, data_dir, model_dir):
    try:
        os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                           "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank)})
        import torch.distributed as dist

        from euler_amd.parallel import dp

        dp.init_distributed(backend="gloo", device=torch.device("cpu"))
        est = _estimator(data_dir, model_dir)
        share = sum(len(b) for b in est.get_input_from_id_file())
        q.put((rank, share, est.rank_evaluate()))
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put((rank, "error", repr(e)))


def test_rank_evaluate_two_ranks(tmp_path):
    data_dir, model_dir = str(tmp_path / "data"), str(tmp_path / "ckpt")
    want = _estimator(data_dir, model_dir).rank_evaluate()  # also writes the dataset files once
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, data_dir, model_dir)) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(60)
        if p.is_alive():
            p.kill()
    assert not [r for r in out if r[1] == "error"], out
    assert sum(r[1] for r in out) == want["n"] and all(0 < r[1] < want["n"] for r in out)
    for _, _, res in out:
        assert res["n"] == want["n"]
        for key in ("mrr", "mr", "hit@1", "hit@3", "hit@10"):
            assert res[key] == pytest.approx(want[key], rel=1e-12)
            assert res["head"][key] == pytest.approx(want["head"][key], rel=1e-12)
            assert res["tail"][key] == pytest.approx(want["tail"][key], rel=1e-12)
