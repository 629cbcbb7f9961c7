"""An edge list as the estimator's graph: ``edge_list_factory`` ->
``params["device_graph_factory"]`` -> ``DeviceGraph.from_edges``; train, evaluate and infer
with no graph engine initialised in the process."""
import logging

import numpy as np
import pytest
import torch

from euler_amd import models as Z
from euler_amd.estimator import NodeEstimator
from euler_amd.graph import edge_list_factory
from euler_amd.graph.device_graph import DeviceGraph

N, C, FD, DEG = 2000, 8, 16, 8


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """planted communities: 2,000 nodes in 8 classes, 16-d features around the class mean,
    ~8 out edges per node (90 % inside the class), dyadic weights (every prefix sum exact in
    fp32), raw ids with gaps, edges in random order"""
    rng = np.random.default_rng(0)
    cls = rng.integers(0, C, N)
    ids = np.arange(N, dtype=np.int64) * 3 + 5
    members = [np.flatnonzero(cls == c) for c in range(C)]
    src = np.repeat(np.arange(N), DEG)
    inside = rng.random(N * DEG) < 0.9
    dst = np.where(inside, np.array([members[c][rng.integers(0, len(members[c]))] for c in cls[src]]),
                   rng.integers(0, N, N * DEG))
    w = (rng.integers(1, 17, N * DEG) * 0.25).astype(np.float32)
    p = rng.permutation(N * DEG)
    means = rng.standard_normal((C, FD)).astype(np.float32)
    feats = (means[cls] + 0.5 * rng.standard_normal((N, FD))).astype(np.float32)
    labels = np.eye(C, dtype=np.float32)[cls]
    arrays = {"src": ids[src[p]], "dst": ids[dst[p]], "weight": w[p], "node_ids": ids, "features": feats,
              "labels": labels}
    d = tmp_path_factory.mktemp("planted")
    path = str(d / "graph.npz")
    np.savez(path, **arrays)
    id_file = str(d / "ids.txt")
    with open(id_file, "w") as f:
        f.write("\n".join(str(int(i)) for i in ids[::7]) + "\n")
    return {"path": path, "arrays": arrays, "id_file": id_file, "rows": (src[p], dst[p]), "n_eval": len(ids[::7])}


class _Losses(logging.Handler):
    """the loss of every logged training step (log_steps = 1)"""

    def __init__(self):
        super().__init__(level=logging.INFO)
        self.losses = []

    def emit(self, record):
        if isinstance(record.msg, str) and record.msg.startswith("step = ") and record.args:
            self.losses.append(float(record.args[1]))

    def __enter__(self):
        self.log = logging.getLogger("euler_amd.estimator")
        self.level = self.log.level
        self.log.setLevel(logging.INFO)
        self.log.addHandler(self)
        return self

    def __exit__(self, *exc):
        self.log.removeHandler(self)
        self.log.setLevel(self.level)


def _sage():
    torch.manual_seed(0)
    return Z.SupervisedGraphSage([16, 16, C], [4, 4], [[0], [0]], "feature", FD, "label", C, max_id=N * 3 + 5)


def _params(tmp, device, factory, steps, id_file=None, **kw):
    p = {"model_dir": str(tmp / "ckpt"), "batch_size": 64, "total_step": steps, "optimizer": "adam",
         "learning_rate": 0.01, "log_steps": 1, "train_node_type": -1, "device": device, "device_graph": True,
         "device_graph_factory": factory, "seed": 5, "infer_dir": str(tmp / "infer")}
    if id_file:
        p["id_file"] = id_file
    p.update(kw)
    return p


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    """no graph engine for the tests of this file (whatever an earlier test of the process
    initialised): any reach for it raises 'graph not initialized'"""
    from euler_amd.ops import base

    monkeypatch.setattr(base, "_ENGINE", None)


def _no_engine():
    from euler_amd.ops import base

    assert base._ENGINE is None, "this test must run without an initialised graph engine"


def _train_eval_infer(planted, tmp_path, device):
    _no_engine()
    est = NodeEstimator(_sage(), _params(tmp_path, device, edge_list_factory(planted["path"]), 60,
                                         planted["id_file"]))
    with _Losses() as h:
        est.train()
    assert len(h.losses) >= 20
    first, last = np.mean(h.losses[:10]), np.mean(h.losses[-10:])
    print("loss: first 10 steps %.4f, last 10 steps %.4f" % (first, last))
    assert last < first
    ev = est.evaluate()
    assert len(ev) == 2 and all(np.isfinite(v) for v in ev.values()) and "loss" in ev
    ids, emb = est.infer()
    want = np.loadtxt(planted["id_file"], dtype=np.int64)
    assert np.array_equal(np.asarray(ids).reshape(-1), want)
    assert emb.shape[0] == planted["n_eval"] and np.isfinite(emb).all()
    assert np.load(str(tmp_path / "infer" / "embedding_0.npy")).shape[0] == planted["n_eval"]
    _no_engine()
    return est


def test_estimator_trains_from_edge_list_without_engine_cpu(planted, tmp_path):
    _train_eval_infer(planted, tmp_path, "cpu")


@pytest.mark.gpu
def test_estimator_trains_from_edge_list_without_engine_gpu(planted, tmp_path):
    est = _train_eval_infer(planted, tmp_path, "cuda")
    assert est.device_trainer.graph.indptr.is_cuda


def _sorted_csr(planted):
    """the oracle's arrays: numpy lexsort by (row, dst, input index)"""
    a = planted["arrays"]
    src, dst = planted["rows"]
    order = np.lexsort((np.arange(len(src)), dst, src))
    indptr = np.searchsorted(src[order], np.arange(N + 1)).astype(np.int64)
    return indptr, dst[order].astype(np.int32), a["weight"][order]


def _csr_factory(planted):
    a = planted["arrays"]
    indptr, nbr, w = _sorted_csr(planted)

    def factory(rank, device):
        g = DeviceGraph.from_csr(indptr, nbr, w, 1, ids=a["node_ids"].astype(np.uint64), seed=rank, device=device)
        g.features = torch.from_numpy(a["features"]).to(device).to(torch.bfloat16)
        g.labels = torch.from_numpy(a["labels"]).to(device)
        return g

    return factory


def test_same_trajectory_as_a_from_csr_graph_cpu(planted, tmp_path):
    """the same model, seed and sampler key on the from_edges graph and on the from_csr graph of
    the numpy-sorted arrays: identical loss sequences (the weights are dyadic, so the two
    graphs are bit-identical)"""
    seqs = []
    for tag, factory in (("edges", edge_list_factory(planted["arrays"])), ("csr", _csr_factory(planted))):
        est = NodeEstimator(_sage(), _params(tmp_path / tag, "cpu", factory, 12))
        with _Losses() as h:
            est.train()
        seqs.append(h.losses)
    assert len(seqs[0]) == 12 and seqs[0] == seqs[1]


@pytest.mark.gpu
def test_same_arrays_as_a_from_csr_graph_gpu(planted):
    g = edge_list_factory(planted["path"])(0, torch.device("cuda"))
    r = _csr_factory(planted)(0, torch.device("cuda"))
    assert g.nbr.is_cuda
    for k in ("indptr", "nbr", "cumw", "features", "labels"):
        assert torch.equal(getattr(g, k), getattr(r, k)), k
    assert np.array_equal(np.asarray(g.ids), np.asarray(r.ids))


def test_deepwalk_trains_from_edge_list_cpu(planted, tmp_path):
    _no_engine()
    a = planted["arrays"]
    src, dst = planted["rows"]  # ids are rows: the id tables are indexed by row
    factory = edge_list_factory({"src": src, "dst": dst, "weight": a["weight"]}, num_nodes=N)
    torch.manual_seed(0)
    model = Z.DeepWalk(-1, -1, N - 1, 16, walk_len=3, num_negs=5)
    est = NodeEstimator(model, _params(tmp_path, "cpu", factory, 40, learning_rate=0.05))
    with _Losses() as h:
        est.train()
    first, last = np.mean(h.losses[:10]), np.mean(h.losses[-10:])
    print("DeepWalk loss: first 10 steps %.4f, last 10 steps %.4f" % (first, last))
    assert len(h.losses) == 40 and last < first
    _no_engine()


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_composes_with_knn_search_output(device):
    """a kNN graph straight from FlatIndex.search's output: every drawn neighbour is
    one of the row's k neighbours"""
    from euler_amd.tools.knn import FlatIndex

    n, k = 500, 6
    x = torch.randn(n, 12, generator=torch.Generator().manual_seed(1))
    index = FlatIndex(12, device=device)
    index.add(x)
    D, I = index.search(x, k)
    g = DeviceGraph.from_edges(np.repeat(np.arange(n), k), I.reshape(-1), np.exp(-D).reshape(-1), num_nodes=n,
                               device=device, seed=3)
    assert g.indptr.device.type == device and g.num_edges == n * k
    draws = g.sample_neighbor(torch.arange(n, dtype=torch.int32, device=g.device), 10).long().cpu()
    assert ((draws.unsqueeze(2) == torch.as_tensor(I).unsqueeze(1)).any(2)).all()
