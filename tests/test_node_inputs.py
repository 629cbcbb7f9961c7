"""Sparse-feature and id-embedding encoder inputs on the device path (graph/device_graph.py
``DeviceGraph.sparse``, ops/mp_ops.py ``node_bag``, models/node_inputs.py), CPU side: the
sparse columns uploaded as CSR equal the engine's lists; the pure-torch twin of the
node-row embedding-bag kernels equals ``ShallowEncoder.forward`` on the raw ids for every
embedding layer, both combiners, with and without a dense column; GeniePath's device-path
logits equal the engine path's; the estimator trains / resumes such models with
``device_graph=True`` (it refused them before) and stays in lockstep over two ranks; the
datasets that existed before ``cora_sparse`` generate the same graphs."""
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cora_sparse(tmp_path_factory):
    from euler_amd.dataset import get_dataset

    return get_dataset("cora_sparse", data_dir=str(tmp_path_factory.mktemp("cora_sparse")), scale=0.05)


def _graph(ds, dense=True, sparse=True, label=True):
    from euler_amd.graph.device_graph import DeviceGraph

    kw = dict(label="label", label_dim=ds.label_dim) if label else {}
    if dense:
        kw.update(features=["feature"], feature_dims=[ds.feature_dim])
    return DeviceGraph.from_engine(feature_dtype=torch.float32, sparse_features=["words"] if sparse else (), seed=5,
                                   device="cpu", **kw)


# ----------------------------------------------------------------------------- 1. CSR upload
@pytest.mark.parametrize("mode", ["local", "local_sharded"])
def test_sparse_columns_upload_as_csr(tmp_path, monkeypatch, mode):
    """from_engine(sparse_features=[f1, f2]) on the 6-node fixture: every node's CSR segment
    is the engine's id list (a node without the feature: an empty segment, where the
    engine's query without defaults fills a single 0); the ids are fetched in chunks"""
    import euler_amd as ea
    from euler_amd.graph import device_graph as dg
    from euler_amd.tools.converter import convert_json

    d = str(tmp_path / "g")
    convert_json(os.path.join(HERE, "data", "graph.json"), d, 2, os.path.join(HERE, "data", "index_meta.json"))
    if mode == "local":
        ea.initialize_embedded_graph(d)
    else:
        ea.initialize_graph({"mode": "local_sharded", "data_path": d, "shard_num": 2})
    monkeypatch.setattr(dg, "_SPARSE_CHUNK", 4)  # two chunks over 6 nodes
    g = dg.DeviceGraph.from_engine(sparse_features=["f1", "f2"], device="cpu")
    assert sorted(g.sparse) == ["f1", "f2"] and g.num_rows == 6
    ids = np.asarray(g.ids).astype(np.int64)
    total = 0
    for name in ("f1", "f2"):
        indptr, values = g.sparse[name]
        assert indptr.dtype == torch.int64 and values.dtype == torch.int64 and indptr.numel() == 7
        assert int(indptr[0]) == 0 and int(indptr[-1]) == values.numel()
        for r, i in enumerate(ids.tolist()):
            want = ea.get_sparse_feature([i], [name])[0].values.to(torch.int64).tolist()
            got = values[int(indptr[r]): int(indptr[r + 1])].tolist()
            assert got == want or (got == [] and want == [0]), (name, i, got, want)
            total += len(got)
    assert total > 0
    assert dg.DeviceGraph.from_engine(device="cpu").sparse == {}


# ----------------------------------------------------------------------------- 2. twin vs layers
def _rows_and_raw(g, ds):
    """rows with duplicates, -1 (the default node) and the nodes without words; their raw
    ids with the engine's default node max_id + 1 for -1"""
    ids = np.asarray(g.ids).astype(np.int64)
    rows = torch.tensor([0, 15, 3, -1, 31, 15, g.num_rows - 1, 7, -1, 47, 2], dtype=torch.long)
    raw = torch.where(rows >= 0, torch.as_tensor(ids)[rows.clamp(min=0)], torch.tensor(ds.max_node_id + 1))
    return rows, raw


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("combiner", ["concat", "add"])
@pytest.mark.parametrize("kind", ["embedding", "hash_embedding", "sparse_sum", "sparse_mean", "hash_sparse"])
def test_device_node_inputs_equal_shallow_encoder(cora_sparse, kind, combiner, dense):
    from euler_amd.models.node_inputs import DeviceNodeInputs
    from euler_amd.utils.encoders import ShallowEncoder
    from euler_amd.utils.layers import Embedding, HashEmbedding, HashSparseEmbedding, SparseEmbedding

    ds = cora_sparse
    ds.load_graph()
    g = _graph(ds)
    lens = (g.sparse["words"][0][1:] - g.sparse["words"][0][:-1])
    assert int((lens == 0).sum()) >= 2 and int(lens[15]) == 0 and int(lens[0]) > 1
    torch.manual_seed(3)
    kw = dict(feature_idx="feature" if dense else -1, feature_dim=ds.feature_dim if dense else 0,
              embedding_dim=16, use_hash_embedding=kind.startswith("hash"), combiner=combiner,
              dim=8 if combiner == "add" else None)
    if kind in ("embedding", "hash_embedding"):
        kw.update(max_id=ds.max_node_id)
    else:
        kw.update(sparse_feature_idx="words", sparse_feature_max_id=ds.sparse_fea_max_id)
    ne = ShallowEncoder(**kw)
    want_cls = {"embedding": Embedding, "hash_embedding": HashEmbedding, "sparse_sum": SparseEmbedding,
                "sparse_mean": SparseEmbedding, "hash_sparse": HashSparseEmbedding}[kind]
    layer = ne.embedding if ne.use_id else ne.sparse_embeddings[0]
    assert type(layer) is want_cls
    if kind == "sparse_mean":
        layer.combiner = "mean"
    with torch.no_grad():
        layer.weight.normal_(0.0, 0.5)  # the default initialisation (std 2e-4) would hide a wrong row
    rows, raw = _rows_and_raw(g, ds)
    with torch.no_grad():
        want = ne(raw)  # also materialises the lazy dense projection
        got = DeviceNodeInputs(ne, g)(rows)
    assert got.shape == (rows.numel(), ne.output_dim)
    assert torch.allclose(got, want, atol=1e-6, rtol=1e-6), float((got - want).abs().max())


def test_device_node_inputs_gradients_reach_the_tables(cora_sparse):
    """concat of id + dense + two sparse columns filled in one buffer: values and the table /
    projection gradients equal the engine path's autograd"""
    from euler_amd.models.node_inputs import DeviceNodeInputs
    from euler_amd.utils.encoders import ShallowEncoder

    ds = cora_sparse
    ds.load_graph()
    g = _graph(ds)
    torch.manual_seed(4)
    ne = ShallowEncoder(dim=12, feature_idx="feature", feature_dim=ds.feature_dim, max_id=ds.max_node_id,
                        sparse_feature_idx=["words", "words"], sparse_feature_max_id=[ds.sparse_fea_max_id] * 2,
                        embedding_dim=[16, 20, 8], use_hash_embedding=[False, False, True], combiner="concat")
    ne.sparse_embeddings[0].combiner = "mean"
    with torch.no_grad():
        for t in [ne.embedding] + list(ne.sparse_embeddings):
            t.weight.normal_(0.0, 0.5)
    rows, raw = _rows_and_raw(g, ds)
    w = torch.randn(rows.numel(), 12, generator=torch.Generator().manual_seed(1))
    (ne(raw) * w).sum().backward()
    ref = {n: p.grad.clone() for n, p in ne.named_parameters()}
    ne.zero_grad(set_to_none=True)
    (DeviceNodeInputs(ne, g)(rows) * w).sum().backward()
    for n, p in ne.named_parameters():
        assert torch.allclose(p.grad, ref[n], atol=1e-5, rtol=1e-5), n


def test_device_node_inputs_validate_at_construction(cora_sparse):
    from euler_amd.models.node_inputs import DeviceNodeInputs
    from euler_amd.utils.encoders import ShallowEncoder

    ds = cora_sparse
    ds.load_graph()
    ne = ShallowEncoder(feature_idx=-1, sparse_feature_idx="words", sparse_feature_max_id=ds.sparse_fea_max_id)
    with pytest.raises(ValueError, match="no sparse feature"):
        DeviceNodeInputs(ne, _graph(ds, sparse=False))
    g = _graph(ds)
    ne.sparse_embeddings[0].weight.data = ne.sparse_embeddings[0].weight.data.double()
    with pytest.raises(ValueError, match="fp32"):
        DeviceNodeInputs(ne, g)
    big = ShallowEncoder(feature_idx=-1, max_id=(1 << 20) - 2, embedding_dim=1)
    with pytest.raises(ValueError, match="2\\^20"):
        DeviceNodeInputs(big, g)


# ----------------------------------------------------------------------------- 3. encoder parity
@pytest.mark.parametrize("config", ["sparse", "id", "dense_sparse_id_residual"])
def test_geniepath_device_logits_equal_engine_path(cora_sparse, config):
    """EncoderFlowTrainer._forward = m.out_fc(m.embed(raw ids)) for GeniePath over sparse /
    id / mixed inputs (the pattern and tolerance of the dense-feature parity test)"""
    from euler_amd import models as Z
    from euler_amd.models.encoder_trainer import EncoderFlowTrainer

    ds = cora_sparse
    ds.load_graph()
    sp = dict(sparse_feature_idx=ds.sparse_fea_idx, sparse_feature_max_id=ds.sparse_fea_max_id)
    dense = dict(feature_idx=ds.feature_idx, feature_dim=ds.feature_dim)
    kw = {"sparse": sp, "id": dict(use_id=True),
          "dense_sparse_id_residual": dict(use_id=True, use_residual=True, **sp, **dense)}[config]
    torch.manual_seed(0)
    m = Z.GeniePath(16, [["train"], ["train"]], ds.label_idx, ds.label_dim, max_id=ds.max_node_id, head_num=1, **kw)
    ne = m._encoder._node_encoder
    with torch.no_grad():
        for t in ([ne.embedding] if ne.use_id else []) + (list(ne.sparse_embeddings) if ne.use_sparse_feature else []):
            t.weight.normal_(0.0, 0.5)
    g = _graph(ds, dense="dense" in config, sparse="sparse" in config)
    assert (g.features is None) == ("dense" not in config)
    roots = torch.randint(0, g.num_rows, (8,), generator=torch.Generator().manual_seed(2))
    roots[1] = 15  # a node without words
    raw = torch.as_tensor(np.asarray(g.ids)[roots.numpy()].astype(np.int64))
    m.eval()
    with torch.no_grad():
        m.out_fc(m.embed(raw))  # materialises the lazy layers
        tr = EncoderFlowTrainer.from_model(m, g, 8)
        dev, _ = tr._forward(roots)
        eng = m.out_fc(m.embed(raw)).float()
    assert torch.allclose(dev, eng, atol=1e-4, rtol=1e-4), float((dev - eng).abs().max())


# ----------------------------------------------------------------------------- 4. estimator
def _base(tmp_path, extra=()):
    return ["--dataset", "cora_sparse", "--scale", "0.05", "--batch_size", "16", "--log_steps", "3", "--device", "cpu",
            "--seed", "1", "--model_dir", str(tmp_path / "ckpt"), "--data_dir", str(tmp_path / "data"),
            "--learning_rate", "0.01", "--device_feature_dtype", "fp32"] + list(extra)


@pytest.mark.parametrize("model,kind,flags", [("geniepath", "encoder_flow", ["--use_sparse_feature"]),
                                              ("dgi", "dgi", ["--use_sparse_feature"]),
                                              ("geniepath", "encoder_flow", ["--use_sparse_feature", "--use_id"])])
def test_estimator_trains_sparse_inputs_on_the_device_path(tmp_path, monkeypatch, model, kind, flags):
    monkeypatch.chdir(tmp_path)
    from euler_amd.tools import runner

    base = _base(tmp_path, ["--device_graph"] + flags)
    r1 = runner.main(base + ["--total_step", "6"], model=model)
    assert r1["step"] == 6 and math.isfinite(r1["loss"])
    a = runner.parse_args(base + ["--total_step", "9"], model=model)
    m, est = runner.build(a)
    r2 = est.train()  # resumes from the checkpoint of step 6
    assert r2["step"] == 9 and math.isfinite(r2["loss"])
    assert est.device_trainer.device_trainer_kind == kind
    st = torch.load(str(tmp_path / "ckpt" / "model.ckpt-9.pt"), weights_only=True)
    assert st["device_trainer"]["step"] == 9
    ne = (m._encoder if model == "geniepath" else m._target_encoder)._node_encoder
    assert ne.use_sparse_feature and ne.use_id == ("--use_id" in flags)
    if model != "geniepath":
        return
    # the trained weights give the same logits on the device and on the engine path, and
    # evaluate() with and without device_graph reports the same numbers from the checkpoint
    tr = est.device_trainer
    g = tr.graph
    rows = torch.arange(g.num_rows - 12, g.num_rows)
    raw = torch.as_tensor(np.asarray(g.ids)[rows.numpy()].astype(np.int64))
    m.eval()
    with torch.no_grad():
        dev, _ = EncoderInfer(tr)(rows)
        eng = m.out_fc(m.embed(raw)).float()
    m.train()
    assert torch.allclose(dev, eng, atol=1e-4, rtol=1e-4)
    ev_dev = runner.main(base + ["--run_mode", "evaluate"], model=model)
    ev_eng = runner.main(_base(tmp_path, flags) + ["--run_mode", "evaluate"], model=model)
    assert math.isfinite(ev_dev["loss"])
    assert abs(ev_dev["loss"] - ev_eng["loss"]) <= 1e-4 and abs(ev_dev["f1"] - ev_eng["f1"]) <= 1e-4


class EncoderInfer:
    """the trainer's forward over exactly the given rows (a flow of their count)"""

    def __init__(self, tr):
        self.tr = tr

    def __call__(self, rows):
        from euler_amd.dataflow.device_flow import DeviceFullFlow

        tr = self.tr
        keep = tr.flow
        tr.flow = DeviceFullFlow(tr.graph, keep.masks, int(rows.numel()), False, "exact")
        try:
            return tr._forward(rows)
        finally:
            tr.flow = keep


@pytest.mark.parametrize("kind", ["supervise", "unsupervise"])
def test_solution_trainers_take_sparse_and_id_inputs(cora_sparse, tmp_path, kind):
    """the solution API over SageEncoders without any dense column (sparse bag + id
    embedding) trains on the device path; the hop inputs equal the engine's for the same
    tree, the samplers' -1 read as the engine's default node max_id + 1"""
    from euler_amd import solution as S
    from euler_amd.estimator import NodeEstimator
    from euler_amd.utils import encoders as E

    ds = cora_sparse
    ds.load_graph()
    torch.manual_seed(0)
    mk = lambda: E.SageEncoder([["train"], ["train"]], [3, 2], 8, feature_idx=-1, use_id=True,  # noqa: E731
                               max_id=ds.max_node_id, sparse_feature_idx="words",
                               sparse_feature_max_id=ds.sparse_fea_max_id, embedding_dim=[4, 16])
    if kind == "supervise":
        m = S.SuperviseSolution(S.GetLabelFromFea("label", ds.label_dim), mk(), S.DenseLogits(ds.label_dim))
    else:
        m = S.UnsuperviseSolution(mk(), mk(), S.SamplePosWithTypes(["train"], 1, ds.max_node_id),
                                  S.SampleNegWithTypes("train", 3))
    p = {"model_dir": str(tmp_path / "ckpt"), "batch_size": 16, "total_step": 6, "optimizer": "adam",
         "learning_rate": 0.01, "log_steps": 3, "train_node_type": "train", "device": "cpu", "device_graph": True,
         "seed": 5, "device_feature_dtype": "fp32"}
    est = NodeEstimator(m, p)
    res = est.train()
    tr = est.device_trainer
    assert res["step"] == 6 and math.isfinite(res["loss"])
    assert type(tr).__name__ == {"supervise": "SolutionTrainer", "unsupervise": "UnsupSolutionTrainer"}[kind]
    assert tr.graph.features is None and "words" in tr.graph.sparse
    enc, inputs = (m.encoder, tr.inputs) if kind == "supervise" else (m.target_encoder, tr.t_inputs)
    rows = torch.tensor([0, 15, -1, 4, 15, -1])
    ids = torch.as_tensor(np.asarray(tr.graph.ids).astype(np.int64))
    raw = torch.where(rows >= 0, ids[rows.clamp(min=0)], torch.tensor(ds.max_node_id + 1))
    with torch.no_grad():
        assert torch.allclose(inputs(rows), enc.node_encoder(raw), atol=1e-6, rtol=1e-6)


def test_runner_flags_are_limited_to_the_encoder_models(tmp_path):
    from euler_amd.tools import runner

    with pytest.raises(SystemExit):
        runner.main(_base(tmp_path, ["--use_id", "--total_step", "1"]), model="gcn")
    with pytest.raises(SystemExit):  # cora has no sparse feature
        runner.main(["--dataset", "cora", "--scale", "0.05", "--device", "cpu", "--use_sparse_feature",
                     "--data_dir", str(tmp_path / "cora"), "--model_dir", str(tmp_path / "c"), "--total_step", "1"],
                    model="geniepath")


def test_sharded_device_graph_keeps_refusing_sparse_inputs(tmp_path):
    from euler_amd.estimator.device_trainers import NoDeviceTrainer
    from euler_amd.tools import runner

    with pytest.raises((NoDeviceTrainer, ValueError)):
        runner.main(_base(tmp_path, ["--device_graph_sharded", "--use_sparse_feature", "--total_step", "2"]),
                    model="geniepath")


# ----------------------------------------------------------------------------- 5. datasets
# sha256 of json.dumps({"nodes", "edges"}, sort_keys=True) of Cora(scale=0.05).synthesize(
# default_rng(0)), recorded from the generator before the extra-feature hook existed
_CORA_005_SHA256 = "78004783bf712d03262f87ab239aff8b078a1a9bda995e366e17d808288227d2"


def test_existing_citation_generator_is_unchanged(tmp_path):
    from euler_amd.dataset import get_dataset

    ds = get_dataset("cora", data_dir=str(tmp_path / "cora"), scale=0.05)
    os.makedirs(ds.data_dir, exist_ok=True)
    data = ds.synthesize(np.random.default_rng(0))
    s = json.dumps({"nodes": data["nodes"], "edges": data["edges"]}, sort_keys=True)
    assert (len(data["nodes"]), len(data["edges"])) == (135, 506)
    assert hashlib.sha256(s.encode()).hexdigest() == _CORA_005_SHA256
    # cora_sparse: the same graph plus the words column (absent on every 16th node)
    sp = get_dataset("cora_sparse", data_dir=str(tmp_path / "cs"), scale=0.05)
    os.makedirs(sp.data_dir, exist_ok=True)
    d2 = sp.synthesize(np.random.default_rng(0))
    assert d2["edges"] == data["edges"]
    for a, b in zip(data["nodes"], d2["nodes"]):
        extra = b["features"][len(a["features"]):]
        assert b["features"][:len(a["features"])] == a["features"] and len(extra) == (0 if a["id"] % 16 == 15 else 1)
        if extra:
            dense = np.asarray(a["features"][1]["value"])
            assert extra[0]["name"] == "words" and extra[0]["value"] == np.flatnonzero(dense).tolist()
    assert sp.sparse_fea_idx == "words" and sp.sparse_fea_max_id == sp.feature_dim - 1


# ----------------------------------------------------------------------------- 6. lockstep
def _worker_sparse_geniepath_dp(rank, world, port, q, tmp):
    """the sparse GeniePath configuration under 2 gloo ranks: the sparse columns cross the
    shared export, per-rank sample streams, the flat gradient (tables included) summed every
    step -> bit-identical parameters on every rank after 3 steps"""
    try:
        import torch.distributed as dist
        from test_parallel import _init

        _init(rank, world, port)
        from euler_amd.tools import runner

        a = runner.parse_args(["--dataset", "cora_sparse", "--scale", "0.05", "--batch_size", "16", "--total_step", "3",
                               "--log_steps", "1", "--data_dir", os.path.join(tmp, "data"), "--model_dir",
                               os.path.join(tmp, f"ckpt_r{rank}"), "--device_graph", "--device", "cpu", "--seed", "1",
                               "--use_sparse_feature", "--use_id"], model="geniepath")
        _, est = runner.build(a)
        est.train()
        tr = est.device_trainer
        p = tr.logical_params()
        flat = torch.cat([p[k].reshape(-1).float() for k in sorted(p)])
        allp = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(allp, flat)
        same = all(torch.equal(x, allp[0]) for x in allp)
        mine = torch.cat([t.reshape(-1).long() for t in tr.samples()])
        got = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(got, mine)
        drew = not all(torch.equal(x, got[0]) for x in got)
        tables = any("sparse_embeddings" in k for k in p) and any(k.endswith("embedding.weight") for k in p)
        ok = same and drew and tables and type(tr).__name__ == "EncoderFlowTrainer" and "words" in tr.graph.sparse \
            and bool(torch.isfinite(flat).all())
        q.put((rank, "sparse_geniepath_dp", bool(ok), same, drew, tables))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "error", traceback.format_exc()))


def test_sparse_geniepath_data_parallel_lockstep(tmp_path):
    from test_parallel import _run

    res = _run(_worker_sparse_geniepath_dp, str(tmp_path))
    assert not [r for r in res if r[1] == "error"], res
    assert len(res) == 2 and all(r[2] for r in res), res
