"""Frontier inference (models/sage_infer.py ``mode="frontier"``, SageTrainer.infer_*_frontier,
estimator ``infer_mode="frontier"``): exact layer-wise GraphSAGE embeddings computed over only
the rows a request reaches.  The reference is the all-rows layer-wise path of the same object:
equal bits on the GPU (the same kernel code over a compact table), 1e-6 on the CPU (the fp32
composition with remapped indices).  CPU tests are unmarked, their GPU twins are ``gpu``.
"""
import numpy as np
import pytest
import torch

from test_frontier_kernels import np_closure
from test_sage_infer import N, _IDS, _ROWS, _counted, _estimator, model_case, one_edge_case


def _same(got, want, device):
    assert got.dtype == want.dtype and got.shape == want.shape
    if str(device).startswith("cuda"):
        return torch.equal(got, want)
    return torch.allclose(got, want, rtol=1e-6, atol=1e-6)


def np_sizes(csr, T, masks, rows):
    """|I_k|, k = 1 .. L - 1, of the numpy closures: I_k = T_k ∪ N(T_k) under hop L - 1 - k's
    mask, T_{L-1} = rows, T_{k-1} = I_k"""
    L = len(masks)
    sizes, targets = [], np.asarray(rows)
    for k in range(L - 1, 0, -1):
        targets = np_closure(csr, T, N, targets, masks[L - 1 - k])
        sizes.insert(0, len(targets))
    return sizes


# ----------------------------------------------------------------------------------------- model


def _frontier_equals_all_rows(device, L, self_loops):
    csr, _, tr = model_case(0, L, self_loops, device)
    rows = torch.tensor(_ROWS)
    lw = tr.layerwise()
    assert lw.last_frontier is None and 0.0 < lw.frontier_max_fraction <= 1.0
    lw.frontier_max_fraction = 1.0  # 7 rows reach most of a 200-row graph in 3 hops: the fallback has its own test
    emb = lw.embed(rows, mode="frontier")
    assert lw._hidden is None  # a frontier call neither makes nor reads the all-rows table
    assert lw.last_frontier == {"sizes": np_sizes(csr, 2, tr.masks, _ROWS), "fallback": False}
    assert len(lw.last_frontier["sizes"]) == L - 1
    emb2, logits = lw.logits(rows, mode="frontier")
    h = lw.last_conv(rows, mode="frontier")
    assert lw._hidden is None
    assert _same(emb, lw.embed(rows), device) and torch.equal(emb, emb2)
    want_emb, want_logits = lw.logits(rows)
    assert _same(logits, want_logits, device) and _same(emb2, want_emb, device)
    assert _same(h, lw.last_conv(rows), device)
    with pytest.raises(ValueError, match="frontier"):
        lw.embed(None, mode="frontier")
    with pytest.raises(ValueError, match="mode"):
        lw.embed(rows, mode="sampled")


@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_frontier_equals_all_rows_cpu(L, self_loops):
    _frontier_equals_all_rows("cpu", L, self_loops)


@pytest.mark.gpu
@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_frontier_equals_all_rows_gpu(cuda, L, self_loops):
    _frontier_equals_all_rows(cuda, L, self_loops)


def _plan_outlives_a_step(device):
    """the plan depends on the graph, the masks and the rows only: reused after a step it
    gives the new parameters' all-rows result"""
    from euler_amd.models.sage_infer import FrontierPlan

    _, _, tr = model_case(1, 3, True, device)
    rows = torch.tensor(_ROWS)
    tr.layerwise().frontier_max_fraction = 1.0  # 7 rows reach most of a 200-row graph in 3 hops: no fallback here
    plan = FrontierPlan(tr.layerwise(), rows)
    assert plan.complete and len(plan.sets) == 2
    e0 = tr.layerwise().embed(rows, mode="frontier", plan=plan).clone()
    tr.step()
    lw = tr.layerwise()
    e1 = lw.embed(rows, mode="frontier", plan=plan)
    assert lw._hidden is None
    assert not torch.equal(e0, e1) and _same(e1, lw.embed(rows), device)
    with pytest.raises(ValueError, match="plan"):
        lw.embed(torch.tensor(_ROWS[:3]), mode="frontier", plan=plan)


def test_plan_outlives_a_step_cpu():
    _plan_outlives_a_step("cpu")


@pytest.mark.gpu
def test_plan_outlives_a_step_gpu(cuda):
    _plan_outlives_a_step(cuda)


def _fallback(device):
    """a set above frontier_max_fraction of the graph: the all-rows passes (and their cache)
    answer, with the same result"""
    _, _, tr = model_case(0, 3, False, device)
    rows = torch.tensor(_ROWS)
    lw = tr.layerwise()
    lw.frontier_max_fraction = 1.0
    want = lw.embed(rows, mode="frontier").clone()
    assert lw.last_frontier["fallback"] is False and lw._hidden is None
    lw.frontier_max_fraction = 0.0
    got = lw.embed(rows, mode="frontier")
    assert lw.last_frontier["fallback"] is True and lw.last_frontier["sizes"]
    assert lw._hidden is not None  # the fallback keeps the all-rows cache
    assert _same(got, want, device) and _same(got, lw.embed(rows), device)


def test_fallback_cpu():
    _fallback("cpu")


@pytest.mark.gpu
def test_fallback_gpu(cuda):
    _fallback(cuda)


def _one_edge_graph(device, self_loops):
    tr = one_edge_case(0, self_loops, device)
    tr.layerwise().frontier_max_fraction = 1.0
    emb_l, logits_l, y_l = tr.infer_logits_layerwise(_IDS)
    emb_f, logits_f, y_f = tr.infer_logits_frontier(_IDS)
    assert tr.layerwise().last_frontier["fallback"] is False
    assert _same(emb_f, emb_l, device) and _same(logits_f, logits_l, device) and torch.equal(y_f, y_l)
    assert torch.equal(tr.infer_embed_frontier(_IDS), emb_f)


@pytest.mark.parametrize("self_loops", [False, True])
def test_frontier_on_one_edge_graph_cpu(self_loops):
    _one_edge_graph("cpu", self_loops)


@pytest.mark.gpu
@pytest.mark.parametrize("self_loops", [False, True])
def test_frontier_on_one_edge_graph_gpu(cuda, self_loops):
    _one_edge_graph(cuda, self_loops)


# ----------------------------------------------------------------------------------------- estimator


def _estimator_frontier(tmp_path, device):
    est = _estimator(tmp_path, device, extra=["--infer_mode", "frontier"])
    assert est.params["infer_mode"] == "frontier"
    est.train()
    tr = est.device_trainer
    tr.layerwise().frontier_max_fraction = 1.0  # the frontier path itself, whatever the batches reach
    hidden_calls = _counted(tr.layerwise(), "hidden")
    f_calls, s_calls = _counted(tr, "infer_embed_frontier"), _counted(tr, "infer_embed")
    ids, embs = est.infer()
    inf = tmp_path / "inf"
    f_emb, f_ids = np.load(inf / "embedding_0.npy"), np.load(inf / "ids_0.npy")
    assert np.array_equal(f_ids, ids) and np.array_equal(f_emb, embs) and len(ids) > 0
    ev = est.evaluate()
    assert f_calls and not s_calls and not hidden_calls  # the all-rows table is never asked for
    assert tr.layerwise().last_frontier["fallback"] is False
    assert np.isfinite(ev["loss"]) and len(ev) == 2
    # the same checkpoint through the layer-wise mode: the same files, the same metrics
    est.params["infer_mode"] = "layerwise"
    l_ids, l_embs = est.infer()
    assert hidden_calls
    assert np.array_equal(np.load(inf / "ids_0.npy"), f_ids) and np.array_equal(l_ids, ids)
    if device == "cuda":
        assert np.array_equal(np.load(inf / "embedding_0.npy"), f_emb)
        assert est.evaluate() == ev
    else:
        assert np.allclose(np.load(inf / "embedding_0.npy"), f_emb, rtol=1e-6, atol=1e-6)
        lev = est.evaluate()
        assert set(lev) == set(ev) and all(abs(lev[k] - ev[k]) <= 1e-6 for k in ev)
    est.params["infer_mode"] = "treewise"
    with pytest.raises(ValueError, match="infer_mode"):
        est.infer()


def test_estimator_infer_mode_frontier_cpu(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _estimator_frontier(tmp_path, "cpu")


@pytest.mark.gpu
def test_estimator_infer_mode_frontier_gpu(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _estimator_frontier(tmp_path, "cuda")


def test_estimator_frontier_refuses_gcn(tmp_path, monkeypatch):
    """never a fall back to sampled or engine-path inference: a ValueError names the reason"""
    monkeypatch.chdir(tmp_path)
    est = _estimator(tmp_path, "cpu", model="gcn", extra=["--infer_mode", "frontier"])
    with pytest.raises(ValueError, match="'frontier'.*layer-wise"):
        est.infer()
    with pytest.raises(ValueError, match="'frontier'.*layer-wise"):
        est.evaluate()
    est.params["device_graph"] = False
    with pytest.raises(ValueError, match="'frontier'.*device_graph"):
        est.infer()


def test_sharded_trainer_has_no_frontier():
    from euler_amd.models.sharded_sage import ShardedSageTrainer

    assert ShardedSageTrainer.infer_logits_frontier is None and ShardedSageTrainer.infer_embed_frontier is None


def test_runner_accepts_the_mode():
    from euler_amd.tools.runner import parse_args

    a = parse_args(["--dataset", "ppi", "--infer_mode", "frontier"], "graphsage")
    assert a.infer_mode == "frontier"
    with pytest.raises(SystemExit):
        parse_args(["--dataset", "ppi", "--infer_mode", "treewise"], "graphsage")
