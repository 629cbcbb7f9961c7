"""Graph-classification evaluate / infer on the device (models/graph_trainer.py
``infer_logits`` / ``infer_embed``; the fused trainer's forward-only pack kernel,
csrc/hip/graph_cls_infer.hip, through ``GraphClsPlan.infer``).

* the pack kernel's logits and pooled embeddings against the generic CPU trainer run in
  float64 (its outputs rounded to fp32), for request lists that hit every pack mechanism;
* its logits against the training step's own loss; inference leaves the step's bits alone;
* the generic path: chunking, the engine-path ``evaluate()`` loss, unknown labels;
* the estimator: ``evaluate()`` / ``infer()`` without the engine's graph queries.
"""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_graph_cls_trainer import _est, _train_eps, _trainer

# 8 x the largest max|a - b| / max|b| of the CPU fp32 forward against the float64 one over
# these models and request lists (profiles/graph_infer/oracle_margins.json: embeddings
# 1.79e-7, logits 1.13e-6, from benchmarks/bench_graph_infer.py --margins); floor 1e-6
EMB_TOL, LOGIT_TOL = 1.43e-6, 9.06e-6


def _pair(tmp_path, model):
    """a CUDA fused trainer and a CPU generic one with the same random weights"""
    eps = model == "gin_eps"
    out = []
    for dev in ("cuda", "cpu"):
        _, est = _est(tmp_path, "gin" if eps else model, dev)
        if eps:
            _train_eps(est)
        out.append(_trainer(est))
    tr, trc = out
    with torch.no_grad():
        gen = torch.Generator().manual_seed(5)
        for pc, pg in zip(trc.flat.params, tr.flat.params):
            v = torch.randn(pc.shape, generator=gen) * 0.3
            pc.copy_(v)
            pg.copy_(v.to(pg.device))
    return tr, trc


def _packs(counts, idx, rows, cap=16):
    """the greedy pass of GraphClsPlan.infer: packs of consecutive requests"""
    n, used, k = 0, 0, 0
    for g in idx:
        c = int(counts[g])
        if k == 0 or k == cap or used + c > rows:
            n, used, k = n + 1, 0, 0
        used, k = used + c, k + 1
    return n


def _rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["gin", "gin_eps", "graphgcn"])
@pytest.mark.parametrize("case", ["single", "packs", "one_per_block", "cap16"])
def test_pack_kernel_matches_float64_cpu(tmp_path, cuda, model, case, monkeypatch):
    from euler_amd.models.graph_cls_trainer import GraphClsTrainer

    tr, trc = _pair(tmp_path, model)
    assert isinstance(tr, GraphClsTrainer)
    counts = (trc.gnodes >= 0).sum(1).tolist()
    rows, cap = tr.plan.infer_rows, 16
    if case == "single":
        idx = [5]
    elif case == "cap16":  # the 16-graph cap, not the row cap, closes the first pack
        small = min(range(len(counts)), key=counts.__getitem__)
        if 17 * counts[small] > rows:
            pytest.skip(f"the smallest graph has {counts[small]} nodes: 17 of them exceed {rows} rows")
        idx = [small] * 17
    else:  # several full packs and a partial one; graph 3 at two row offsets
        idx = list(range(14)) + [3]
        if case == "one_per_block":
            monkeypatch.setenv("EULER_AMD_GRAPH_INFER_PACK", "1")
            cap = 1
    idx = torch.tensor(idx)
    g, logits, y = tr.infer_logits(idx)
    npacks = tr.plan.infer_packs
    emb = tr.infer_embed(idx)
    torch.cuda.synchronize()
    assert npacks == _packs(counts, idx.tolist(), rows, cap)
    if case == "packs":
        assert npacks >= 3 and npacks < len(idx)
    assert torch.equal(g.cpu(), idx) and torch.equal(y.cpu(), trc.onehot[idx])
    m64 = copy.deepcopy(trc.model).double()
    trc.model, trc.gnn = m64, m64.gnn
    _, ref_logits, _ = trc.infer_logits(idx)
    ref_emb = trc.infer_embed(idx)
    e_emb, e_log = _rel(emb, ref_emb), _rel(logits, ref_logits)
    print(f"{model} {case}: packs {npacks} emb {e_emb:.3e} logits {e_log:.3e}")
    assert emb.shape == ref_emb.shape and logits.shape == ref_logits.shape
    assert e_emb < EMB_TOL and e_log < LOGIT_TOL, (e_emb, e_log)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["gin", "graphgcn"])
def test_inference_agrees_with_the_step_and_leaves_it_alone(tmp_path, cuda, model):
    tr, _ = _pair(tmp_path, model)
    state = tr.graph.rng.clone()

    def step():
        tr.graph.rng.copy_(state)
        tr.flat.zero_grad()
        tr.forward_backward_only()
        return tr.loss_out.clone(), tr.flat.grad[: tr.flat.numel].clone(), tr.plan.gidx().clone()

    loss0, grad0, drawn = step()
    _, logits, y = tr.infer_logits(drawn)
    assert math.isclose(float(F.binary_cross_entropy_with_logits(logits, y)), float(loss0), rel_tol=1e-5)
    tr.infer_embed(torch.arange(40))
    loss1, grad1, drawn1 = step()
    assert torch.equal(loss0, loss1) and torch.equal(grad0, grad1) and torch.equal(drawn, drawn1)
    g, logits, y = tr.infer_logits(torch.zeros(0, dtype=torch.int64))
    emb = tr.infer_embed([])
    assert tuple(logits.shape) == (0, tr.onehot.shape[1]) and tuple(y.shape) == tuple(logits.shape)
    assert tuple(emb.shape) == (0, tr.gnn.fc.weight.shape[0]) and g.numel() == 0 and tr.plan.infer_packs == 0


def test_generic_infer_chunks_and_engine_evaluate_cpu(tmp_path):
    _, est = _est(tmp_path, "gin", "cpu", steps=6)
    est.train()
    tr = est.device_trainer
    labels = tr.graph_labels_of(torch.arange(tr.onehot.shape[0]))
    _, whole, _ = tr.infer_logits(labels)
    # chunks of B graphs inside one call against calls of 7 (each padded to B)
    parts = [tr.infer_logits(labels[i:i + 7])[1] for i in range(0, len(labels), 7)]
    assert whole.shape == (len(labels), tr.onehot.shape[1])
    np.testing.assert_allclose(torch.cat(parts).numpy(), whole.numpy(), rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError, match="no-such-graph"):
        tr.infer_logits(labels[:2] + ["no-such-graph"])
    ev_d = est.evaluate()
    _, eng = _est(tmp_path, "gin", "cpu", steps=6)  # the same checkpoint and id file, engine path
    eng.params["device_infer"] = False
    ev_e = eng.evaluate()
    assert math.isclose(ev_d["loss"], ev_e["loss"], rel_tol=1e-4), (ev_d, ev_e)
    assert 0.0 <= ev_d["accuracy"] <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["gin", "graphgcn"])
def test_estimator_evaluates_and_infers_without_engine_queries(tmp_path, cuda, model, monkeypatch):
    import euler_amd.ops.graph_api as ge

    _, est = _est(tmp_path, model, "cuda")
    est.train()
    assert type(est.device_trainer).__name__ == "GraphClsTrainer"

    def boom(*a, **k):
        raise AssertionError("get_graph_by_label on the device path")

    monkeypatch.setattr(ge, "get_graph_by_label", boom)
    ev = est.evaluate()
    assert math.isfinite(ev["loss"]) and 0.0 <= ev["accuracy"] <= 1.0
    ids, emb = est.infer()
    want = [s for b in est.get_input_from_id_file() for s in b]
    assert [str(s) for s in ids] == want and len(want) > est.params["batch_size"]
    ref = est.device_trainer.infer_embed(want)
    assert emb.shape == (len(want), ref.shape[1]) and np.array_equal(emb, ref.cpu().numpy())
