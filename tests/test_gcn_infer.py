"""Layer-wise full-neighbourhood inference of the fused GCN family (models/gcn_infer.py) through
GcnTrainer and the estimator: against today's exact-block inference with every node a root
(then the in-block source counts are the graph's own and the two compute the same function),
batch independence, FastGCN / AdaptiveGCN on the device, and ``infer_mode`` of the estimator.
"""
import numpy as np
import pytest
import torch

from test_gcn_csr_kernels import adjacency, dense_layer
from test_gcn_trainer import _graph, _materialize, _setup, _setup_fast
from test_sage_csr_kernels import REL, bf, check_abc
from test_sage_infer import _estimator

# Layer-wise computes on bf16 tables and bf16 weight images, infer_logits in fp32 on the model's
# own modules: their difference is the cost of bf16 over the whole model.  (c)'s absolute term =
# 4 x the largest excess max(|lw - s| - 2^-7 |s|) of the embeddings over L = 1, 2 and init seeds
# 0..4 on an MI355X (profiles/gcn_infer/oracle_margins.json, "layerwise_vs_block").
# Measured: 3.093e-4 (largest |lw - s| 5.1e-4 on embeddings of magnitude ~0.1; RMS ratio of
# layer-wise against its own bf16-aware oracle, in units of that difference: at most 0.021).
# The logits (out_fc of the embeddings) are checked the same way with their own measured excess
# ("logits_excess" of the same records).
MEASURED_BLOCK_EXCESS = 0.0003092503466177732
MEASURED_BLOCK_LOGITS_EXCESS = 0.00041432000580243766  # on logits of magnitude ~0.1; RMS ratio at most 0.027
ATOL_BLOCK = 4.0 * MEASURED_BLOCK_EXCESS
ATOL_BLOCK_LOGITS = 4.0 * MEASURED_BLOCK_LOGITS_EXCESS


def trainer(layers=2, model=None, seed=0):
    from euler_amd.models.gcn_trainer import GcnTrainer

    m = (_setup("cuda", layers=layers) if model is None else _setup_fast("cuda", model=model)).to("cuda")
    g = _graph(m, "cuda")
    torch.manual_seed(seed)
    _materialize(m, g, 64)
    return GcnTrainer.from_model(m, g, 64, caps="exact")


def all_ids(tr):
    n = tr.graph.num_rows
    return np.arange(n) if tr.graph.ids is None else np.asarray(tr.graph.ids)


def dense_model(tr, rounded):
    """fp32 embeddings of every node from dense adjacencies and the model's parameters;
    ``rounded``: bf16 weights, tables and A operands as the GPU path"""
    g, L = tr.graph, len(tr.gnn.convs)
    csr = (g.indptr.cpu().numpy(), g.nbr.cpu().numpy(), None)
    rnd = bf if rounded else (lambda t: t)
    sl = int(bool(tr.gnn.sampler.add_self_loops))
    seg = np.diff(csr[0]).reshape(g.num_rows, g.num_types)
    norm = lambda d: (d.double() + sl).clamp(min=1).rsqrt() * (d + sl > 0)  # noqa: E731  (deg + self)^-1/2, 0 at 0
    ops = []
    for k in range(L):
        mask = tr.masks[L - 1 - k]
        A = adjacency(csr, g.num_types, mask)
        deg_t = torch.from_numpy((seg * [(mask >> t) & 1 for t in range(g.num_types)]).sum(1))
        ops.append((A, norm(deg_t), norm(A.sum(0))))
    h = tr.features[:, : tr.D].float().cpu()
    for k, (A, a, b) in enumerate(ops):
        W = rnd(tr.gnn.convs[k].fc.weight.detach().float().cpu())
        h = dense_layer(A, h, W, a, b if k == 0 else None, ops[k + 1][2] if k < L - 1 else None, sl, True,
                        rounded).float()
    emb = h @ rnd(tr.gnn.fc.weight.detach().float().cpu()).t() + tr.gnn.fc.bias.detach().float().cpu()
    return emb, rnd(emb) @ rnd(tr.model.out_fc.weight.detach().float().cpu()).t()  # gemm rounds its fp32 operand


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2])
def test_layerwise_equals_one_block_over_all_nodes(L):
    tr = trainer(L)
    ids = all_ids(tr)
    emb_s, logits_s, y_s = tr.infer_logits(ids)
    emb_l, logits_l, y_l = tr.infer_logits_layerwise(ids)
    assert emb_l.dtype == torch.float32 and emb_l.shape == emb_s.shape and logits_l.shape == logits_s.shape
    assert torch.equal(y_l, y_s)
    # (a): layer-wise is as close to its bf16-aware oracle as the kernel tests demand, measured in
    # units of what bf16 costs against the fp32 block path; (c): per element against infer_logits
    for what, lw, oracle, s, atol in zip(("emb", "logits"), (emb_l, logits_l), dense_model(tr, True),
                                         (emb_s, logits_s), (ATOL_BLOCK, ATOL_BLOCK_LOGITS)):
        check_abc(lw, oracle, s, float("inf"), f"gcn model {what} L={L}", exact_share=False)
        d = (lw - s).abs()
        excess = float((d - REL * s.abs()).clamp(min=0).max())
        print(f"[gcn block {what} L={L}] max |diff| {float(d.max()):.3e}  (c) excess {excess:.3e}  atol {atol:.3e}")
        assert excess <= atol, (what, excess, atol)


@pytest.mark.gpu
def test_batch_independent():
    tr = trainer(2)
    ids = all_ids(tr)
    pick = np.random.default_rng(0).choice(len(ids), 50, replace=False)
    every, some = tr.infer_logits_layerwise(ids), tr.infer_logits_layerwise(ids[pick])
    for a, s in zip(every, some):
        assert torch.equal(a[torch.from_numpy(pick).to(a.device)], s)
    assert torch.equal(tr.infer_embed_layerwise(ids[pick]), some[0])
    # today's block inference normalises with in-block counts: its rows move with the batch
    assert not torch.equal(tr.infer_logits(ids)[0][torch.from_numpy(pick).to("cuda")], tr.infer_logits(ids[pick])[0])
    table = tr.layerwise().hidden()
    assert tr.layerwise().hidden() is table  # cached while the parameters stand
    tr.step()
    assert tr.layerwise().hidden() is not table and not torch.equal(tr.infer_embed_layerwise(ids[pick]), some[0])


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["fastgcn", "adaptivegcn"])
def test_fastgcn_and_adaptive_infer_on_device(model):
    from euler_amd.models.gcn_infer import LayerwiseGcnInference

    tr = trainer(model=model)
    assert tr.layer_draws is not None
    ids = all_ids(tr)[:300]
    with pytest.raises(NotImplementedError):
        tr.infer_logits(ids)
    emb, logits, y = tr.infer_logits_layerwise(ids)
    assert torch.isfinite(emb).all() and torch.isfinite(logits).all() and float(emb.abs().max()) > 0
    plain = LayerwiseGcnInference(tr.graph, tr.features, [c.fc.weight for c in tr.gnn.convs], tr.masks,
                                  bool(tr.gnn.sampler.add_self_loops), fc=(tr.gnn.fc.weight, tr.gnn.fc.bias),
                                  out_fc=tr.model.out_fc.weight)
    e2, l2 = plain.logits(tr.graph.rows_of(ids))
    assert torch.equal(emb, e2) and torch.equal(logits, l2) and tuple(y.shape) == tuple(logits.shape)


@pytest.mark.gpu
def test_estimator_infer_mode_layerwise_gcn(tmp_path, monkeypatch):
    from euler_amd.models.gcn_trainer import GcnTrainer

    monkeypatch.chdir(tmp_path)
    est = _estimator(tmp_path, "cuda", model="gcn", extra=["--infer_mode", "layerwise"])
    est.train()
    tr = est.device_trainer
    assert isinstance(tr, GcnTrainer)
    ids, embs = est.infer()
    f_emb, f_ids = np.load(tmp_path / "inf" / "embedding_0.npy"), np.load(tmp_path / "inf" / "ids_0.npy")
    assert len(ids) > 0 and np.array_equal(f_ids, ids) and np.array_equal(f_emb, embs)
    assert np.array_equal(f_emb, tr.infer_embed_layerwise(ids).float().cpu().numpy())
    ev = est.evaluate()
    assert np.isfinite(ev["loss"]) and len(ev) == 2 and est.evaluate() == ev
