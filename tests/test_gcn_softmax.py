"""``loss="softmax"`` through the fused GCN step (csrc/hip/gcn_tiles.h gcn_head_kernel<.., softmax>,
models/gcn_trainer.py): the head's softmax cross-entropy against the bf16-aware oracle at the
label widths where the merge of a row's logits tiles can go wrong, large logits, determinism,
the accuracy counts, and the estimator's routing.  Batch 24 = one full 16-row tile + a tail of
8 rows and 8 empty ones; hidden width 32."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

B, HID = 24, 32
# (C, layers, self loops, labels): 5 one tile, mostly padding; 16 exactly one tile; 17 one real
# column in the second tile; 40 one tile per wave, the last all padding; 100 two tiles per wave,
# tile 6 partial, tile 7 all padding.  "dense": non-negative rows whose sum is not 1
CASES = [(5, 1, False, "onehot"), (16, 2, True, "onehot"), (17, 2, False, "onehot"), (40, 1, True, "dense"),
         (100, 2, True, "onehot"), (100, 1, False, "dense")]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(dataset, its device graph with fp32 features) of a 4000-node community graph"""
    from euler_amd.dataset.base import Community
    from euler_amd.graph.device_graph import DeviceGraph

    ds = Community(data_dir=str(tmp_path_factory.mktemp("community")), scale=0.2)
    ds.load_graph()
    g = DeviceGraph.from_engine(features=["feature"], feature_dims=[ds.feature_dim], label="label",
                                label_dim=ds.label_dim, feature_dtype=torch.float32, seed=5, device="cuda")
    return ds, g


def _trainer(world, C, layers=2, self_loops=False, labels="onehot", out_scale=1.0):
    """a GcnTrainer of a softmax GCN with C classes: the graph's 16 community classes spread
    over the C columns (learnable for every C), one-hot or a dense multiple of it plus noise"""
    import euler_amd as ea
    from euler_amd import models as Z
    from euler_amd.models.full_trainer import FullFlowTrainer
    from euler_amd.models.gcn_trainer import GcnTrainer

    ds, base = world
    ds.load_graph()
    ea.set_seed(1)
    torch.manual_seed(0)
    g = copy.copy(base)
    g.manual_seed(5)
    cls = (base.labels.argmax(1) * max(C // 16, 1)) % C
    y = F.one_hot(cls, C).float()
    if labels == "dense":
        y = 2.5 * y + 0.25 * torch.rand(y.shape, generator=torch.Generator().manual_seed(3)).to(y.device)
    g.labels = y
    m = Z.SupervisedGNN("gcn", "full", [HID] * (layers + 1), None, [["train"]] * layers, "feature", ds.feature_dim,
                        "label", C, add_self_loops=self_loops, loss="softmax").to("cuda")
    FullFlowTrainer.from_model(m, g, B, caps="exact")  # materialises the lazy layers
    with torch.no_grad():
        m.out_fc.weight.mul_(out_scale)
    assert GcnTrainer.supports(m, g)
    return GcnTrainer.from_model(m, g, B, caps="exact", learning_rate=0.02), m, g


def _step(tr, m):
    loss = float(tr.forward_backward_only())
    torch.cuda.synchronize()
    assert int(tr.flow.overflow.item()) == 0
    return loss, {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _check_oracle(tr, loss_k, grads_k, tag):
    """the project's bf16-oracle bounds: loss 1e-4, every gradient 1e-3 relative"""
    loss_b, grads_b = tr.reference_loss_and_grads_bf16()
    rels = {n: float((grads_k[n].float().cpu() - r).norm() / max(float(r.norm()), 1e-12)) for n, r in grads_b.items()}
    print("oracle margin", tag, {"loss_rel": abs(loss_k - loss_b) / abs(loss_b), "grad_rel": rels})
    assert math.isfinite(loss_k) and abs(loss_k - loss_b) <= 1e-4 * abs(loss_b), (loss_k, loss_b)
    assert set(grads_b) == set(grads_k)
    for n, e in rels.items():
        assert e < 1e-3, (n, e)


@pytest.mark.gpu
@pytest.mark.parametrize("labels", ["onehot", "dense"])
def test_gcn_softmax_oracle_is_autograd_cross_entropy(world, labels, monkeypatch):
    """with the bf16 rounding switched off, the oracle's hand-written softmax head is autograd's
    cross-entropy (``-sum_c y_c log_softmax(x)_c`` for a dense row) of the model on the same roots"""
    from euler_amd.models.full_trainer import FullFlowTrainer

    tr, m, g = _trainer(world, 40, 2, True, labels)
    _step(tr, m)
    orig = torch.Tensor.to
    monkeypatch.setattr(torch.Tensor, "to",
                        lambda self, *a, **k: self if a and a[0] is torch.bfloat16 else orig(self, *a, **k))
    loss_o, grads_o = tr.reference_loss_and_grads_bf16()
    monkeypatch.setattr(torch.Tensor, "to", orig)
    roots = tr.plan.flow()["roots"].long().clone()
    for p in m.parameters():
        p.grad = None
    logits, _ = FullFlowTrainer.from_model(m, g, B, caps="exact")._forward(roots)
    y = g.labels[roots]
    if labels == "dense":
        assert (y.sum(1) != 1).any(), "the dense case must pin the s term"
        loss = -(y * torch.log_softmax(logits, 1)).sum(1).mean()
    else:
        loss = F.cross_entropy(logits, y.argmax(1))
    loss.backward()
    loss_r = float(loss.detach())
    print("oracle vs autograd", labels, abs(loss_o - loss_r) / loss_r)
    assert abs(loss_o - loss_r) <= 1e-6 * abs(loss_r)
    for n, p in m.named_parameters():
        err = float((grads_o[n] - p.grad.cpu()).norm() / p.grad.norm())
        print(" ", n, err)
        assert err < 1e-5, (n, err)


@pytest.mark.gpu
@pytest.mark.parametrize("C,layers,self_loops,labels", CASES)
def test_gcn_softmax_head_matches_oracle(world, C, layers, self_loops, labels):
    tr, m, _ = _trainer(world, C, layers, self_loops, labels)
    assert tr.loss_name == "softmax" and tr.metric_name == "acc"
    loss_k, grads_k = _step(tr, m)
    _check_oracle(tr, loss_k, grads_k, f"C{C}_L{layers}_sl{int(self_loops)}_{labels}")


@pytest.mark.gpu
def test_gcn_softmax_head_large_logits(world):
    """out_fc scaled by 64: exp overflows without the row max; loss and gradients stay finite
    and inside the oracle bounds"""
    tr, m, _ = _trainer(world, 100, 2, True, "onehot", out_scale=64.0)
    loss_k, grads_k = _step(tr, m)
    assert all(bool(torch.isfinite(v).all()) for v in grads_k.values())
    _check_oracle(tr, loss_k, grads_k, "large_logits")


@pytest.mark.gpu
def test_gcn_softmax_is_deterministic_and_counts_accuracy(world):
    tr, m, g = _trainer(world, 100, 1, False, "onehot")
    for _ in range(150):  # confident rows: the arg-max does not hang on bf16 rounding
        tr.step()
    rng = g.rng.clone()
    out = []
    for _ in range(2):
        g.rng.copy_(rng)
        tr.reset_metric()
        loss, grads = _step(tr, m)
        out.append((loss, torch.cat([v.reshape(-1) for v in grads.values()]), tr.counts.clone()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    tp, fp, fn = tr.counts.tolist()
    assert tp + fp == B and fp == fn
    roots = tr.plan.flow()["roots"].long()
    ids = roots.cpu().numpy() if g.ids is None else g.ids[roots.cpu().numpy()]
    _, logits, y = tr.infer_logits(ids)
    want = int((logits.argmax(1) == y.argmax(1)).sum())
    top = logits.topk(2, 1).values
    print("accuracy", tp, want, "least top-2 gap", float((top[:, 0] - top[:, 1]).min()))
    assert tp == want and 0 < want and tr.metric() == want / B


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["gcn", "fastgcn"])
def test_estimator_routes_softmax_gcn_to_the_fused_step(tmp_path, monkeypatch, model):
    monkeypatch.chdir(tmp_path)
    import euler_amd.estimator.base as eb
    from euler_amd.models.gcn_trainer import GcnTrainer
    from euler_amd.tools.runner import main

    box = {}
    orig = eb.BaseEstimator._train_device_graph
    monkeypatch.setattr(eb.BaseEstimator, "_train_device_graph", lambda self: (box.update(est=self), orig(self))[1])
    torch.manual_seed(0)
    argv = ["--dataset", "community", "--scale", "0.2", "--batch_size", "64", "--device", "cuda", "--seed", "1",
            "--model_dir", str(tmp_path / "ckpt"), "--device_graph", "--loss", "softmax", "--learning_rate", "0.01",
            "--data_dir", str(tmp_path / "data"),
            # FastGCN keeps only the edges into its sampled layer: a layer of half the 4000-node
            # graph leaves neighbourhoods to learn from (GCN takes no fanouts)
            "--fanouts", "2000", "2000"]
    first = main(argv + ["--total_step", "8", "--log_steps", "8"], model=model)
    last = main(argv + ["--total_step", "72", "--log_steps", "32"], model=model)  # resumes at step 8
    tr = box["est"].device_trainer
    assert isinstance(tr, GcnTrainer) and tr.device_trainer_kind == "gcn" and tr.loss_name == "softmax"
    assert last["step"] == 72 and last["loss"] < first["loss"] and "acc" in last and "f1" not in last
    ev = main(argv + ["--run_mode", "evaluate"], model=model)
    assert math.isfinite(ev["loss"]) and 0.0 <= ev["acc"] <= 1.0 and "f1" not in ev
