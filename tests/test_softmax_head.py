"""``loss="softmax"``: single-label node classification through every layer — the softmax
instantiation of the fused head (csrc/hip/tree_head.hip), SageTrainer and its oracles, the
SupervisedGNN models, the estimator's device evaluate and the runner flag.

GPU: the head against the bf16-aware oracle at the smallest shapes at which it can go wrong
(padded columns inside a tile, a real column alone in its tile, 7 tiles merged, dense target
rows whose sums are not 1, 1 / 2 / 3 hops, the bench widths), logits beyond +-88, bitwise
determinism, hipGraph replay, exact accuracy counts, and the sigmoid head bit for bit.
CPU: the oracles against autograd, the torch trainer, the engine-path model, the runner.
"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# _graph / _tables / _cmp / _trainer: the shapes of tests/test_sage_trainer.py, with a ``loss``
# argument, a one-hot dense label mode, and class ids that cover all C classes when C > D


def _graph(device, n=6000, types=1, seed=3):
    from euler_amd.graph.device_graph import DeviceGraph

    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 12, n * types)
    indptr = np.zeros(n * types + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    nbr = rng.integers(0, n, int(indptr[-1])).astype(np.int32)
    for s in range(n * types):  # sorted segments like the engine
        a, b = indptr[s], indptr[s + 1]
        nbr[a:b].sort()
    w = rng.uniform(0.5, 1.5, int(indptr[-1]))
    nw = rng.uniform(0.1, 1.0, n)
    return DeviceGraph.from_csr(indptr, nbr, w, num_types=types, node_weights=nw, seed=seed, device=device)


def _tables(device, n, D, C, mode, fdt=torch.bfloat16, seed=5):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=gen)
    score = x[:, :C] if C <= D else x @ torch.randn(D, C, generator=gen)
    if mode == "class":
        lab = score.argmax(1).to(torch.int16)
    elif mode == "class32":
        lab = score.argmax(1).to(torch.int32)
    elif mode == "onehot":
        lab = F.one_hot(score.argmax(1), C).float()
    else:  # multi-hot rows: sums 0 .. C, the s term of the dense softmax gradient
        lab = (score > 0.3).float()
    return x.to(device=device, dtype=fdt), lab.to(device)


def _cmp(a, b):
    a, b = a.float().reshape(-1).cpu(), b.float().reshape(-1).cpu()
    if b.norm() < 1e-9:
        return 1.0, float(a.norm())
    cos = F.cosine_similarity(a, b, dim=0).item()
    rel = ((a - b).norm() / b.norm()).item()
    return cos, rel


def _trainer(device, fanouts, dims, C, mode="class", fdt=torch.bfloat16, D=20, B=64, self_loops=False, opt="adam",
             seed=3, lr=0.01, **kw):
    from euler_amd.models.sage_trainer import SageTrainer

    g = _graph(device, seed=seed)
    g.manual_seed(seed + 17)
    x, lab = _tables(device, g.num_rows, D, C, mode, fdt)
    return SageTrainer(g, B, fanouts, dims, C, features=x, labels=lab, add_self_loops=self_loops, optimizer=opt,
                       learning_rate=lr, init_seed=seed, **kw)


def _first_max(t):
    """arg-max with ties to the lowest column"""
    return (t == t.max(1, keepdim=True).values).int().argmax(1)


# ----------------------------------------------------------------------------------------- CPU


def test_unknown_loss_is_refused_cpu():
    from euler_amd import models as Z

    with pytest.raises(ValueError, match="loss"):
        _trainer("cpu", [5, 3], [32, 32, 16], 5, loss="hinge")
    with pytest.raises(ValueError, match="loss"):
        Z.SupervisedGraphSage([16, 16, 7], [3, 3], [["train"], ["train"]], "feature", 8, "label", 7, loss="hinge")
    assert _trainer("cpu", [5, 3], [32, 32, 16], 5).metric_name == "f1"
    assert _trainer("cpu", [5, 3], [32, 32, 16], 5, loss="softmax").metric_name == "acc"


# the three configurations of test_bf16_oracle_is_the_model_without_rounding_cpu; the dense ones
# have rows that are not one-hot (sums != 1: the s term)
@pytest.mark.parametrize("cfg", [dict(fanouts=[6], dims=[40, 24], C=10),
                                 dict(fanouts=[5, 3], dims=[64, 64, 32], C=10, self_loops=True, mode="dense"),
                                 dict(fanouts=[3, 20, 2], dims=[64, 128, 64, 32], C=16, D=64, mode="dense",
                                      self_loops=True)])
def test_softmax_oracles_are_autograd_cross_entropy_cpu(cfg, monkeypatch):
    """with the bf16 rounding switched off the hand-written softmax head of the bf16-aware oracle
    is autograd's: ``F.cross_entropy`` for class ids, ``-sum_c y_c log_softmax(x)_c`` per row for
    dense rows (s logsumexp(x) - sum_c y_c x_c)"""
    tr = _trainer("cpu", fdt=torch.float32, loss="softmax", **cfg)
    tr.step()
    orig = torch.Tensor.to

    def no_bf16(self, *a, **k):
        return self if a and a[0] is torch.bfloat16 else orig(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "to", no_bf16)
    loss_o, grads_o = tr.reference_loss_and_grads_bf16()
    monkeypatch.setattr(torch.Tensor, "to", orig)
    # autograd, written here independently of the trainer's loss helper
    params = {k: v.detach().float().clone().requires_grad_(True) for k, v in tr.logical_params().items()}
    roots, nodes, leaf = tr.samples()
    logits = tr.logical_forward(params, roots, nodes, leaf)
    if tr.label_mode == 2:
        y = tr._labels_dense[roots]
        assert (y.sum(1) != 1).any(), "the dense case must pin the s term"
        loss = -(y * torch.log_softmax(logits, 1)).sum(1).mean()
    else:
        loss = F.cross_entropy(logits, tr.labels[roots].long())
    loss.backward()
    loss_r, grads_r = float(loss.detach()), {k: v.grad for k, v in params.items()}
    loss_f, grads_f = tr.reference_loss_and_grads()
    for lo, gr in ((loss_o, grads_o), (loss_f, grads_f)):
        assert abs(lo - loss_r) <= 1e-6 * abs(loss_r) and set(gr) == set(grads_r)
        for k in grads_r:
            assert ((gr[k] - grads_r[k]).norm() / grads_r[k].norm()).item() < 1e-5, k


def test_cpu_softmax_trainer_learns_and_reports_accuracy():
    tr = _trainer("cpu", [5, 3], [32, 32, 16], 5, loss="softmax")
    first = np.mean([float(tr.step()) for _ in range(5)])
    for _ in range(60):
        tr.step()
    # metric() is the row accuracy of the steps since the reset, recomputed here from the
    # parameters each step started with
    tr.reset_metric()
    last, ok, rows = [], 0, 0
    for _ in range(5):
        P = tr.logical_params()
        last.append(float(tr.step()))
        roots, nodes, leaf = tr.samples()
        with torch.no_grad():
            pred = _first_max(tr.logical_forward(P, roots, nodes, leaf))
        ok += int((pred == tr.labels[roots].long()).sum())
        rows += roots.numel()
    assert np.mean(last) < first, (first, np.mean(last))
    assert tr.metric() == pytest.approx(ok / rows, abs=1e-12) and 0 < ok < rows


@pytest.fixture(scope="module")
def _cora(tmp_path_factory):
    from euler_amd.dataset import get_dataset

    ds = get_dataset("cora", data_dir=str(tmp_path_factory.mktemp("cora")), scale=0.08)
    ds.get_data_dir()
    return ds


def test_supervised_graphsage_softmax_engine_path_cpu(_cora):
    import euler_amd as ea
    import euler_amd.ops.graph_api as ge
    from euler_amd import models as Z

    ds = _cora
    ds.load_graph()
    ld = ds.label_dim

    def build(**kw):
        torch.manual_seed(0)
        return Z.SupervisedGraphSage([16, 16, ld], [3, 3], [["train"], ["train"]], "feature", 1433, "label", ld,
                                     max_id=ds.max_node_id, **kw)

    ea.set_seed(3)
    ids = torch.as_tensor(np.asarray(ge.sample_node(48, -1)).astype(np.int64))
    label = ge.get_dense_feature(ids, ["label"], [ld])[0]
    out = {}
    for name, kw in (("default", {}), ("sigmoid", dict(loss="sigmoid")), ("softmax", dict(loss="softmax"))):
        m = build(**kw)
        ea.set_seed(11)  # the same sampled neighbourhoods for every model
        emb, loss, mname, metric = m(ids)
        out[name] = (m.out_fc(emb).float().detach(), float(loss), mname, float(metric))
    logits, loss, mname, metric = out["softmax"]
    assert mname == "acc"
    assert loss == pytest.approx(float(F.cross_entropy(logits, label.argmax(1))), rel=1e-6)
    assert metric == pytest.approx(float((logits.argmax(1) == label.argmax(1)).float().mean()), abs=1e-6)
    # a sigmoid model is what it was: the default, BCE and micro-F1
    assert out["default"][1:] == out["sigmoid"][1:] and torch.equal(out["default"][0], out["sigmoid"][0])
    logits, loss, mname, metric = out["sigmoid"]
    assert mname == "f1" and torch.equal(logits, out["softmax"][0])
    assert loss == pytest.approx(float(F.binary_cross_entropy_with_logits(logits, label.float())), rel=1e-6)


def test_runner_softmax_device_graph_train_resume_evaluate_cpu(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from euler_amd.tools.runner import main

    def run(steps):
        return main(["--dataset", "ppi", "--scale", "0.05", "--batch_size", "64", "--total_step", str(steps),
                     "--log_steps", "10", "--model_dir", str(tmp_path / "ckpt"), "--device_graph", "--device", "cpu",
                     "--seed", "1", "--fanouts", "5", "3", "--loss", "softmax"], model="graphsage")

    r1 = run(20)
    assert r1["step"] == 20 and math.isfinite(r1["loss"]) and "acc" in r1 and "f1" not in r1
    r2 = run(30)  # resumes from model.ckpt-20
    assert r2["step"] == 30 and math.isfinite(r2["loss"])
    ev = main(["--dataset", "ppi", "--scale", "0.05", "--batch_size", "64", "--model_dir", str(tmp_path / "ckpt"),
               "--run_mode", "evaluate", "--device", "cpu", "--fanouts", "5", "3", "--loss", "softmax"],
              model="graphsage")
    assert math.isfinite(ev["loss"]) and 0.0 <= ev["acc"] <= 1.0 and "f1" not in ev
    with pytest.raises(SystemExit, match="--loss softmax"):
        main(["--dataset", "cora", "--loss", "softmax", "--total_step", "1"], model="lgcn")


def test_gcn_softmax_model_trains_on_the_generic_trainer_cpu():
    """the fused GCN head is sigmoid only: GcnTrainer.supports turns a softmax model away"""
    from types import SimpleNamespace

    from euler_amd.models.gcn_trainer import GcnTrainer

    assert GcnTrainer.supports(SimpleNamespace(loss="softmax")) is False


def test_community_heldout_accuracy_engine_and_device_paths_cpu(tmp_path, monkeypatch):
    monkeypatch.setenv("EULER_AMD_DATA", str(tmp_path / "data"))
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(ROOT, "benchmarks"))
    from bench_community_f1 import main

    out = main(["--steps", "150", "--device", "cpu", "--loss", "softmax"])
    eng, dev = out["engine"]["heldout"]["acc"], out["device"]["heldout"]["acc"]
    # floor: the engine path (plain torch, independent of the device trainer) measured 0.8942
    # held-out accuracy on the CPU at these flags; 0.05 under it
    assert eng > 0.844 and dev > 0.844, (eng, dev)
    assert abs(eng - dev) < 0.05, (eng, dev)


# ----------------------------------------------------------------------------------------- GPU

CASES = [
    # one hop, two blocks, padded columns inside the only real tile pair
    dict(fanouts=[6], dims=[40, 24], C=10, B=32),
    dict(fanouts=[5, 3], dims=[64, 64, 32], C=32),                                # int16 ids, no padding
    dict(fanouts=[5, 3], dims=[64, 64, 32], C=33, mode="class32"),                # one real column alone in its tile
    dict(fanouts=[5, 3], dims=[40, 72, 24], C=100, mode="onehot"),                # Cp = 128, 7 tiles merged
    dict(fanouts=[5, 3], dims=[64, 64, 32], C=16, mode="dense"),                  # dense rows, sums != 1
    dict(fanouts=[4, 3, 2], dims=[64, 64, 64, 32], C=64, self_loops=True),        # three hops
    dict(fanouts=[25, 10], dims=[256, 256, 256], C=64, D=128, B=128),             # bench widths
]
_MARGINS = {}


def _check_oracle(tr, tag):
    """forward_backward() against the bf16-aware oracle (tight) and the fp32 model (loose);
    returns the oracle's logits-free figures for the margin file"""
    tr.forward_backward()
    torch.cuda.synchronize()
    loss_k = float(tr.loss_acc.item())
    grads_k = tr.gradients()
    assert math.isfinite(loss_k) and all(bool(torch.isfinite(g).all()) for g in grads_k.values())
    loss_b, grads_b = tr.reference_loss_and_grads_bf16()
    rels = {name: _cmp(grads_k[name], grads_b[name])[1] for name in grads_b}
    _MARGINS[tag] = {"loss_rel": abs(loss_k - loss_b) / abs(loss_b), "grad_rel_max": max(rels.values()),
                     "grad_rel": rels, "bounds": {"loss_rel": 1e-4, "grad_rel": 1e-3}}
    print(tag, json.dumps(_MARGINS[tag]))
    assert abs(loss_k - loss_b) <= 1e-4 * abs(loss_b), (loss_k, loss_b)
    for name, rel in rels.items():
        assert rel < 1e-3, (name, rel)
    return loss_k, grads_k


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    if _MARGINS and os.environ.get("EULER_AMD_WRITE_MARGINS"):
        path = os.path.join(ROOT, "profiles", "softmax_head", "oracle_margins.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_MARGINS, f, indent=1, sort_keys=True)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CASES, ids=[f"case{i}" for i in range(len(CASES))])
def test_softmax_head_matches_oracle(cuda, cfg):
    tr = _trainer(cuda, loss="softmax", **cfg)
    loss_k, grads_k = _check_oracle(tr, "case%d" % CASES.index(cfg))
    # loose, second check: the plain fp32 model (bf16 operand noise)
    loss_r, grads_r = tr.reference_loss_and_grads()
    assert abs(loss_k - loss_r) <= 2e-2 * abs(loss_r) + 1e-4, (loss_k, loss_r)
    for name in grads_r:
        cos, rel = _cmp(grads_k[name], grads_r[name])
        assert cos > 0.995 and rel < 0.1, (name, cos, rel)
    # padded parameter entries get no gradient
    ref = torch.zeros_like(tr.grad)
    tr._pack(grads_k, ref)
    assert torch.equal(ref, tr.grad)


@pytest.mark.gpu
def test_softmax_head_large_logits(cuda):
    """out_fc scaled by 64: logits beyond +-88 (exp overflows without the row max) give a finite
    loss and finite gradients that still meet the tight oracle"""
    tr = _trainer(cuda, [5, 3], [40, 72, 24], 100, mode="onehot", loss="softmax")
    P = tr.logical_params()
    P["out_fc.weight"] = P["out_fc.weight"] * 64.0
    tr.load_logical(P)
    _check_oracle(tr, "large_logits")
    roots, nodes, leaf = tr.samples()
    logits = tr.logical_forward(tr.logical_params(), roots, nodes, leaf)
    assert float(logits.abs().max()) > 88.0, float(logits.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [CASES[3], CASES[4]], ids=["onehot100", "dense16"])
def test_softmax_head_is_deterministic_and_counts_accuracy(cuda, cfg):
    a = _trainer(cuda, loss="softmax", **cfg)
    b = _trainer(cuda, loss="softmax", **cfg)
    a.forward_backward()
    b.forward_backward()
    torch.cuda.synchronize()
    assert torch.equal(a.grad, b.grad) and torch.equal(a.loss_acc, b.loss_acc)
    # accuracy counts: exactly the arg-max count of the oracle's logits (bf16-aware forward)
    tp, fp, fn = a.counts.tolist()
    assert tp + fp == a.B and fp == fn
    roots, nodes, leaf = a.samples()
    logits = _oracle_logits(a)
    gap = logits.topk(2, 1).values
    assert float((gap[:, 0] - gap[:, 1]).min()) > 1e-4, "a near-tie would make the count depend on rounding"
    want = int((_first_max(logits) == _first_max(a._labels_of(roots).to(logits.device))).sum())
    assert tp == want and 0 < want < a.B, (tp, want)
    assert a.metric() == want / a.B and a.metric_name == "acc"


def _oracle_logits(tr):
    """the logits of reference_loss_and_grads_bf16 (its loss helper sees them)"""
    from euler_amd.models import sage_trainer

    seen = {}
    orig = sage_trainer.head_loss

    def spy(logits, y, loss="sigmoid"):
        seen["logits"] = logits.detach().clone()
        return orig(logits, y, loss)

    sage_trainer.head_loss = spy
    try:
        tr.reference_loss_and_grads_bf16()
    finally:
        sage_trainer.head_loss = orig
    return seen["logits"]


@pytest.mark.gpu
def test_softmax_graph_replay_matches_eager(cuda):
    a = _trainer(cuda, [5, 3], [64, 64, 32], 32, loss="softmax")
    b = _trainer(cuda, [5, 3], [64, 64, 32], 32, loss="softmax")
    la = []
    for _ in range(12):
        a.step()
        la.append(float(a.loss.item()))
    b.capture(warmup=2)
    lb = []
    for _ in range(10):
        b.replay()
        lb.append(float(b.loss.item()))
    np.testing.assert_allclose(lb, la[2:], rtol=2e-3, atol=1e-5)
    assert la[-1] < la[0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["class", "dense"])
def test_sigmoid_head_is_untouched(cuda, mode):
    """no ``loss=`` and ``loss="sigmoid"``: the same kernel, bit-identical gradient, loss, counts"""
    a = _trainer(cuda, [5, 3], [40, 72, 24], 10, mode=mode)
    b = _trainer(cuda, [5, 3], [40, 72, 24], 10, mode=mode, loss="sigmoid")
    c = _trainer(cuda, [5, 3], [40, 72, 24], 10, mode=mode, loss="softmax")
    for t in (a, b, c):
        t.forward_backward()
    torch.cuda.synchronize()
    assert torch.equal(a.grad, b.grad) and torch.equal(a.loss_acc, b.loss_acc) and torch.equal(a.counts, b.counts)
    assert a.metric_name == "f1" and not torch.equal(a.grad, c.grad)
    loss_b, _ = a.reference_loss_and_grads_bf16()
    assert abs(float(a.loss_acc.item()) - loss_b) <= 1e-4 * abs(loss_b)


@pytest.mark.gpu
def test_softmax_head_refuses_more_classes_than_its_waves_hold(cuda):
    with pytest.raises(ValueError, match="at most 256 classes"):
        _trainer(cuda, [5, 3], [64, 64, 32], 300, loss="softmax")
    _trainer(cuda, [5, 3], [64, 64, 32], 300)  # the sigmoid head loops over its tiles
