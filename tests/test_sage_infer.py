"""Layer-wise full-neighbourhood GraphSAGE inference (models/sage_infer.py) through
SageTrainer and the estimator: a dense-adjacency model oracle, the cross-check against the
sampled path on a graph where sampling is deterministic, cache invalidation, and
``infer_mode`` of the estimator / runner.  CPU tests are unmarked, their GPU twins are ``gpu``.
"""
import numpy as np
import pytest
import torch

from test_sage_csr_kernels import ATOL, REL, bf, check_abc, dense_adj, figures, graph_of, make_csr, oracle_layer

# The model-level oracle checks use (c)'s ATOL of tests/test_sage_csr_kernels.py (their own
# measured excess over seeds 0..4, L = 1..3, with and without self loops, is 0).
# Layer-wise against the sampled path (test 7) is another comparison: the sampled path computes
# in fp32 on the fp32 master weights, layer-wise on bf16 tables and bf16 weight shadows, so the
# difference is the cost of bf16 over the whole model, not rare rounding flips.  Its absolute
# term is measured the same way: 4 x the largest excess max(|lw - s| - 2^-7 |s|) over seeds
# 0..4 on an MI355X, 8.748e-3 (largest |lw - s| 1.143e-2 on embeddings of magnitude ~1);
# profiles/sage_infer/oracle_margins.json, measure_margins().
ATOL_MODEL = ATOL
MEASURED_SAMPLED_EXCESS = 0.008748186752200127
ATOL_SAMPLED = 4.0 * MEASURED_SAMPLED_EXCESS

N, D, HID, E, C = 200, 24, 64, 32, 5
_PATHS = {1: [[0, 1]], 2: [[0, 1], [0]], 3: [[0, 1], [1], [0]]}
_FANOUTS = {1: [4], 2: [4, 3], 3: [4, 3, 2]}


def model_case(seed, L, self_loops, device):
    """a SageTrainer on a seeded 2-type graph with real-valued edge weights"""
    from euler_amd.models.sage_trainer import SageTrainer

    rng = np.random.default_rng(seed)
    d = rng.integers(0, 7, (N, 2))
    csr = make_csr(rng, N, 2, lambda r, t: int(d[r, t]), lambda n: rng.uniform(0.5, 1.5, n))
    gen = torch.Generator().manual_seed(seed)
    feats = torch.randn(N, D, generator=gen)
    labels = (torch.rand(N, C, generator=gen) < 0.3).float()
    tr = SageTrainer(graph_of(csr, 2, device), 32, _FANOUTS[L], [HID] * L + [E], C, features=feats, labels=labels,
                     metapath=_PATHS[L], add_self_loops=self_loops, init_seed=seed + 1)
    return csr, feats, tr


def dense_model(g_cpu, feats, params, fanouts, masks, self_loops, rows, rounded):
    """(h_{L-1} [n, H], fp32 embeddings [n, E]) of the rows from dense normalised adjacencies
    and the logical parameters; ``rounded``: bf16 weights, tables and A operands as the GPU path"""
    L = len(fanouts)
    inc = 1 if self_loops else 0
    rnd = bf if rounded else (lambda t: t)
    h = feats.float()
    for k in range(L):
        hop = L - 1 - k
        P, S = dense_adj(g_cpu, masks[hop], rows if k == L - 1 else None)
        W = torch.cat([params[f"gnn.convs.{k}.self_fc.weight"], params[f"gnn.convs.{k}.neigh_fc.weight"]], 1).cpu()
        F = fanouts[hop]
        h = oracle_layer(P, S, h, rnd(W.float()), F / (F + inc), inc / (F + inc), True, rounded)
    wfc, b = rnd(params["gnn.fc.weight"].float().cpu()), params["gnn.fc.bias"].float().cpu()
    return h, h @ wfc.t() + b


def _oracles(csr, feats, tr, rows, rounded):
    return dense_model(graph_of(csr, 2, "cpu"), feats, tr.logical_params(), tr.fanouts, tr.masks, tr.include_self,
                       rows, rounded)


_ROWS = [0, 199, 17, 17, 3, 150, 42]


# ----------------------------------------------------------------------------------------- 6. model oracle

@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_layerwise_matches_dense_model_cpu(L, self_loops):
    csr, feats, tr = model_case(0, L, self_loops, "cpu")
    lw = tr.layerwise()
    want = _oracles(csr, feats, tr, _ROWS, False)[1]
    emb = lw.embed(torch.tensor(_ROWS))
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (len(_ROWS), E)
    assert torch.allclose(emb, want, rtol=1e-5, atol=1e-5)
    emb2, logits = lw.logits(torch.tensor(_ROWS))
    assert tuple(logits.shape) == (len(_ROWS), C)
    assert torch.allclose(logits, want @ tr.logical_params()["out_fc.weight"].t(), rtol=1e-5, atol=1e-5)
    every = lw.embed()
    assert torch.allclose(every[_ROWS], want, rtol=1e-5, atol=1e-5)
    if L > 1:
        assert tuple(lw.hidden().shape) == (N, HID) and lw.hidden() is lw.hidden()
    else:
        assert lw.hidden() is lw.features  # a 1-hop model has no all-rows pass


@pytest.mark.gpu
@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_layerwise_matches_dense_model_gpu(cuda, L, self_loops):
    csr, feats, tr = model_case(0, L, self_loops, cuda)
    (ho, o), (hf, f) = _oracles(csr, feats, tr, _ROWS, True), _oracles(csr, feats, tr, _ROWS, False)
    lw = tr.layerwise()
    emb, logits = lw.logits(torch.tensor(_ROWS))
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (len(_ROWS), E) and tuple(logits.shape) == (
        len(_ROWS), C)
    # (a)-(c) on the bf16 output of the last conv layer, the last rounded value of the model;
    # (a) and (c) on the fp32 embeddings = fc of it (check_abc: why (b) says nothing there)
    check_abc(lw.last_conv(torch.tensor(_ROWS)), ho, hf, ATOL_MODEL, f"model h L={L} self={self_loops}")
    check_abc(emb, o, f, ATOL_MODEL, f"model emb L={L} self={self_loops}", exact_share=False)
    if L > 1:
        assert lw.hidden().dtype == torch.bfloat16 and tuple(lw.hidden().shape) == (N, HID)
    # row chunks give the same tables
    from euler_amd.models.sage_infer import LayerwiseSageInference

    convs, fc, out_fc = tr._layerwise_weights()
    small = LayerwiseSageInference(tr.graph, tr.features, convs, tr.fanouts, tr.masks, tr.include_self, fc=fc,
                                   out_fc=out_fc, row_chunk=64, embed_dim=E, logits_dim=C)
    assert torch.equal(small.embed(torch.tensor(_ROWS)), emb)


# ----------------------------------------------------------------------------------------- 7. sampled path

def one_edge_case(seed, self_loops, device):
    """every row has exactly one out-edge: every sampled draw is that neighbour"""
    from euler_amd.models.sage_trainer import SageTrainer

    rng = np.random.default_rng(seed)
    csr = make_csr(rng, N, 1, lambda r, t: 1, lambda n: rng.uniform(0.5, 1.5, n))
    gen = torch.Generator().manual_seed(seed)
    feats = torch.randn(N, D, generator=gen)
    labels = (torch.rand(N, C, generator=gen) < 0.3).float()
    return SageTrainer(graph_of(csr, 1, device), 32, [4, 3], [HID, HID, E], C, features=feats, labels=labels,
                       add_self_loops=self_loops, init_seed=seed + 1)


_IDS = np.array([0, 5, 199, 5, 64, 120, 33, 1])


@pytest.mark.parametrize("self_loops", [False, True])
def test_layerwise_equals_sampled_on_one_edge_graph_cpu(self_loops):
    tr = one_edge_case(0, self_loops, "cpu")
    emb_s, logits_s, y_s = tr.infer_logits(_IDS)
    emb_l, logits_l, y_l = tr.infer_logits_layerwise(_IDS)
    assert emb_l.shape == emb_s.shape and logits_l.shape == logits_s.shape and torch.equal(y_l, y_s)
    assert torch.allclose(emb_l, emb_s, rtol=1e-5, atol=1e-5)
    assert torch.allclose(logits_l, logits_s, rtol=1e-5, atol=1e-5)
    assert torch.equal(tr.infer_embed_layerwise(_IDS), emb_l)


@pytest.mark.gpu
@pytest.mark.parametrize("self_loops", [False, True])
def test_layerwise_equals_sampled_on_one_edge_graph_gpu(cuda, self_loops):
    tr = one_edge_case(0, self_loops, cuda)
    emb_s, logits_s, y_s = tr.infer_logits(_IDS)
    emb_l, logits_l, y_l = tr.infer_logits_layerwise(_IDS)
    assert emb_l.shape == emb_s.shape and logits_l.shape == logits_s.shape and torch.equal(y_l, y_s)
    d = (emb_l - emb_s).abs()
    excess = float((d - REL * emb_s.abs()).clamp(min=0).max())
    print(f"[sampled self={self_loops}] max |diff| {float(d.max()):.3e}  (c) excess {excess:.3e}  "
          f"atol {ATOL_SAMPLED:.3e}")
    assert excess <= ATOL_SAMPLED, (excess, ATOL_SAMPLED)


# ----------------------------------------------------------------------------------------- 8. cache

def _cache_invalidation(device):
    _, _, tr = model_case(1, 2, True, device)
    p0 = {k: v.clone() for k, v in tr.logical_params().items()}
    e0 = tr.infer_embed_layerwise(_IDS).clone()
    table = tr.layerwise().hidden()
    assert tr.layerwise().hidden() is table  # cached while the parameters stand
    tr.step()
    e1 = tr.infer_embed_layerwise(_IDS).clone()
    assert tr.layerwise().hidden() is not table
    assert not torch.equal(e0, e1)
    tr.load_logical(p0)
    assert torch.equal(tr.infer_embed_layerwise(_IDS), e0)


def test_cache_invalidation_cpu():
    _cache_invalidation("cpu")


@pytest.mark.gpu
def test_cache_invalidation_gpu(cuda):
    _cache_invalidation(cuda)


# ----------------------------------------------------------------------------------------- 9. estimator

def _estimator(tmp_path, device, model="graphsage", extra=()):
    from euler_amd.tools.runner import build, parse_args

    a = parse_args(["--dataset", "ppi", "--scale", "0.05", "--batch_size", "64", "--total_step", "4", "--log_steps",
                    "2", "--model_dir", str(tmp_path / "ckpt"), "--infer_dir", str(tmp_path / "inf"),
                    "--device_graph", "--device", device, "--seed", "1", "--fanouts", "5", "3",
                    "--device_feature_dtype", "fp32"] + list(extra), model)
    return build(a)[1]


def _counted(obj, name):
    calls = []
    fn = getattr(obj, name)

    def wrapper(*a, **kw):
        calls.append(1)
        return fn(*a, **kw)

    setattr(obj, name, wrapper)
    return calls


def _estimator_layerwise(tmp_path, device):
    est = _estimator(tmp_path, device, extra=["--infer_mode", "layerwise"])
    assert est.params["infer_mode"] == "layerwise"
    est.train()
    tr = est.device_trainer
    ids, embs = est.infer()
    inf = tmp_path / "inf"
    f_emb, f_ids = np.load(inf / "embedding_0.npy"), np.load(inf / "ids_0.npy")
    assert np.array_equal(f_ids, ids) and np.array_equal(f_emb, embs) and len(ids) > 0
    want = tr.infer_embed_layerwise(ids).float().cpu().numpy()
    assert np.array_equal(f_emb, want)
    est.infer()  # deterministic: a second run writes the same files
    assert np.array_equal(np.load(inf / "embedding_0.npy"), f_emb) and np.array_equal(np.load(inf / "ids_0.npy"),
                                                                                       f_ids)
    lw_calls, s_calls = _counted(tr, "infer_logits_layerwise"), _counted(tr, "infer_logits")
    ev = est.evaluate()
    assert lw_calls and not s_calls
    assert np.isfinite(ev["loss"]) and len(ev) == 2
    assert est.evaluate() == ev
    # "sampled" and an absent key take the sampled path
    for mode in ("sampled", None):
        if mode is None:
            est.params.pop("infer_mode")
        else:
            est.params["infer_mode"] = mode
        s_emb, l_emb = _counted(tr, "infer_embed"), _counted(tr, "infer_embed_layerwise")
        est.infer()
        assert s_emb and not l_emb
    est.params["infer_mode"] = "treewise"
    with pytest.raises(ValueError, match="infer_mode"):
        est.infer()


def test_estimator_infer_mode_layerwise_cpu(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _estimator_layerwise(tmp_path, "cpu")


@pytest.mark.gpu
def test_estimator_infer_mode_layerwise_gpu(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _estimator_layerwise(tmp_path, "cuda")


def test_estimator_layerwise_refuses_gcn(tmp_path, monkeypatch):
    """a trainer without layer-wise inference is an error that names the reason, never a
    silent fall back to sampled or engine-path inference"""
    monkeypatch.chdir(tmp_path)
    est = _estimator(tmp_path, "cpu", model="gcn", extra=["--infer_mode", "layerwise"])
    with pytest.raises(ValueError, match="layer-wise"):
        est.infer()
    with pytest.raises(ValueError, match="layer-wise"):
        est.evaluate()
    est.params["device_graph"] = False
    with pytest.raises(ValueError, match="device_graph"):
        est.infer()


def test_sharded_trainer_has_no_layerwise():
    from euler_amd.models.sharded_sage import ShardedSageTrainer

    assert ShardedSageTrainer.infer_logits_layerwise is None and ShardedSageTrainer.infer_embed_layerwise is None


# ----------------------------------------------------------------------------------------- margins

def measure_margins(device, seeds=range(5)):
    """the figures behind ATOL_MODEL / ATOL_SAMPLED: per seed, (a) / (b) / (c)-excess of the
    embeddings against the model oracles, and the excess of layer-wise against sampled"""
    rec = {"rel": REL, "seeds": list(seeds), "model_vs_oracle": [], "layerwise_vs_sampled": []}
    for s in seeds:
        for L in (1, 2, 3):
            for sl in (False, True):
                csr, feats, tr = model_case(s, L, sl, device)
                (ho, o), (hf, f) = _oracles(csr, feats, tr, _ROWS, True), _oracles(csr, feats, tr, _ROWS, False)
                lw = tr.layerwise()
                for what, got, a, b in (("h", lw.last_conv(torch.tensor(_ROWS)), ho, hf),
                                        ("emb", lw.embed(torch.tensor(_ROWS)), o, f)):
                    ratio, share, excess = figures(got, a, b)
                    rec["model_vs_oracle"].append({"seed": s, "L": L, "self_loops": sl, "what": what,
                                                   "rms_ratio": ratio, "share": share, "excess": excess})
        for sl in (False, True):
            tr = one_edge_case(s, sl, device)
            es, el = tr.infer_embed(_IDS), tr.infer_embed_layerwise(_IDS)
            d = (el - es).abs()
            rec["layerwise_vs_sampled"].append({"seed": s, "self_loops": sl, "max_abs_diff": float(d.max()),
                                                "excess": float((d - REL * es.abs()).clamp(min=0).max())})
    for name in ("model_vs_oracle", "layerwise_vs_sampled"):
        rec["max_excess_" + name] = max(r["excess"] for r in rec[name])
    return rec
