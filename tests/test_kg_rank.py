"""Link-prediction ranking on the CPU: the torch twin of ops/kg_rank_ops.py, the model hooks of
models/knowledge_graph.py, models/kg_eval.py, EdgeEstimator.rank_evaluate() and the runner.

Exact data as in tests/test_kg_rank_kernels.py: integers in [-4, 4] stored as fp32, so every
score is an exact integer and the comparisons are ``torch.equal``.
"""
import functools

import numpy as np
import pytest
import torch

import euler_amd as ea
from euler_amd import models as Z
from euler_amd.dataset import get_dataset
from euler_amd.estimator import EdgeEstimator
from euler_amd.models import kg_eval
from euler_amd.ops import kg_rank_ops

KINDS = ("l1", "l2", "dot")


# ----------------------------------------------------------------------------- the twin
@functools.lru_cache(maxsize=None)
def _int_data():
    g = torch.Generator().manual_seed(11)
    c = torch.randint(-4, 5, (200, 20), generator=g)
    q = torch.randint(-4, 5, (33, 20), generator=g)
    c[3] = c[0]       # copies of true rows: ties, never better
    c[198] = c[199]
    t = (torch.arange(33) * 37) % 200
    t[0], t[32] = 0, 199
    return c, q, t


def _brute(q, c, t, kind, lists=None):
    """one python loop per (query, candidate) pair, int arithmetic"""
    q, c = q.tolist(), c.tolist()
    better, ties = [], []

    def score(a, b):
        if kind == "dot":
            return -sum(x * y for x, y in zip(a, b))  # lower is better from here on
        return sum(abs(x - y) if kind == "l1" else (x - y) ** 2 for x, y in zip(a, b))

    for b, row in enumerate(q):
        ts = score(row, c[t[b]])
        out = set(lists[b]) if lists is not None else set()
        nb = nt = 0
        for e, cand in enumerate(c):
            if e == t[b] or e in out:
                continue
            s = score(row, cand)
            nb += s < ts
            nt += s == ts
        better.append(nb)
        ties.append(nt)
    return torch.tensor(better), torch.tensor(ties)


def _lists(name, b, n, t):
    if name == "none":
        return None
    if name == "empty":
        return [[] for _ in range(b)]
    if name == "only_true":
        return [[t[i]] for i in range(b)]
    if name == "all":
        return [list(range(n)) for _ in range(b)]
    g = torch.Generator().manual_seed(5)
    return [sorted(torch.randperm(n, generator=g)[:[0, 1, 5, n // 3, n // 2 + 7, n][(i + 4) % 6]].tolist())
            for i in range(b)]


def _csr(lists):
    ptr = torch.zeros(len(lists) + 1, dtype=torch.long)
    ptr[1:] = torch.tensor([len(l) for l in lists]).cumsum(0)
    return ptr, torch.tensor([e for l in lists for e in l], dtype=torch.int32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["none", "empty", "only_true", "all", "mixed"])
def test_twin_equals_brute_force(name, kind, monkeypatch):
    c, q, t = _int_data()
    lists = _lists(name, q.shape[0], c.shape[0], t.tolist())
    ptr, idx = _csr(lists) if lists is not None else (None, None)
    monkeypatch.setattr(kg_rank_ops, "_TWIN_SCORES", 7 * 200 * 20)  # several chunks of queries
    better, ties = kg_rank_ops.rank_counts(q.float(), c.float(), t, kind, ptr, idx)
    wb, wt = _brute(q, c, t.tolist(), kind, lists)
    assert torch.equal(better, wb) and torch.equal(ties, wt)
    if name in ("none", "empty", "only_true"):
        assert int(ties[0]) >= 1 and int(ties[-1]) >= 1  # the copies of the true rows
    rb, rt = _brute(q, c, t.tolist(), kind)
    assert bool((better <= rb).all()) and bool((ties <= rt).all())


def test_twin_rejects_bad_operands():
    c, q, t = _int_data()
    q, c = q.float(), c.float()
    ptr, idx = _csr([[] for _ in range(q.shape[0])])
    for args in [(q.t().contiguous().t(), c, t), (q, c.t().contiguous().t(), t), (q.double(), c, t),
                 (q, c, t.int()), (q, c, t + 1), (q, c, t - 1), (q, c, t, ptr[:-1], idx), (q, c, t, ptr, idx.long()),
                 (q, c, t, ptr, None)]:
        with pytest.raises(ValueError):
            kg_rank_ops.rank_counts(args[0], args[1], args[2], "l1", *args[3:])
    with pytest.raises(ValueError):
        kg_rank_ops.rank_counts(q, c, t, "cosine")


# ----------------------------------------------------------------------------- the models
N_ENT, N_REL, DIM = 40, 5, 8


def _dyadic_rows(rows, dim, g, nonzero=4):
    """rows with ``nonzero`` entries of +-0.5: their l2 norm is exactly 1 and F.normalize
    returns them unchanged, so every normalised table is dyadic"""
    out = torch.zeros(rows, dim)
    for i in range(rows):
        cols = torch.randperm(dim, generator=g)[:nonzero]
        out[i, cols] = (torch.randint(0, 2, (nonzero,), generator=g).float() - 0.5)
    return out


def _small_ints(rows, dim, g):
    return torch.randint(-2, 3, (rows, dim), generator=g).float() / 2


def _model(kind, g):
    args = (-1, [0], N_ENT - 1, N_REL - 1)
    if kind == "transe_l2":
        m = Z.TransE(*args, DIM, DIM, l1=False)
    elif kind == "transr":
        m = Z.TransR(*args, DIM, 6)
    else:
        m = {"transe": Z.TransE, "transh": Z.TransH, "transd": Z.TransD, "distmult": Z.DistMult}[kind](*args, DIM, DIM)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith(("entity_encoder", "relation_encoder", "hyper_vector")) and kind not in (
                    "transr", "transd"):
                p.copy_(_dyadic_rows(p.shape[0], p.shape[1], g))
            else:
                p.copy_(_small_ints(p.shape[0], p.shape[1], g))
    return m


def _test_triples(g, n=60):
    return (torch.randint(0, N_ENT, (n,), generator=g), torch.randint(0, N_REL, (n,), generator=g),
            torch.randint(0, N_ENT, (n,), generator=g))


def _own_scores(model, src, rel, dst, dtype):
    """scores of every entity as tail and as head through the model's own generate_embedding +
    calculate_scores, the candidates passed as ``neg``; the embeddings are cast to ``dtype``
    before calculate_scores.  Returns (pos [B], tail [B, N], head [B, N], emb)."""
    b = src.numel()
    neg = torch.arange(N_ENT).repeat(b, 1)
    with torch.no_grad():
        s, d, n, r = model.generate_embedding(src.view(-1, 1), dst.view(-1, 1), neg, rel.view(-1, 1))
        s, d, n, r = s.to(dtype), d.to(dtype), n.to(dtype), r.to(dtype)
        return (model.calculate_scores(s, r, d).reshape(b), model.calculate_scores(s, r, n),
                model.calculate_scores(n, r, d), (s, d, n, r))


@pytest.mark.parametrize("kind", ["transe", "transe_l2", "distmult", "transh"])
def test_rank_triples_equals_model_scores_dyadic(kind):
    """Equality was chosen here: the tables hold rows of four +-0.5 entries, which every
    normalisation leaves unchanged, so both paths compute exact dyadic sums."""
    g = torch.Generator().manual_seed(2)
    model = _model(kind, g)
    src, rel, dst = _test_triples(g)
    ranks = kg_eval.rank_triples(model, src, rel, dst, known=None, ties="pessimistic", batch=16)
    pos, tail, head, _ = _own_scores(model, src, rel, dst, torch.float32)
    ar = torch.arange(src.numel())
    for side, sc, true in (("tail", tail, dst), ("head", head, src)):
        keep = torch.ones_like(sc, dtype=torch.bool)
        keep[ar, true] = False
        want = 1 + ((sc >= pos.unsqueeze(1)) & keep).sum(1)  # higher model score is better
        assert torch.equal(ranks[side], want), side
    assert int((ranks["tail"] > 1).sum()) > 0


@pytest.mark.parametrize("kind", ["transr", "transd"])
def test_rank_triples_sandwiches_model_scores(kind):
    """The sandwich rule was chosen here: TransR / TransD normalise after their projection, so
    the candidate rows are not dyadic.  The raw tables are small multiples of 1/2, which makes
    the projection before the normalisation exact, and entity_space(r) is then bitwise the
    model's own projected rows (asserted).  The oracle is the model's calculate_scores on
    float64 casts of those rows, and the margin is the one of the kernel tests,
    m = 2 * D' * 2^-23 * S_max (S_max: the largest sum of absolute terms over all pairs, from
    the oracle): the rank must lie between the number of candidates better than the true
    score by more than m and the number better than the true score minus m."""
    g = torch.Generator().manual_seed(4)
    model = _model(kind, g)
    src, rel, dst = _test_triples(g)
    ranks = kg_eval.rank_triples(model, src, rel, dst, known=None, ties="pessimistic", batch=16)
    opt = kg_eval.rank_triples(model, src, rel, dst, known=None, ties="optimistic", batch=16)
    pos, tail, head, (s, d, n, r) = _own_scores(model, src, rel, dst, torch.float64)
    for i in range(src.numel()):
        assert torch.equal(model.entity_space(int(rel[i])).double(), n[i])
    dp = model.rel_dim
    s_max = float(max((s + r - n).abs().sum(-1).max(), (n + r - d).abs().sum(-1).max()))
    m = 2 * dp * 2.0 ** -23 * s_max
    ar = torch.arange(src.numel())
    for side, sc, true in (("tail", tail, dst), ("head", head, src)):
        keep = torch.ones_like(sc, dtype=torch.bool)
        keep[ar, true] = False
        lo = 1 + ((sc > pos.unsqueeze(1) + m) & keep).sum(1)
        hi = 1 + ((sc > pos.unsqueeze(1) - m) & keep).sum(1)
        print(kind, side, "m", m, "max hi - lo", int((hi - lo).max()))
        for got in (ranks[side], opt[side]):
            assert bool((lo <= got).all()) and bool((got <= hi).all()), side


def test_model_hooks():
    g = torch.Generator().manual_seed(1)
    for kind, dep, rk in [("transe", False, "l1"), ("transe_l2", False, "l2"), ("distmult", False, "dot"),
                          ("transh", True, "l1"), ("transr", True, "l1"), ("transd", True, "l1")]:
        m = _model(kind, g)
        assert m.relation_dependent is dep and m.rank_kind == rk
        assert m.entity_space(1).shape == (N_ENT, m.rel_dim)  # no padding row
        assert m.relation_row(1).shape == (m.rel_dim,)
        assert torch.equal(m.relation_row(torch.tensor([1, 3]))[1], m.relation_row(3))


def test_sharded_model_raises():
    m = Z.TransE(-1, [0], N_ENT - 1, N_REL - 1, DIM, DIM, sharded=True)
    z = torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="sharded"):
        kg_eval.rank_triples(m, z, z, z + 1)
    with pytest.raises(ValueError, match="sharded"):
        m.entity_space()


# ----------------------------------------------------------------------------- the library
def test_known_triples_against_sets():
    g = torch.Generator().manual_seed(9)
    n, r, m = 30, 4, 400
    src, rel, dst = (torch.randint(0, n, (m,), generator=g), torch.randint(0, r, (m,), generator=g),
                     torch.randint(0, n, (m,), generator=g))
    src, rel, dst = torch.cat([src, src[:50]]), torch.cat([rel, rel[:50]]), torch.cat([dst, dst[:50]])  # repeats
    tails, heads = {}, {}
    for h, k, t in zip(src.tolist(), rel.tolist(), dst.tolist()):
        tails.setdefault((h, k), set()).add(t)
        heads.setdefault((k, t), set()).add(h)
    known = kg_eval.KnownTriples(src, rel, dst, n)
    assert len(known) == len({(h, k, t) for h, k, t in zip(src.tolist(), rel.tolist(), dst.tolist())})
    qs, qr, qd = (torch.randint(0, n, (100,), generator=g), torch.randint(0, r, (100,), generator=g),
                  torch.randint(0, n, (100,), generator=g))
    for (ptr, idx), want in ((known.tail_filter(qs, qr), [tails.get((h, k), set()) for h, k in
                                                           zip(qs.tolist(), qr.tolist())]),
                             (known.head_filter(qd, qr), [heads.get((k, t), set()) for k, t in
                                                           zip(qr.tolist(), qd.tolist())])):
        assert ptr.dtype == torch.long and idx.dtype == torch.int32 and ptr.numel() == 101
        assert int(ptr[0]) == 0 and int(ptr[-1]) == idx.numel()
        for i, w in enumerate(want):
            got = idx[int(ptr[i]):int(ptr[i + 1])].tolist()
            assert got == sorted(w)
    with pytest.raises(ValueError):
        kg_eval.KnownTriples(src, rel, dst, n - 1 if int(max(src.max(), dst.max())) == n - 1 else 1)
    with pytest.raises(ValueError, match="int64"):  # rel * n^2 would wrap the packed keys
        kg_eval.KnownTriples(torch.tensor([1]), torch.tensor([3000]), torch.tensor([2]), 1 << 26)
    assert known.to("cpu") is known and known.to(torch.device("cpu")).device == known.device


@pytest.mark.parametrize("kind", ["transe", "transh", "distmult"])
def test_filtered_and_tie_rules(kind):
    g = torch.Generator().manual_seed(6)
    model = _model(kind, g)
    src, rel, dst = _test_triples(g, 200)
    known = kg_eval.KnownTriples(src, rel, dst, N_ENT)
    test = (src[:80], rel[:80], dst[:80])
    raw = {t: kg_eval.rank_triples(model, *test, ties=t, batch=32) for t in kg_eval.TIE_RULES}
    fil = {t: kg_eval.rank_triples(model, *test, known=known, ties=t, batch=32) for t in kg_eval.TIE_RULES}
    changed = 0
    for side in ("head", "tail"):
        for t in kg_eval.TIE_RULES:
            assert bool((fil[t][side] <= raw[t][side]).all())
            assert bool((fil[t][side] >= 1).all())
            changed += int((fil[t][side] < raw[t][side]).sum())
        for res in (raw, fil):
            assert res["pessimistic"][side].dtype == torch.long and res["mean"][side].dtype == torch.float64
            assert bool((res["optimistic"][side] <= res["mean"][side]).all())
            assert bool((res["mean"][side] <= res["pessimistic"][side]).all())
            assert torch.equal(res["mean"][side] * 2, (res["optimistic"][side] + res["pessimistic"][side]).double())
    assert changed > 0
    # a filter by hand: the known answers of the first triple, brute force on the model's hooks
    h, r, t = int(src[0]), int(rel[0]), int(dst[0])
    with torch.no_grad():
        space, rho = model.entity_space(r), model.relation_row(r)
    sc = kg_rank_ops._scores(model.rank_query(space[h:h + 1], rho, "tail"), space, model.rank_kind)[0]
    sc = -sc if model.rank_kind == "dot" else sc
    others = {int(d) for s_, r_, d in zip(src.tolist(), rel.tolist(), dst.tolist()) if (s_, r_) == (h, r)} - {t}
    want = 1 + sum(1 for e in range(N_ENT) if e != t and e not in others and float(sc[e]) <= float(sc[t]))
    assert int(fil["pessimistic"]["tail"][0]) == want


def test_cands_subset():
    g = torch.Generator().manual_seed(8)
    model = _model("transe", g)
    src, rel, dst = _test_triples(g, 40)
    cands = torch.unique(torch.cat([src, dst, torch.tensor([0, 5])]))
    known = kg_eval.KnownTriples(src, rel, dst, N_ENT)
    sub = kg_eval.rank_triples(model, src, rel, dst, known=known, cands=cands.flip(0))
    full = kg_eval.rank_triples(model, src, rel, dst, known=known)
    with torch.no_grad():
        space = model.entity_space()
    for side in ("head", "tail"):
        assert bool((sub[side] <= full[side]).all()) and bool((sub[side] >= 1).all())
    # tail side of the first triples by hand among the candidates only
    for i in range(5):
        h, r, t = int(src[i]), int(rel[i]), int(dst[i])
        sc = (space[h] + model.relation_row(r).detach() - space).abs().sum(-1)
        others = {int(d) for s_, r_, d in zip(src.tolist(), rel.tolist(), dst.tolist()) if (s_, r_) == (h, r)} - {t}
        want = 1 + sum(1 for e in cands.tolist() if e != t and e not in others and float(sc[e]) <= float(sc[t]))
        assert int(sub["tail"][i]) == want
    with pytest.raises(ValueError, match="not among cands"):
        kg_eval.rank_triples(model, src, rel, dst, cands=cands[cands != dst[0]])


def test_link_prediction_metrics_by_hand():
    g = torch.Generator().manual_seed(3)
    model = _model("transe", g)
    test = _test_triples(g, 50)
    ranks = kg_eval.rank_triples(model, *test)
    res = kg_eval.link_prediction(model, test, ks=(1, 3, 10))
    assert set(res) == {"mrr", "mr", "hit@1", "hit@3", "hit@10", "head", "tail", "n"} and res["n"] == 50
    for side in ("head", "tail"):
        r = [float(x) for x in ranks[side].tolist()]
        assert set(res[side]) == {"mrr", "mr", "hit@1", "hit@3", "hit@10"}
        assert res[side]["mrr"] == pytest.approx(sum(1 / x for x in r) / 50, rel=1e-12)
        assert res[side]["mr"] == pytest.approx(sum(r) / 50, rel=1e-12)
        for k in (1, 3, 10):
            assert res[side]["hit@%d" % k] == pytest.approx(sum(x <= k for x in r) / 50, rel=1e-12)
    for key in ("mrr", "mr", "hit@1", "hit@3", "hit@10"):
        assert res[key] == pytest.approx((res["head"][key] + res["tail"][key]) / 2, rel=1e-12)
    one = kg_eval.link_prediction(model, test, sides=("tail",))
    assert "head" not in one and one["mrr"] == one["tail"]["mrr"]


# ----------------------------------------------------------------------------- estimator, runner
@pytest.fixture(scope="module")
def _fb(tmp_path_factory):
    ds = get_dataset("fb15k", data_dir=str(tmp_path_factory.mktemp("fb")), scale=0.01)
    ds.get_data_dir()
    return ds


@pytest.fixture
def fb(_fb):
    _fb.load_graph()
    ea.set_seed(5)
    return _fb


def test_rank_evaluate_on_synthetic_fb15k(fb, tmp_path):
    torch.manual_seed(0)
    params = {"model_dir": str(tmp_path / "ckpt"), "batch_size": 64, "total_step": 30, "optimizer": "adam",
              "learning_rate": 0.02, "log_steps": 10, "train_edge_type": "train", "device": "cpu", "seed": 7,
              "id_file": fb.edge_id_file}

    def model():
        return Z.TransE("train", "train", fb.max_node_id, fb.max_edge_id, 16, 16, num_negs=4)

    def evaluate():
        ea.set_seed(21)  # the corruptions of evaluate() are engine draws
        torch.manual_seed(21)
        return EdgeEstimator(model(), params).evaluate()

    EdgeEstimator(model(), params).train()
    before = evaluate()
    est = EdgeEstimator(model(), dict(params, rank_filter_edge_types=list(fb.all_edge_type)))
    res = est.rank_evaluate()
    with open(fb.edge_id_file) as f:
        lines = sum(1 for line in f if line.strip())
    keys = {"mrr", "mr", "hit@1", "hit@3", "hit@10"}
    assert set(res) == keys | {"head", "tail", "n"} and set(res["head"]) == keys and set(res["tail"]) == keys
    assert res["n"] == lines and lines > 0
    assert 0.0 < res["mrr"] <= 1.0 and 1.0 <= res["mr"] <= fb.max_node_id + 1
    default = EdgeEstimator(model(), params).rank_evaluate()  # no edge types named: every edge of the graph
    assert default == res
    raw = EdgeEstimator(model(), dict(params, rank_filter_edge_types=[])).rank_evaluate()
    assert raw["n"] == lines and raw["mrr"] <= res["mrr"] and raw["mr"] >= res["mr"]
    # the restored tables rank as the library does on the same triples
    triples = torch.tensor(np.loadtxt(fb.edge_id_file, dtype=np.int64).reshape(-1, 3))
    rel = torch.as_tensor(np.asarray(ea.get_edge_dense_feature(triples.numpy(), ["id"], [1])[0])).reshape(-1).long()
    lib = kg_eval.link_prediction(est.model, (triples[:, 0], rel, triples[:, 1]))
    assert lib["mrr"] == pytest.approx(raw["mrr"], rel=1e-12)
    # evaluate() is untouched: the training metric against the sampled corruptions
    after = evaluate()
    assert set(after) == {"loss", "mrr"} and after == before


def test_runner_rank_evaluate(tmp_path):
    from euler_amd.tools import runner

    common = ["--model", "transe", "--data_dir", str(tmp_path / "fb15k"), "--scale", "0.004", "--batch_size", "8",
              "--dim", "8", "--model_dir", str(tmp_path / "ckpt"), "--device", "cpu", "--num_negs", "2"]
    runner.main(common + ["--total_step", "2", "--log_steps", "1"])
    res = runner.main(common + ["--run_mode", "rank_evaluate"])
    raw = runner.main(common + ["--run_mode", "rank_evaluate", "--rank_filter", "raw", "--rank_ties", "optimistic"])
    assert res["n"] == raw["n"] > 0 and 0.0 < res["mrr"] <= 1.0
    a = runner.parse_args(["--model", "transe", "--run_mode", "rank_evaluate"])
    assert a.rank_filter == "filtered" and a.rank_ties == "pessimistic"
