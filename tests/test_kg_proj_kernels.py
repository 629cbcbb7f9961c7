"""TransH / TransD scores with the projection inside the score kernel (csrc/hip/kg_proj.hip
kgp_fwd / kgp_bwd behind ops/gnn_ops.kg_score_proj) against the formulas in fp64, and the two
models' routing onto it (models/knowledge_graph.py, ``EULER_AMD_KG_PROJ_FUSED``).

Bounds: those of tests/test_gnn_kernels.py::test_kg_score_matches_reference (scores atol = rtol =
1e-4; gradients atol 1e-4, rtol 1e-3).  Measured maxima: profiles/kg_proj/oracle_margins.json.
"""
import pytest
import torch

from euler_amd.models.knowledge_graph import TransD, TransH
from euler_amd.ops import gnn_ops as G

B, K, NE, NR = 37, 3, 11, 5  # 37: the last block is partly empty; 11 / 5: every table row is hot


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def ref64(model, ent, rel, proj, src, dst, ridx, neg, kind, corrupt):
    """the issue's formulas, written out (fp64 when the tables are)"""
    r = _unit(rel[ridx])
    if model == "transh":
        w = _unit(proj[0][ridx])

        def P(i, w):
            return ent[i] - (ent[i] * w).sum(-1, keepdim=True) * w
    else:
        w = proj[1][ridx]

        def P(i, w):
            return _unit(ent[i] + (ent[i] * proj[0][i]).sum(-1, keepdim=True) * w)

    def score(d):
        return -(d.abs().sum(-1) if kind == "l1" else d.norm(dim=-1))

    h, t, n = P(src, w), P(dst, w), P(neg, w[:, None])
    front, tail = score(n + (r - t)[:, None]), score((h + r)[:, None] - n)
    return score(h + r - t), {"front": front, "tail": tail, "both": torch.cat([front, tail], -1)}[corrupt]


def inputs(model, D, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    shapes = [(NE, D), (NR, D)] + ([(NR, D)] if model == "transh" else [(NE, D), (NR, D)])
    tabs = [torch.randn(*s, generator=g).to(dev) for s in shapes]
    ids = [torch.randint(0, n, s, generator=g).to(dev) for n, s in ((NE, (B,)), (NE, (B,)), (NR, (B,)), (NE, (B, K)))]
    return tabs, ids


def run(fn, tabs, ids, kind, corrupt, model, grads=None):
    """scores and every table's gradient under the upstream gradients ``grads``"""
    tabs = [t.detach().clone().requires_grad_(True) for t in tabs]
    ps, ns = fn(model, tabs[0], tabs[1], tuple(tabs[2:]), *ids, kind, corrupt)
    if grads is None:
        g = torch.Generator().manual_seed(5)
        grads = [torch.randn(x.shape, generator=g).to(x) for x in (ps, ns)]
    ((ps * grads[0].to(ps)).sum() + (ns * grads[1].to(ns)).sum()).backward()
    return [ps.detach(), ns.detach()] + [t.grad for t in tabs], grads


CASES = [("transh", "l1", "both", 4), ("transd", "l2", "front", 4), ("transh", "l2", "both", 20),
         ("transd", "l1", "both", 20), ("transh", "l1", "front", 20), ("transd", "l2", "tail", 20),
         ("transh", "l1", "tail", 100), ("transd", "l1", "both", 100), ("transh", "l2", "front", 100),
         ("transd", "l2", "both", 100), ("transh", "l2", "tail", 256), ("transd", "l1", "front", 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("model,kind,corrupt,D", CASES)
def test_kg_score_proj_matches_fp64(cuda, model, kind, corrupt, D):
    tabs, ids = inputs(model, D, cuda)
    assert bool((ids[3] == ids[0][:, None]).any()), "a triple's negative should equal its own head"
    got, grads = run(G.kg_score_proj, tabs, ids, kind, corrupt, model)
    want, _ = run(ref64, [t.double() for t in tabs], ids, kind, corrupt, model, grads)
    names = ["pos", "neg", "d_ent", "d_rel"] + (["d_hyper"] if model == "transh" else ["d_ent_t", "d_rel_t"])
    for name, a, b in zip(names, got, want):
        print(name, "max abs err %.3e of max %.3e" % (float((a - b.float()).abs().max()), float(b.abs().max())))
    for i, (name, a, b) in enumerate(zip(names, got, want)):
        tol = dict(atol=1e-4, rtol=1e-4) if i < 2 else dict(atol=1e-4, rtol=1e-3)
        torch.testing.assert_close(a, b.float(), msg=lambda m, name=name: name + ": " + m, **tol)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", [TransH, TransD])
@pytest.mark.parametrize("rows_mode", [False, True])
def test_models_route_to_the_fused_scores(cuda, monkeypatch, cls, rows_mode):
    """loss_scores of a fused model against the same weights on the torch composition, on dense
    ids and on RowSparseKGTrainer's gathered rows + positions"""
    torch.manual_seed(2)
    fused = cls("n", "e", NE - 2, NR - 2, 20, 20, num_negs=K, l1=cls is TransH).to(cuda)
    monkeypatch.setenv("EULER_AMD_KG_PROJ_FUSED", "0")
    plain = cls("n", "e", NE - 2, NR - 2, 20, 20, num_negs=K, l1=cls is TransH).to(cuda)
    plain.load_state_dict(fused.state_dict())
    assert fused.fused_kind == ("l1" if cls is TransH else "l2") and plain.fused_kind is None
    _, (src, dst, rel, neg) = inputs("transh", 20, cuda)
    src[0] = -1  # the default node: the table's last row on both routes (Embedding._rows)
    out = []
    for m in (fused, plain):
        rows = None
        if rows_mode:  # every row gathered, in reverse order: position p holds entity NE - 1 - p
            rows = {k: getattr(m, k).weight.detach().flip(0).requires_grad_(True)
                    for k in ("entity_encoder", "entity_transfer") if hasattr(m, k)}
        loss, pos, neg_s = m.loss_scores(src.view(-1, 1), dst.view(-1, 1), neg, rel.view(-1, 1), rows=rows)
        loss.backward()
        grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
        grads.update({"rows." + k: v.grad for k, v in (rows or {}).items()})
        out.append((loss.detach(), pos.detach(), neg_s.detach(), grads))
    # the rows forward() returns next to the fused loss: the projected ones of the unfused forward
    s, d, _, r = plain.generate_embedding(src.view(-1, 1), dst.view(-1, 1), neg, rel.view(-1, 1))
    for a, b in zip(fused._fused_embeddings(src.view(-1, 1), dst.view(-1, 1), rel.view(-1, 1)), (s, r, d)):
        assert torch.equal(a, b)
    (l0, p0, n0, g0), (l1, p1, n1, g1) = out
    for a, b in ((l0, l1), (p0, p1), (n0, n1)):
        torch.testing.assert_close(a, b, atol=1e-4, rtol=1e-4)
    tables = {"relation_encoder.weight"} | ({"hyper_vector.weight"} if cls is TransH else {"relation_transfer.weight"})
    ent = {"entity_encoder"} | (set() if cls is TransH else {"entity_transfer"})
    tables |= {"rows." + k for k in ent} if rows_mode else {k + ".weight" for k in ent}
    assert set(g0) == set(g1) == tables
    for k in tables:
        assert float(g1[k].abs().max()) > 0
        torch.testing.assert_close(g0[k], g1[k], atol=1e-4, rtol=1e-3, msg=lambda m, k=k: k + ": " + m)


@pytest.mark.parametrize("model,D", [("transh", 6), ("transd", 8)])
def test_kg_score_proj_cpu_is_the_reference(model, D):
    tabs, ids = inputs(model, D, "cpu")
    for kind, corrupt in (("l1", "both"), ("l2", "front")):
        got, grads = run(G.kg_score_proj, tabs, ids, kind, corrupt, model)
        same, _ = run(G.kg_score_proj_reference, tabs, ids, kind, corrupt, model, grads)
        want, _ = run(ref64, tabs, ids, kind, corrupt, model, grads)
        for a, b, c in zip(got, same, want):
            assert torch.equal(a, b)
            torch.testing.assert_close(a, c, atol=1e-5, rtol=1e-4)
