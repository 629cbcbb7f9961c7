"""TransR scores with the per-triple MFMA projection inside the score kernel (csrc/hip/kg_transr.hip
kgr_fwd / kgr_bwd behind ops/gnn_ops.kg_score_proj) against the formulas in fp64, and the model's
routing onto it (models/knowledge_graph.py, ``EULER_AMD_KG_PROJ_FUSED``).

Bounds: those of tests/test_kg_proj_kernels.py (scores atol = rtol = 1e-4; gradients atol 1e-4,
rtol 1e-3).  Measured maxima: profiles/kg_transr/oracle_margins.json.
"""
import json
import os

import pytest
import torch

from euler_amd.models.knowledge_graph import TransR
from euler_amd.ops import gnn_ops as G

B, NE, NR = 37, 11, 5  # every table row is hot; each M_r takes several triples' atomics
MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kg_transr",
                       "oracle_margins.json")


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def ref64(model, ent, rel, proj, src, dst, ridx, neg, kind, corrupt, diffs=None):
    """the issue's formulas, written out (fp64 when the tables are); ``diffs`` collects every
    score's difference vector"""
    M = proj[0][ridx].reshape(-1, ent.shape[1], rel.shape[1])
    r = _unit(rel[ridx])

    def P(i):
        return _unit(torch.einsum("b...e,ber->b...r", ent[i], M))

    def score(d):
        if diffs is not None:
            diffs.append(d.detach().reshape(-1))
        return -(d.abs().sum(-1) if kind == "l1" else d.norm(dim=-1))

    h, t, n = P(src), P(dst), P(neg)
    front, tail = score(n + (r - t)[:, None]), score((h + r)[:, None] - n)
    return score(h + r - t), {"front": front, "tail": tail, "both": torch.cat([front, tail], -1)}[corrupt]


def inputs(E, R, K, dev, seed=7):
    g = torch.Generator().manual_seed(seed)
    tabs = [torch.randn(*s, generator=g).to(dev) for s in ((NE, E), (NR, R), (NR, E * R))]
    ids = [torch.randint(0, n, s, generator=g).to(dev) for n, s in ((NE, (B,)), (NE, (B,)), (NR, (B,)), (NE, (B, K)))]
    return tabs, ids


def run(fn, tabs, ids, kind, corrupt, grads=None, **kw):
    """scores and every table's gradient under the upstream gradients ``grads``"""
    tabs = [t.detach().clone().requires_grad_(True) for t in tabs]
    ps, ns = fn("transr", tabs[0], tabs[1], (tabs[2],), *ids, kind, corrupt, **kw)
    if grads is None:
        g = torch.Generator().manual_seed(5)
        grads = [torch.randn(x.shape, generator=g).to(x) for x in (ps, ns)]
    ((ps * grads[0].to(ps)).sum() + (ns * grads[1].to(ns)).sum()).backward()
    return [ps.detach(), ns.detach()] + [t.grad for t in tabs], grads


CASES = [("l1", "both", 4, 4, 3), ("l2", "front", 20, 12, 3), ("l1", "tail", 12, 36, 0), ("l2", "both", 100, 100, 5),
         ("l1", "both", 128, 128, 14), ("l2", "tail", 64, 128, 14), ("l1", "front", 128, 16, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,corrupt,E,R,K", CASES)
def test_kg_score_transr_matches_fp64(cuda, kind, corrupt, E, R, K):
    tabs, ids = inputs(E, R, K, cuda)
    assert K == 0 or bool((ids[3] == ids[0][:, None]).any()), "a triple's negative should equal its own head"
    got, grads = run(G.kg_score_proj, tabs, ids, kind, corrupt)
    diffs = []
    want, _ = run(ref64, [t.double() for t in tabs], ids, kind, corrupt, grads, diffs=diffs)
    # the L1 gradient is a sign: no component of any score's difference may sit at its jump (seed
    # 7 was picked for this on the CPU).  The full tile at 128 x 128 has 137,344 components and
    # no seed of 1..39 keeps them all above 1.8e-5: its floor is 1e-5, ~100 fp32 errors of one.
    assert kind == "l2" or float(torch.cat(diffs).abs().min()) > (1e-5 if (E, R, K) == (128, 128, 14) else 1e-4)
    names = ["pos", "neg", "d_ent", "d_rel", "d_mat"]
    errs = {n: float((a - b.float()).abs().max()) if a.numel() else 0.0 for n, a, b in zip(names, got, want)}
    print(kind, corrupt, E, R, K, errs)
    if os.path.isdir(os.path.dirname(MARGINS)):
        seen = json.load(open(MARGINS)) if os.path.exists(MARGINS) else {}
        seen["%s-%s-%d-%d-%d" % (kind, corrupt, E, R, K)] = errs
        json.dump(seen, open(MARGINS, "w"), indent=1, sort_keys=True)
    for i, (name, a, b) in enumerate(zip(names, got, want)):
        tol = dict(atol=1e-4, rtol=1e-4) if i < 2 else dict(atol=1e-4, rtol=1e-3)
        torch.testing.assert_close(a, b.float(), msg=lambda m, name=name: name + ": " + m, **tol)


@pytest.mark.gpu
@pytest.mark.parametrize("rows_mode", [False, True])
def test_transr_routes_to_the_fused_scores(cuda, monkeypatch, rows_mode):
    """loss_scores of the fused model against the same weights on the torch composition, on dense
    ids and on RowSparseKGTrainer's gathered rows + positions"""
    K = 3
    torch.manual_seed(2)
    fused = TransR("n", "e", NE - 2, NR - 2, 20, 12, num_negs=K, l1=False).to(cuda)
    assert TransR("n", "e", NE - 2, NR - 2, 20, 6, num_negs=K).fused_kind is None  # rel_dim outside the kernels
    monkeypatch.setenv("EULER_AMD_KG_PROJ_FUSED", "0")
    plain = TransR("n", "e", NE - 2, NR - 2, 20, 12, num_negs=K, l1=False).to(cuda)
    plain.load_state_dict(fused.state_dict())
    assert fused.fused_kind == "l2" and plain.fused_kind is None
    _, (src, dst, rel, neg) = inputs(20, 12, K, cuda)
    src[0] = -1  # the default node: the table's last row on both routes (Embedding._rows)
    out = []
    for m in (fused, plain):
        rows = None
        if rows_mode:  # every row gathered, in reverse order: position p holds entity NE - 1 - p
            rows = {"entity_encoder": m.entity_encoder.weight.detach().flip(0).requires_grad_(True)}
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
    tables = {"relation_encoder.weight", "transfer_matrix.weight",
              "rows.entity_encoder" if rows_mode else "entity_encoder.weight"}
    assert set(g0) == set(g1) == tables
    for k in tables:
        assert float(g1[k].abs().max()) > 0
        torch.testing.assert_close(g0[k], g1[k], atol=1e-4, rtol=1e-3, msg=lambda m, k=k: k + ": " + m)
    # 15 negatives do not fit the 16-row tile: the composition, without error
    wide = torch.randint(0, NE, (B, 15), device=cuda)
    _, _, n15 = fused.loss_scores(src.view(-1, 1), dst.view(-1, 1), wide, rel.view(-1, 1))
    _, _, w15 = plain.loss_scores(src.view(-1, 1), dst.view(-1, 1), wide, rel.view(-1, 1))
    assert torch.equal(n15, w15)


def test_kg_score_transr_cpu_is_the_reference():
    tabs, ids = inputs(8, 6, 3, "cpu")
    for kind, corrupt in (("l1", "both"), ("l2", "front")):
        got, grads = run(G.kg_score_proj, tabs, ids, kind, corrupt)
        same, _ = run(G.kg_score_proj_reference, tabs, ids, kind, corrupt, grads)
        want, _ = run(ref64, tabs, ids, kind, corrupt, grads)
        for a, b, c in zip(got, same, want):
            assert torch.equal(a, b)
            torch.testing.assert_close(a, c, atol=1e-5, rtol=1e-4)
