"""models/kg_eval.rank_triples of the projected models (TransH / TransD / TransR) on the fused
route (ops/kg_rank_ops.rank_counts_proj: one call per batch and side, no entity_space) against
the per-relation loop it replaces (EULER_AMD_KG_RANK_PROJ_FUSED=0).
"""
import copy

import pytest
import torch

from euler_amd import models as Z
from euler_amd.models import kg_eval
from test_kg_rank_proj_kernels import _dyadic_rows, oracle, sandwich

N_ENT, N_REL, DIM, N_TEST = 300, 40, 20, 200


def _model(name, g):
    args = (-1, [0], N_ENT - 1, N_REL - 1, DIM, 8 if name == "transr" else DIM)
    m = {"transh": Z.TransH, "transd": Z.TransD, "transr": Z.TransR}[name](*args, l1=name != "transd")
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(_dyadic_rows(*p.shape, g) if name == "transh" else torch.randn(p.shape, generator=g))
    return m


def _triples(g):
    src, dst = torch.randint(0, N_ENT, (2, N_TEST), generator=g)
    return src, torch.randint(0, N_REL, (N_TEST,), generator=g), dst


def _loop(model, *a, **kw):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("EULER_AMD_KG_RANK_PROJ_FUSED", "0")
        return kg_eval.rank_triples(model, *a, **kw)


def _close(model, got, want, src, rel, dst, known):
    """random tables: the routes round differently, so both must lie in the sandwich of the
    float64 oracle (test_kg_rank_proj_kernels.oracle derives the margin); rank - 1 is
    ``better + ties``"""
    proj = [p.detach() for p in model._proj_tables()]
    if model.proj_model == "transd":
        proj[0] = proj[0][:N_ENT]
    tabs = [model._rank_table().detach(), model.relation_encoder.weight.detach()] + proj
    for side in ("head", "tail"):
        given, true = (src, dst) if side == "tail" else (dst, src)
        lists = None
        if known is not None:
            ptr, idx = known.filter(side, src, rel, dst)
            lists = [idx[ptr[i]:ptr[i + 1]].tolist() for i in range(src.numel())]
        lo, _, hi, _, _ = sandwich(*oracle(model.proj_model, tabs, given, rel, side, model.rank_kind), true, lists)
        for ranks in (got[side], want[side]):
            assert bool((lo <= ranks - 1).all()) and bool((ranks - 1 <= hi).all()), side


@pytest.mark.parametrize("name", ["transh", "transd", "transr"])
def test_cpu_twin_equals_loop(name):
    g = torch.Generator().manual_seed(21)
    model = _model(name, g)
    src, rel, dst = _triples(g)
    known = kg_eval.KnownTriples(src, rel, dst, N_ENT)
    for kw in (dict(), dict(known=known, batch=70)):
        got = kg_eval.rank_triples(model, src, rel, dst, **kw)
        want = _loop(model, src, rel, dst, **kw)
        if name == "transh":
            assert all(torch.equal(got[s], want[s]) for s in ("head", "tail"))
        else:
            _close(model, got, want, src, rel, dst, kw.get("known"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["transh", "transd", "transr"])
def test_gpu_route_takes_no_entity_space(name, monkeypatch):
    g = torch.Generator().manual_seed(22)
    cpu = _model(name, g)
    gpu = copy.deepcopy(cpu).cuda()
    src, rel, dst = _triples(g)
    known = kg_eval.KnownTriples(src, rel, dst, N_ENT)
    want = kg_eval.rank_triples(cpu, src, rel, dst, known=known)
    calls = []
    real = type(gpu).entity_space
    monkeypatch.setattr(type(gpu), "entity_space", lambda self, r=None: calls.append(r) or real(self, r))
    got = {s: r.cpu() for s, r in kg_eval.rank_triples(gpu, src, rel, dst, known=known, batch=70).items()}
    assert calls == []  # no per-relation projection on the fused route
    if name == "transh":
        assert all(torch.equal(got[s], want[s]) for s in ("head", "tail"))
    else:
        _close(cpu, got, want, src, rel, dst, known)
    # the candidate subset and the switch keep the per-relation loop
    kg_eval.rank_triples(gpu, src[:20], rel[:20], dst[:20], cands=torch.unique(torch.cat([src, dst])))
    assert len(calls) > 0
    n = len(calls)
    loop = _loop(gpu, src[:20], rel[:20], dst[:20])
    assert len(calls) > n
    fused = kg_eval.rank_triples(gpu, src[:20], rel[:20], dst[:20])
    if name == "transh":
        assert all(torch.equal(fused[s], loop[s]) for s in ("head", "tail"))
