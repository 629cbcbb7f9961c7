"""models/kg_eval.rank_triples on the GPU (the kg_rank.hip kernels) against the CPU twin.

The tables hold rows of four +-0.5 entries: every normalisation leaves them unchanged and
every score is an exact dyadic sum, so the ranks are equal, not merely close.  TransH
exercises the relation-dependent grouping (one entity_space per relation).
"""
import copy

import pytest
import torch

from euler_amd import models as Z
from euler_amd.models import kg_eval

pytestmark = pytest.mark.gpu

N_ENT, N_REL, DIM = 300, 7, 20


def _dyadic_rows(rows, dim, g):
    out = torch.zeros(rows, dim)
    for i in range(rows):
        cols = torch.randperm(dim, generator=g)[:4]
        out[i, cols] = torch.randint(0, 2, (4,), generator=g).float() - 0.5
    return out


def _model(kind, g):
    args = (-1, [0], N_ENT - 1, N_REL - 1, DIM, DIM)
    m = {"transe": lambda: Z.TransE(*args), "transe_l2": lambda: Z.TransE(*args, l1=False),
         "distmult": lambda: Z.DistMult(*args), "transh": lambda: Z.TransH(*args)}[kind]()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(_dyadic_rows(p.shape[0], p.shape[1], g))
    return m


@pytest.mark.parametrize("kind", ["transe", "transe_l2", "distmult", "transh"])
def test_rank_triples_gpu_equals_cpu(kind):
    g = torch.Generator().manual_seed(12)
    cpu = _model(kind, g)
    gpu = copy.deepcopy(cpu).cuda()
    n = 500
    src, rel, dst = (torch.randint(0, N_ENT, (n,), generator=g), torch.randint(0, N_REL, (n,), generator=g),
                     torch.randint(0, N_ENT, (n,), generator=g))
    known = kg_eval.KnownTriples(src, rel, dst, N_ENT)
    cands = torch.unique(torch.cat([src, dst]))
    for kw in (dict(), dict(known=known), dict(known=known, ties="mean", batch=130), dict(known=known, cands=cands)):
        want = kg_eval.rank_triples(cpu, src[:200], rel[:200], dst[:200], **kw)
        if "known" in kw:
            kw = dict(kw, known=kg_eval.KnownTriples(src, rel, dst, N_ENT, device="cuda"))
        got = kg_eval.rank_triples(gpu, src[:200], rel[:200], dst[:200], **kw)
        for side in ("head", "tail"):
            assert got[side].is_cuda and got[side].dtype == want[side].dtype
            assert torch.equal(got[side].cpu(), want[side]), (kind, side, sorted(kw))
    res = kg_eval.link_prediction(gpu, (src[:200], rel[:200], dst[:200]), known=known)
    assert known.device.type == "cpu" and not known.tail_keys.is_cuda  # copied for the call, not moved
    ref = kg_eval.link_prediction(cpu, (src[:200], rel[:200], dst[:200]), known=known)
    # the ranks are equal; the float64 sums over them run in another order on the GPU
    # (n = 200 terms per side: a relative difference of at most n * 2^-53)
    assert res["n"] == ref["n"] == 200
    for key in ("mrr", "mr", "hit@1", "hit@3", "hit@10"):
        assert res[key] == pytest.approx(ref[key], rel=1e-12)
        for side in ("head", "tail"):
            assert res[side][key] == pytest.approx(ref[side][key], rel=1e-12)
