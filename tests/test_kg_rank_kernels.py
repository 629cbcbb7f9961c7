"""Link-prediction rank kernels (csrc/hip/kg_rank.hip) behind ops/kg_rank_ops.py.

Exact data: candidate and query values are integers in [-4, 4] stored as fp32 with D <= 200,
so every l1 sum, squared l2 sum and dot product is an integer below 2^24 and exact in fp32 in
any summation order.  The oracle is int64 arithmetic on the CPU and the comparisons are
``torch.equal`` on ``better`` and ``ties``.  Integer data produces many ties, which is the
point.

Float data: l2-normalised normal rows against a float64 oracle under the fp32 summation
bound (see ``test_float_sandwich``).
"""
import functools

import pytest
import torch

from euler_amd.ops import kg_rank_ops
from euler_amd.ops._native import hip

pytestmark = pytest.mark.gpu

NMAX, DMAX, BMAX = 1000, 200, 130
KINDS = ("l1", "l2", "dot")


@functools.lru_cache(maxsize=None)
def _int_data():
    g = torch.Generator().manual_seed(11)
    c = torch.randint(-4, 5, (NMAX, DMAX), generator=g)
    q = torch.randint(-4, 5, (BMAX, DMAX), generator=g)
    return c, q


def _true_idx(b, n):
    """first candidate for query 0, last candidate for the last query, spread in between"""
    t = (torch.arange(b) * 37) % n
    t[0] = 0
    t[b - 1] = n - 1
    return t


def _cands(n, d):
    """the first n rows; rows 3 and n - 2 are copies of the first and the last row, the
    true rows of the first and the last query"""
    c = _int_data()[0][:n, :d].clone()
    if n > 4:
        c[3] = c[0]
        c[n - 2] = c[n - 1]
    return c


def _int_scores(q, c, kind):
    q, c = q.long(), c.long()
    if kind == "dot":
        return q @ c.t()
    diff = q.unsqueeze(1) - c.unsqueeze(0)
    return diff.abs().sum(-1) if kind == "l1" else (diff * diff).sum(-1)


@functools.lru_cache(maxsize=None)
def _score_matrix(n, d, kind):
    return _int_scores(_int_data()[1][:, :d], _cands(n, d), kind)


def _oracle(b, n, d, kind, lists=None):
    """(better, ties) by int64 arithmetic; lists: per-query python lists of filtered positions"""
    sc = _score_matrix(n, d, kind)[:b]
    t = _true_idx(b, n)
    ts = sc.gather(1, t.unsqueeze(1))
    keep = torch.ones(b, n, dtype=torch.bool)
    keep[torch.arange(b), t] = False
    if lists is not None:
        for i, l in enumerate(lists):
            keep[i, torch.tensor(l, dtype=torch.long)] = False
    bt = sc > ts if kind == "dot" else sc < ts
    return (bt & keep).sum(1), ((sc == ts) & keep).sum(1)


def _csr(lists):
    ptr = torch.zeros(len(lists) + 1, dtype=torch.long)
    ptr[1:] = torch.tensor([len(l) for l in lists]).cumsum(0)
    idx = torch.tensor([e for l in lists for e in l], dtype=torch.int32)
    return ptr.cuda(), idx.cuda()


def _run(b, n, d, kind, lists=None, **kw):
    q = _int_data()[1][:b, :d].float().contiguous().cuda()
    c = _cands(n, d).float().contiguous().cuda()
    ptr, idx = _csr(lists) if lists is not None else (None, None)
    better, ties = kg_rank_ops.rank_counts(q, c, _true_idx(b, n).cuda(), kind, ptr, idx, **kw)
    assert better.dtype == torch.long and ties.dtype == torch.long
    return better.cpu(), ties.cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
@pytest.mark.parametrize("b", [1, 7, 130])
@pytest.mark.parametrize("d", [1, 4, 20, 100, 200])
def test_shapes(d, b, n, kind):
    better, ties = _run(b, n, d, kind)
    ob, ot = _oracle(b, n, d, kind)
    assert torch.equal(better, ob)
    assert torch.equal(ties, ot)
    if n > 4:
        # the copy of the true row is a tie, never better
        assert int(ties[0]) >= 1 and int(ties[b - 1]) >= 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("splits", [1, 3, 16, 4096])
def test_splits_agree(kind, splits):
    """any number of candidate ranges, including more ranges than tiles and more
    (query tile, range) items than the grid holds"""
    better, ties = _run(130, 1000, 20, kind, splits=splits)
    ob, ot = _oracle(130, 1000, 20, kind)
    assert torch.equal(better, ob) and torch.equal(ties, ot)


def _filter_lists(name, b, n):
    t = _true_idx(b, n).tolist()
    if name == "empty":
        return [[] for _ in range(b)]
    if name == "only_true":
        return [[t[i]] for i in range(b)]
    if name == "all":
        return [list(range(n)) for _ in range(b)]
    g = torch.Generator().manual_seed(5)
    lists = []
    for i in range(b):
        ln = [0, 1, 5, n // 3, n // 2 + 7, n][i % 6] if i else n // 2 + 7  # one longer than N / 2
        lists.append(sorted(torch.randperm(n, generator=g)[:min(ln, n)].tolist()))
    return lists


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b,n,d", [(130, 1000, 20), (7, 63, 100), (130, 65, 1)])
@pytest.mark.parametrize("name", ["empty", "only_true", "all", "mixed"])
def test_filters(name, b, n, d, kind):
    lists = _filter_lists(name, b, n)
    better, ties = _run(b, n, d, kind, lists)
    ob, ot = _oracle(b, n, d, kind, lists)
    assert torch.equal(better, ob) and torch.equal(ties, ot)
    rb, rt = _oracle(b, n, d, kind)
    assert bool((better <= rb).all()) and bool((ties <= rt).all())
    if name in ("empty", "only_true"):
        assert torch.equal(better, rb) and torch.equal(ties, rt)
    if name == "all":
        assert int(better.sum()) == 0 and int(ties.sum()) == 0


def test_rejects_bad_operands():
    c, q = _int_data()
    q = q[:7, :20].float().contiguous().cuda()
    c = c[:63, :20].float().contiguous().cuda()
    t = _true_idx(7, 63).cuda()
    ptr, idx = _csr([[] for _ in range(7)])
    native = hip().kg_rank_counts
    errors = (ValueError, RuntimeError, TypeError)
    bad = [
        dict(q=q.t().contiguous().t()),                      # non-contiguous
        dict(cands=c.t().contiguous().t()),
        dict(q=q.double()), dict(cands=c.half()), dict(true_idx=t.int()),
        dict(q=q.cpu()),
        dict(true_idx=torch.where(t == 0, torch.full_like(t, 63), t)),   # one past the end
        dict(true_idx=torch.where(t == 0, torch.full_like(t, -1), t)),
        dict(filt_ptr=ptr[:-1], filt_idx=idx), dict(filt_ptr=torch.cat([ptr, ptr[-1:]]), filt_idx=idx),
        dict(filt_ptr=ptr.int(), filt_idx=idx), dict(filt_ptr=ptr, filt_idx=idx.long()),
        dict(filt_ptr=ptr),
    ]
    for change in bad:
        args = dict(q=q, cands=c, true_idx=t, filt_ptr=None, filt_idx=None)
        args.update(change)
        with pytest.raises(errors):
            kg_rank_ops.rank_counts(args["q"], args["cands"], args["true_idx"], "l1", args["filt_ptr"],
                                    args["filt_idx"])
        with pytest.raises(errors):  # the binding validates on its own
            native(args["q"], args["cands"], args["true_idx"], 0, args["filt_ptr"], args["filt_idx"], 1)
    with pytest.raises(errors):
        kg_rank_ops.rank_counts(q, c, t, "cosine")
    with pytest.raises(errors):
        native(q, c, t, 3, None, None, 1)
    with pytest.raises(errors):
        native(q, c, t, 0, None, None, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [20, 7])
def test_unaligned_rows(d, kind):
    """a candidate table that starts at an odd float offset takes the scalar-load variant"""
    b, n = 130, 1000
    q = _int_data()[1][:b, :d].float().contiguous().cuda()
    c = _cands(n, d).float().contiguous().cuda()
    buf = torch.zeros(1 + n * d, device="cuda")
    view = buf[1:].view(n, d)
    view.copy_(c)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    t = _true_idx(b, n).cuda()
    got = kg_rank_ops.rank_counts(q, view, t, kind)
    want = kg_rank_ops.rank_counts(q, view.clone(), t, kind)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ob, ot = _oracle(b, n, d, kind)
    assert torch.equal(got[0].cpu(), ob) and torch.equal(got[1].cpu(), ot)


@pytest.mark.parametrize("kind", KINDS)
def test_float_sandwich(kind):
    """l2-normalised normal rows, D = 100, N = 1000, B = 130 against a float64 oracle.

    An fp32 sum of D terms differs from the exact sum by at most D * 2^-24 * (sum of the
    absolute terms) to first order, the candidate's score and the true score both carry that
    error, so two scores further apart than m = 2 * D * 2^-23 * (largest sum of absolute terms
    over all pairs) cannot change order.  ``better`` and ``better + ties`` must therefore lie
    between the number of candidates better than the true score by more than m and the number
    better than the true score minus m."""
    D, N, B = 100, 1000, 130
    g = torch.Generator().manual_seed(3)
    c = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    q = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=-1)
    t = _true_idx(B, N)
    q64, c64 = q.double(), c.double()
    if kind == "dot":
        terms = q64.unsqueeze(1) * c64.unsqueeze(0)
    else:
        terms = q64.unsqueeze(1) - c64.unsqueeze(0)
        terms = terms.abs() if kind == "l1" else terms * terms
    sc = terms.sum(-1)
    m = 2 * D * 2.0 ** -23 * float(terms.abs().sum(-1).max())
    if kind == "dot":
        sc = -sc  # lower is better from here on
    ts = sc.gather(1, t.unsqueeze(1))
    keep = torch.ones(B, N, dtype=torch.bool)
    keep[torch.arange(B), t] = False
    lo = ((sc < ts - m) & keep).sum(1)
    hi = ((sc < ts + m) & keep).sum(1)
    exact = ((sc < ts) & keep).sum(1)
    assert bool((lo <= exact).all()) and bool((exact <= hi).all())
    better, ties = kg_rank_ops.rank_counts(q.cuda(), c.cuda(), t.cuda(), kind)
    better, ties = better.cpu(), ties.cpu()
    print(kind, "m", m, "max |better - exact|", int((better - exact).abs().max()), "ties", int(ties.sum()),
          "max hi - lo", int((hi - lo).max()))
    assert bool((lo <= better).all()) and bool((better <= hi).all())
    assert bool((lo <= better + ties).all()) and bool((better + ties <= hi).all())
