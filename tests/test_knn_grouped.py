"""The list-grouped IVF search (csrc/hip/knn_grouped.hip): ``ivf_topk(..., schedule="list")``.

Exact data, as in test_knn_kernels.py / test_knn_bf16.py: integers in [-4, 4] with d <= 200, so
every score is an integer below 2^24, exact in fp32 and in bf16 inputs in any summation order.
The oracle is int64 arithmetic on the CPU under (distance, row); comparisons are ``torch.equal``.

Widths (rows are staged 128 bytes per chunk: 64 bf16 or 32 fp32 columns): 3 is under one 16-byte
vector and unaligned (scalar loads), 21 is unaligned with whole units and a partial one, 72 is a chunk plus a padded tail (bf16) or two and a tail
(fp32), 200 is several chunks.  TQ = ``knn_ops.LIST_TQ`` queries share a work item.
"""
import functools

import numpy as np
import pytest
import torch

from euler_amd.ops import knn_ops
from euler_amd.ops._native import hip
from euler_amd.tools import knn

gpu = pytest.mark.gpu
TQ = knn_ops.LIST_TQ
NQ, DMAX, KMAX, NCENT = TQ + 6, 200, 128, 8
SIZES = [0, 300, 1, 100, 90, 60, 49, 40]  # list 0 empty, list 1 over two row tiles, list 2 of one row
INF = float("inf")
DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _case():
    """640 rows in 8 lists and TQ + 6 queries probing 3 lists each.  List 1 is probed by the first
    TQ + 1 queries (two query tiles, the second of one query), list 3 by query 5 alone, list 7 by
    nobody; lists 0 (empty) and 2 (one row) are probed by many."""
    g = torch.Generator().manual_seed(11)
    n = sum(SIZES)
    x = torch.randint(-4, 5, (n, DMAX), generator=g)
    q = torch.randint(-4, 5, (NQ, DMAX), generator=g)
    assign = torch.cat([torch.full((s,), l) for l, s in enumerate(SIZES)])[torch.randperm(n, generator=g)]
    probe = torch.tensor([[1, 4 + i % 3, (0, 2)[i % 2]] for i in range(NQ)])
    probe[1] = torch.tensor([1, -1, 4])        # -1 in the middle
    probe[5, 1] = 3
    probe[TQ + 1] = torch.tensor([-1, -1, -1])
    probe[TQ + 2] = torch.tensor([0, 2, -1])   # one row in all: the tail must be inf / -1
    probe[TQ + 3] = torch.tensor([9, 6, 5])    # 9 is no list
    probe[TQ + 4] = torch.tensor([4, 5, 6])
    probe[TQ + 5] = torch.tensor([6, 2, 0])
    return x, q, assign, probe


def _oracle(x, q, assign, probe, k):
    q, x = q.long(), x.long()
    dist = (q * q).sum(1, keepdim=True) - 2 * (q @ x.t()) + (x * x).sum(1).unsqueeze(0)
    D = torch.full((q.shape[0], k), INF)
    I = torch.full((q.shape[0], k), -1, dtype=torch.long)
    for i in range(q.shape[0]):
        rows = torch.nonzero(torch.isin(assign, probe[i][probe[i] >= 0])).reshape(-1)  # ascending rows
        o = torch.argsort(dist[i, rows], stable=True)[:k]
        D[i, :o.numel()] = dist[i, rows[o]].float()
        I[i, :o.numel()] = rows[o]
    return D, I


@functools.lru_cache(maxsize=None)
def _case_oracle(d):
    x, q, assign, probe = _case()
    return _oracle(x[:, :d], q[:, :d], assign, probe, KMAX)


def _search(x, q, assign, probe, k, dtype, device, ncent=NCENT, **kw):
    list_ptr, row_of = knn_ops.build_lists(assign, ncent)
    xs = x[row_of].to(dtype).contiguous().to(device)
    return knn_ops.ivf_topk(q.to(dtype).to(device), xs, list_ptr.to(device), row_of.to(device), probe.to(device), k,
                            **kw)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [3, 21, 72, 200])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_list_schedule_shapes(dtype, d, k):
    x, q, assign, probe = _case()
    D, I = _search(x[:, :d], q[:, :d], assign, probe, k, dtype, "cuda", schedule="list")
    Do, Io = _case_oracle(d)
    assert torch.equal(D.cpu(), Do[:, :k]) and torch.equal(I.cpu(), Io[:, :k])
    assert bool((I[TQ + 1] == -1).all()) and bool((I[TQ + 2, 1:] == -1).all()) and bool(torch.isinf(D[TQ + 2, 1:]).all())


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_query_tile_too_wide_for_lds_is_staged(dtype):
    """d = 1100 (2200 / 4400 bytes a row) is past the resident query tile at any k: the query chunk
    is re-gathered with every row tile.  Scores stay integers below 2^24 (|q.x| <= 16 * 1100)."""
    x, q, assign, probe = _case()
    x, q = x.repeat(1, 6)[:, :1100], q.repeat(1, 6)[:, :1100]
    D, I = _search(x, q, assign, probe, 10, dtype, "cuda", schedule="list")
    Do, Io = _oracle(x, q, assign, probe, 10)
    assert torch.equal(D.cpu(), Do) and torch.equal(I.cpu(), Io)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [10, 128])
def test_identical_rows_return_lowest_rows(dtype, k):
    """a list of 300 equal rows (over two row tiles) probed by TQ + 1 queries (two query tiles)"""
    x, q, assign, _ = _case()
    same = x[:1, :8].expand(x.shape[0], 8)
    probe = torch.ones(TQ + 1, 1, dtype=torch.long)
    D, I = _search(same, q[:TQ + 1, :8], assign, probe, k, dtype, "cuda", schedule="list")
    Do, Io = _oracle(same, q[:TQ + 1, :8], assign, probe, k)
    assert torch.equal(Io, torch.nonzero(assign == 1).reshape(-1)[:k].expand(TQ + 1, k))
    assert torch.equal(D.cpu(), Do) and torch.equal(I.cpu(), Io)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_run_to_run_and_grouping_independence(dtype):
    _, _, assign, probe = _case()
    g = torch.Generator().manual_seed(5)
    x, q = torch.randn(assign.numel(), 72, generator=g), torch.randn(NQ, 72, generator=g)
    D1, I1 = _search(x, q, assign, probe, 10, dtype, "cuda", schedule="list")
    D2, I2 = _search(x, q, assign, probe, 10, dtype, "cuda", schedule="list")
    assert torch.equal(D1, D2) and torch.equal(I1, I2)
    h = NQ // 2
    halves = [_search(x, q[s], assign, probe[s], 10, dtype, "cuda", schedule="list") for s in (slice(0, h), slice(h, NQ))]
    assert torch.equal(D1, torch.cat([halves[0][0], halves[1][0]]))
    assert torch.equal(I1, torch.cat([halves[0][1], halves[1][1]]))


@gpu
@pytest.mark.parametrize("schedule", ["query", "list"])
def test_rounding_on_real_valued_data(schedule):
    """the check and the bound of test_knn_bf16.py::test_rounding_on_real_valued_data, every list probed:
    B(q, x) = 2 (d + 3) 2^-24 (||q|| + ||x||)^2"""
    g = torch.Generator().manual_seed(3)
    d, k = 128, 10
    x = torch.randn(1000, d, generator=g).to(torch.bfloat16)
    q = torch.randn(64, d, generator=g).to(torch.bfloat16)
    assign = torch.randint(0, NCENT, (1000,), generator=g)
    probe = torch.stack([torch.randperm(NCENT, generator=g) for _ in range(64)])
    D, I = _search(x, q, assign, probe, k, torch.bfloat16, "cuda", schedule=schedule)
    D, I = D.cpu().double(), I.cpu()
    assert bool((I >= 0).all()) and all(len(set(r)) == k for r in I.tolist())
    xd, qd = x.double(), q.double()
    ref = (qd * qd).sum(1, keepdim=True) - 2 * (qd @ xd.t()) + (xd * xd).sum(1).unsqueeze(0)
    B = 2 * (d + 3) * 2.0 ** -24 * (qd.norm(dim=1).unsqueeze(1) + xd.norm(dim=1).unsqueeze(0)) ** 2
    of_returned, b_returned = torch.gather(ref, 1, I), torch.gather(B, 1, I)
    top = torch.sort(ref, dim=1)[0][:, :k]
    print("max |D - ref| / B", float(((D - of_returned).abs() / b_returned).max()),
          "max |sorted D - top k| / B", float(((D - top).abs() / b_returned).max()))
    assert bool(((D - of_returned).abs() <= b_returned).all())
    assert bool(((D - top).abs() <= b_returned).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_list_schedule_on_cpu_is_the_twin(dtype):
    x, q, assign, probe = _case()
    D, I = _search(x[:, :72], q[:, :72], assign, probe, 10, dtype, "cpu", schedule="list")
    Do, Io = _case_oracle(72)
    assert torch.equal(D, Do[:, :10]) and torch.equal(I, Io[:, :10])
    with pytest.raises(ValueError, match="query | list"):
        _search(x[:, :72], q[:, :72], assign, probe, 10, dtype, "cpu", schedule="bogus")


def test_index_and_cli_take_the_schedule(tmp_path):
    """on the CPU the "list" index runs the ops' twin, the default one the torch composition: the same
    neighbours, distances up to fp32 rounding"""
    x = torch.randn(300, 6, generator=torch.Generator().manual_seed(4))
    a = knn.IVFFlatIndex(6, 5, nprobe=2, device="cpu", schedule="list")
    b = knn.IVFFlatIndex(6, 5, nprobe=2, device="cpu")
    for idx in (a, b):
        idx.train(x)
        idx.add(x)
    (Da, Ia), (Db, Ib) = a.search(x[:9], 4), b.search(x[:9], 4)
    assert np.array_equal(Ia, Ib) and np.allclose(Da, Db, atol=1e-5) and (Ia[:, 0] == np.arange(9)).all()
    with pytest.raises(ValueError, match="query | list"):
        knn.IVFFlatIndex(6, 5, schedule="auto")
    np.save(tmp_path / "e.npy", x.numpy())
    common = ["--embedding_file", str(tmp_path / "e.npy"), "--k", "4", "--device", "cpu"]
    D1, I1 = knn.main(common + ["--out", str(tmp_path / "l.npz"), "--ivf_schedule", "list"])
    D2, I2 = knn.main(common + ["--out", str(tmp_path / "q.npz")])
    assert np.array_equal(I1, I2) and np.allclose(D1, D2, atol=1e-5) and (I1[:, 0] == np.arange(25)).all()


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
def test_list_index_without_kernels_launches_none(device, monkeypatch):
    """use_kernels=False with schedule="list": torch probe selection and the ops' twin on any device; the
    neighbours of the torch composition of a default use_kernels=False index"""
    def no_kernels():
        raise AssertionError("use_kernels=False reached the HIP ops")

    monkeypatch.setattr(knn_ops, "hip", no_kernels)
    x = torch.randn(300, 6, generator=torch.Generator().manual_seed(4))
    a = knn.IVFFlatIndex(6, 5, nprobe=2, device=device, use_kernels=False, schedule="list")
    b = knn.IVFFlatIndex(6, 5, nprobe=2, device=device, use_kernels=False)
    for idx in (a, b):
        idx.train(x)
        idx.add(x)
    (Da, Ia), (Db, Ib) = a.search(x[:40], 4), b.search(x[:40], 4)
    assert np.array_equal(Ia, Ib) and np.allclose(Da, Db, atol=1e-5) and (Ia[:, 0] == np.arange(40)).all()


@gpu
def test_bindings_refuse_bad_operands_by_name():
    x, q, assign, probe = _case()
    grouped = hip().knn_grouped
    assert grouped.tq == TQ
    list_ptr, row_of = (t.cuda() for t in knn_ops.build_lists(assign, NCENT))
    xs, qd, pc = x[row_of.cpu(), :72].float().cuda(), q[:, :72].float().cuda(), probe.cuda()
    xn = (xs * xs).sum(1)

    def run():
        qptr, pairs, items, n_items, pd, pr = grouped.invert(pc, NCENT, 10)
        grouped.scan(qd, xs, xn, list_ptr, row_of, qptr, pairs, items, n_items, pd, pr)
        return (qptr, pairs, items, n_items), pd, pr

    table, pd, pr = run()
    assert pd.shape == (NQ, 3, 10) and pd.dtype == torch.float32 and pr.dtype == torch.int64
    assert int(table[0][-1]) == int(((probe >= 0) & (probe < NCENT)).sum()) and int(table[3]) == 8
    with pytest.raises(RuntimeError, match="knn_grouped_invert: probe has dtype"):
        grouped.invert(pc.int(), NCENT, 10)
    with pytest.raises(RuntimeError, match="knn_grouped_invert: probe must be a GPU tensor"):
        grouped.invert(probe, NCENT, 10)
    with pytest.raises(RuntimeError, match="knn_grouped_invert: probe must be contiguous"):
        grouped.invert(pc.t().contiguous().t(), NCENT, 10)
    with pytest.raises(RuntimeError, match="knn_grouped_scan: q has dtype"):
        grouped.scan(qd.bfloat16(), xs, xn, list_ptr, row_of, *table, pd.clone(), pr.clone())
    with pytest.raises(RuntimeError, match="knn_grouped_scan: xn must be a GPU tensor"):
        grouped.scan(qd, xs, xn.cpu(), list_ptr, row_of, *table, pd.clone(), pr.clone())
    _, pd2, pr2 = run()
    assert torch.equal(pd, pd2) and torch.equal(pr, pr2)
