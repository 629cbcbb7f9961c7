"""bf16 tables searched in place (csrc/hip/knn_bf16.hip) behind ops/knn_ops.py and tools/knn.py.

Exact data, as in test_knn_kernels.py: integers in [-4, 4] stored as bf16 with d <= 200, so
every norm, dot product and distance is an integer below 2^24, exact in bf16 inputs and in fp32
sums in any order.  The oracle is int64 arithmetic on the CPU under (distance, row); the
comparisons are ``torch.equal`` on D and I.

Widths (the flat scan stages 64 columns per chunk and takes 16 per MFMA): 3 is under one
16-byte vector and unaligned (scalar loads); 8 is one vector, half an MFMA step; 67 is a chunk
plus a tail with unaligned rows (scalar loads past the first chunk); 72 is a chunk plus a
padded tail with aligned rows; 200 is three chunks and a tail.  130 queries are past one query
tile of 128 (k <= 32) and of 64 (k = 128) and leave a tail.
"""
import functools

import numpy as np
import pytest
import torch

from euler_amd.ops import knn_ops
from euler_amd.ops._native import hip
from euler_amd.tools import knn

gpu = pytest.mark.gpu
N, DMAX, NQMAX, KMAX = 1000, 200, 130, 128
INF = float("inf")
BF = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _int_data():
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-4, 5, (N, DMAX), generator=g)
    q = torch.randint(-4, 5, (NQMAX, DMAX), generator=g)
    return x, q


def _oracle_dist(q, x):
    q, x = q.long(), x.long()
    return (q * q).sum(1, keepdim=True) - 2 * (q @ x.t()) + (x * x).sum(1).unsqueeze(0)


@functools.lru_cache(maxsize=None)
def _flat_oracle(d):
    x, q = _int_data()
    v, i = torch.sort(_oracle_dist(q[:, :d], x[:, :d]), dim=1, stable=True)
    return v[:, :KMAX].float(), i[:, :KMAX]


def _bf(t, device="cuda"):
    return t.to(BF).contiguous().to(device)


@gpu
@pytest.mark.parametrize("d", [3, 8, 67, 72, 200])
@pytest.mark.parametrize("nq", [1, 130])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_flat_scan_shapes(d, nq, k):
    x, q = _int_data()
    D, I = knn_ops.flat_topk(_bf(q[:nq, :d]), _bf(x[:, :d]), k)
    v, i = _flat_oracle(d)
    assert torch.equal(D.cpu(), v[:nq, :k])
    assert torch.equal(I.cpu(), i[:nq, :k])


@gpu
@pytest.mark.parametrize("k", [10, 128])
def test_splits_bit_identical(k):
    x, q = _int_data()
    xd, qd = _bf(x[:, :72]), _bf(q[:, :72])
    v, i = _flat_oracle(72)
    for s in (1, 3, 7):
        D, I = knn_ops.flat_topk(qd, xd, k, splits=s)
        assert torch.equal(D.cpu(), v[:, :k]), s
        assert torch.equal(I.cpu(), i[:, :k]), s


@gpu
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("k", [10, 128])
def test_identical_rows_return_first(splits, k):
    x, q = _int_data()
    same = x[:1, :8].expand(N, 8)
    D, I = knn_ops.flat_topk(_bf(q[:9, :8]), _bf(same), k, splits=splits)
    assert torch.equal(I.cpu(), torch.arange(k).expand(9, k))
    assert torch.equal(D.cpu(), _oracle_dist(q[:9, :8], x[:1, :8]).float().expand(9, k))


@gpu
def test_fewer_rows_than_k_pads():
    x, q = _int_data()
    D, I = knn_ops.flat_topk(_bf(q[:7, :72]), _bf(x[:5, :72]), 10)
    i = torch.sort(_oracle_dist(q[:7, :72], x[:5, :72]), dim=1, stable=True)[1]
    assert torch.equal(I[:, :5].cpu(), i) and bool((I[:, 5:] == -1).all()) and bool(torch.isinf(D[:, 5:]).all())


def _ivf_case(d):
    """n = 600 rows in 7 lists: list 0 empty, list 1 of 300 rows, list 2 of one row"""
    g = torch.Generator().manual_seed(11)
    x, q = _int_data()
    x, q = x[:600, :d], q[:40, :d]
    sizes = [0, 300, 1, 100, 90, 60, 49]
    assign = torch.cat([torch.full((s,), l) for l, s in enumerate(sizes)])[torch.randperm(600, generator=g)]
    probe = torch.stack([torch.randperm(7, generator=g)[:3] for _ in range(40)])
    probe[0] = torch.tensor([0, 2, -1])   # one row in all: the tail must be -1 / inf
    probe[1] = torch.tensor([-1, -1, -1])
    probe[2] = torch.tensor([1, 3, 4])
    return x, q, assign, probe


def _ivf_oracle(x, q, assign, probe, k):
    dist = _oracle_dist(q, x)
    D = torch.full((q.shape[0], k), INF)
    I = torch.full((q.shape[0], k), -1, dtype=torch.long)
    for i in range(q.shape[0]):
        rows = torch.nonzero(torch.isin(assign, probe[i][probe[i] >= 0])).reshape(-1)  # ascending rows
        o = torch.argsort(dist[i, rows], stable=True)[:k]
        D[i, :o.numel()] = dist[i, rows[o]].float()
        I[i, :o.numel()] = rows[o]
    return D, I


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
@pytest.mark.parametrize("d", [3, 72])
def test_ivf_scan(d, device):
    """on the CPU this is the twin's bf16 branch"""
    x, q, assign, probe = _ivf_case(d)
    list_ptr, row_of = knn_ops.build_lists(assign, 7)
    xs = _bf(x[row_of], device)
    assert xs.dtype == BF
    D, I = knn_ops.ivf_topk(_bf(q, device), xs, list_ptr.to(device), row_of.to(device), probe.to(device), 10)
    Do, Io = _ivf_oracle(x, q, assign, probe, 10)
    assert torch.equal(D.cpu(), Do) and torch.equal(I.cpu(), Io)
    assert bool((I[0, 1:] == -1).all()) and bool((I[1] == -1).all())


def test_flat_twin_on_cpu():
    x, q = _int_data()
    D, I = knn_ops.flat_topk(q[:, :72].float(), _bf(x[:, :72], "cpu"), 10)  # fp32 queries are rounded to bf16
    v, i = _flat_oracle(72)
    assert torch.equal(D, v[:, :10]) and torch.equal(I, i[:, :10])


@gpu
@pytest.mark.parametrize("d", [3, 200])
def test_row_norms(d):
    x, _ = _int_data()
    got = hip().knn_bf16.row_norms(_bf(x[:, :d]))
    assert torch.equal(got.cpu(), (x[:, :d] * x[:, :d]).sum(1).float())


@gpu
def test_rounding_on_real_valued_data():
    """B(q, x) = 2 (d + 3) 2^-24 (||q|| + ||x||)^2: products of bf16 values are exact in fp32,
    the three sums (||x||^2, q.x, ||q||^2) have at most d terms each with unit roundoff 2^-24."""
    g = torch.Generator().manual_seed(3)
    d, k = 128, 10
    x = torch.randn(1000, d, generator=g).to(BF)
    q = torch.randn(64, d, generator=g).to(BF)
    D, I = knn_ops.flat_topk(q.cuda(), x.cuda(), k)
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


@gpu
def test_bindings_take_bf16_and_refuse_fp32():
    x, q = _int_data()
    xb, qb = _bf(x[:, :72]), _bf(q[:9, :72])
    xn = (x[:, :72] * x[:, :72]).sum(1).float().cuda()
    pd, pr = hip().knn_bf16.flat_scan(qb, xb, xn, 10, 2)
    assert pd.shape == (9, 2, 10) and pd.dtype == torch.float32 and pr.dtype == torch.int64
    lp, ro = torch.tensor([0, N]).cuda(), torch.arange(N).cuda()
    pd, pr = hip().knn_bf16.ivf_scan(qb, xb, xn, lp, ro, torch.zeros(9, 1, dtype=torch.long).cuda(), 10)
    v, i = _flat_oracle(72)
    assert torch.equal(pr[:, 0].cpu(), i[:9, :10])
    with pytest.raises(RuntimeError, match="knn_flat_scan_bf16: x has dtype"):
        hip().knn_bf16.flat_scan(qb, xb.float(), xn, 10, 2)
    with pytest.raises(RuntimeError, match="knn_ivf_scan_bf16: q has dtype"):
        hip().knn_bf16.ivf_scan(qb.float(), xb, xn, lp, ro, torch.zeros(9, 1, dtype=torch.long).cuda(), 10)


@gpu
def test_indexes_store_bf16():
    x, q = _int_data()
    x, q = x[:600, :72], q[:40, :72]
    flat = knn.FlatIndex(72, device="cuda", dtype=BF)
    flat.add(x.float().numpy())  # host fp32 input, converted in row chunks
    assert flat.xb.dtype == BF
    D, I = flat.search(q.float().numpy(), 10)
    v, i = torch.sort(_oracle_dist(q, x), dim=1, stable=True)
    assert np.array_equal(D, v[:, :10].float().numpy()) and np.array_equal(I, i[:, :10].numpy())
    cent = torch.cat([x[[5, 17, 100, 250, 17, 400]], torch.full((1, 72), 50)])  # one duplicate, one far away
    ivf = knn.IVFFlatIndex(72, 7, nprobe=3, device="cuda", dtype=BF)
    ivf.cent = cent.float().cuda()
    given = _bf(x)
    ivf.add(given)
    assert ivf.xb.data_ptr() == given.data_ptr() and ivf.xs.dtype == BF
    assign = torch.sort(_oracle_dist(x, cent), dim=1, stable=True)[1][:, 0]
    assert torch.equal(ivf.assign.cpu(), assign)
    probe = torch.sort(_oracle_dist(q, cent), dim=1, stable=True)[1][:, :3]
    D, I = ivf.search(q.float().numpy(), 10)
    Do, Io = _ivf_oracle(x, q, assign, probe, 10)
    assert np.array_equal(D, Do.numpy()) and np.array_equal(I, Io.numpy())


@gpu
def test_add_and_search_make_no_fp32_copy():
    """partials 64 * S (<= 64) * 10 * 12 B < 0.5 MB, norms 0.8 MB, queries and results under
    0.1 MB: under 2 MB against the 51.2 MB bound, which is half an fp32 copy"""
    n, d = 200_000, 128
    g = torch.Generator().manual_seed(5)
    table = torch.randn(n, d, generator=g).to(BF).cuda()
    q = torch.randn(64, d, generator=g).numpy()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    idx = knn.FlatIndex(d, device="cuda", dtype=BF)
    idx.add(table)
    D, I = idx.search(q, 10)
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise over the table: %.2f MB" % (rise / 2 ** 20))
    assert idx.xb.data_ptr() == table.data_ptr()
    assert rise < n * d * 2, rise
    assert D.shape == (64, 10) and bool((np.diff(D, axis=1) >= 0).all()) and bool((I >= 0).all())
