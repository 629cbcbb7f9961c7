"""Fused distance + top-k kernels (csrc/hip/knn.hip) behind ops/knn_ops.py and tools/knn.py.

Exact data: embeddings and queries are integers in [-4, 4] stored as fp32 with d <= 200, so
every norm, dot product and distance is an integer below 2^24 and exact in fp32 in any
summation order.  The oracle is int64 arithmetic on the CPU under the ordering rule
(distance, then original row) and the comparisons are ``torch.equal`` on D and I.
"""
import functools

import numpy as np
import pytest
import torch

from euler_amd.ops import knn_ops
from euler_amd.tools import knn

pytestmark = pytest.mark.gpu

N, DMAX, NQMAX, KMAX = 1000, 200, 130, 128
INF = float("inf")


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
    """sorted (distance, row) of every query against every row, computed once per width"""
    x, q = _int_data()
    v, i = torch.sort(_oracle_dist(q[:, :d], x[:, :d]), dim=1, stable=True)
    return v[:, :KMAX].float(), i[:, :KMAX]


def _dev(t):
    return t.float().contiguous().cuda()


@pytest.mark.parametrize("d", [4, 20, 128, 200])
@pytest.mark.parametrize("nq", [1, 7, 130])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_flat_scan_shapes(d, nq, k):
    x, q = _int_data()
    D, I = knn_ops.flat_topk(_dev(q[:nq, :d]), _dev(x[:, :d]), k)
    v, i = _flat_oracle(d)
    assert torch.equal(D.cpu(), v[:nq, :k])
    assert torch.equal(I.cpu(), i[:nq, :k])


def test_flat_index_fewer_rows_than_k():
    x, q = _int_data()
    idx = knn.FlatIndex(20, device="cuda")
    idx.add(x[:5, :20].float().numpy())
    D, I = idx.search(q[:7, :20].float().numpy(), 10)
    v, i = torch.sort(_oracle_dist(q[:7, :20], x[:5, :20]), dim=1, stable=True)
    assert D.shape == (7, 5) and I.shape == (7, 5)
    assert np.array_equal(D, v.float().numpy()) and np.array_equal(I, i.numpy())
    # the op itself pads to k columns
    D, I = knn_ops.flat_topk(_dev(q[:7, :20]), _dev(x[:5, :20]), 10)
    assert torch.equal(I[:, :5].cpu(), i) and bool((I[:, 5:] == -1).all()) and bool(torch.isinf(D[:, 5:]).all())


@pytest.mark.parametrize("k", [10, 128])
def test_splits_bit_identical(k):
    x, q = _int_data()
    xd, qd = _dev(x[:, :128]), _dev(q[:, :128])
    v, i = _flat_oracle(128)
    for s in (1, 3, 7):
        D, I = knn_ops.flat_topk(qd, xd, k, splits=s)
        assert torch.equal(D.cpu(), v[:, :k]), s
        assert torch.equal(I.cpu(), i[:, :k]), s


@pytest.mark.parametrize("splits", [1, 3, 7])
@pytest.mark.parametrize("k", [10, 128])
def test_identical_rows_return_first(splits, k):
    x, q = _int_data()
    same = x[:1, :20].expand(N, 20)
    D, I = knn_ops.flat_topk(_dev(q[:9, :20]), _dev(same), k, splits=splits)
    assert torch.equal(I.cpu(), torch.arange(k).expand(9, k))
    assert torch.equal(D.cpu(), _oracle_dist(q[:9, :20], x[:1, :20]).float().expand(9, k))


def _ivf_case(d):
    """n = 600 rows in 7 lists: list 0 empty, list 1 of 300 rows, list 2 of one row"""
    g = torch.Generator().manual_seed(11)
    x, q = _int_data()
    x, q = x[:600, :d], q[:40, :d]
    sizes = [0, 300, 1, 100, 90, 60, 49]
    assign = torch.cat([torch.full((s,), l) for l, s in enumerate(sizes)])[torch.randperm(600, generator=g)]
    probe = torch.stack([torch.randperm(7, generator=g)[:3] for _ in range(40)])
    probe[torch.rand(40, 3, generator=g) < 0.2] = -1
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


@pytest.mark.parametrize("d", [20, 128])
def test_ivf_scan(d):
    x, q, assign, probe = _ivf_case(d)
    list_ptr, row_of = knn_ops.build_lists(assign, 7)
    assert list_ptr.tolist() == [0, 0, 300, 301, 401, 491, 551, 600]
    xs = x[row_of].float()
    D, I = knn_ops.ivf_topk(_dev(q), xs.cuda(), list_ptr.cuda(), row_of.cuda(), probe.cuda(), 10)
    Do, Io = _ivf_oracle(x, q, assign, probe, 10)
    Dt, It = knn_ops.ivf_topk(q.float(), xs, list_ptr, row_of, probe, 10)  # the torch twin
    assert torch.equal(Dt, Do) and torch.equal(It, Io)
    assert torch.equal(D.cpu(), Do) and torch.equal(I.cpu(), Io)
    assert I[0, 0].item() >= 0 and bool((I[0, 1:] == -1).all()) and bool(torch.isinf(D[0, 1:]).all())
    assert bool((I[1] == -1).all())


def test_ivf_index_explicit_centroids():
    """tools path without k-means: integer centroids, one far away (its list stays empty) and
    one duplicated (the assignment goes to the lower index)"""
    x, q = _int_data()
    x, q = x[:600, :20], q[:40, :20]
    cent = x[[5, 17, 100, 250, 17, 400]].clone()
    cent = torch.cat([cent, torch.full((1, 20), 50)])
    idx = knn.IVFFlatIndex(20, 7, nprobe=3, device="cuda")
    idx.cent = _dev(cent)
    idx.add(x.float().numpy())
    assign = torch.sort(_oracle_dist(x, cent), dim=1, stable=True)[1][:, 0]
    assert torch.equal(idx.assign.cpu(), assign)
    assert int((assign == 4).sum()) == 0 and int((assign == 6).sum()) == 0
    probe = torch.sort(_oracle_dist(q, cent), dim=1, stable=True)[1][:, :3]
    D, I = idx.search(q.float().numpy(), 10)
    Do, Io = _ivf_oracle(x, q, assign, probe, 10)
    assert np.array_equal(D, Do.numpy()) and np.array_equal(I, Io.numpy())


def test_nearest_lowest_index_among_equals():
    x, q = _int_data()
    cent = x[:20, :20].clone()
    cent[10] = cent[3]
    cent[15] = cent[3]
    pts = torch.cat([x[:300, :20], cent])  # the centroids themselves: distance 0 to all copies
    got = knn_ops.nearest(_dev(pts), _dev(cent))
    want = torch.sort(_oracle_dist(pts, cent), dim=1, stable=True)[1][:, 0]
    assert torch.equal(got.cpu(), want)
    assert got[300 + 10].item() == 3 and got[300 + 15].item() == 3


def test_more_query_tiles_than_the_grid_cap():
    """600 000 queries are 4688 tiles of 128, more than the 4096 blocks a launch gets: the
    blocks loop over work items and reuse their LDS lists"""
    g = torch.Generator().manual_seed(13)
    pts = torch.randint(-4, 5, (600_000, 4), generator=g)
    cent = torch.randint(-4, 5, (50, 4), generator=g)
    got = knn_ops.nearest(_dev(pts), _dev(cent))
    dist = _oracle_dist(pts, cent)
    lowest = torch.where(dist == dist.min(1, keepdim=True)[0], torch.arange(50), torch.tensor(50)).min(1)[0]
    assert torch.equal(got.cpu(), lowest)


def test_rounding_on_real_valued_data():
    """tol = 1e-5 (||q||^2 + max ||x||^2): about 50 times the fp32 bound of an fmaf chain
    (<= 1.5e-7 sum |q_i x_i| for the dot, plus three roundings of the sum); derived, not
    measured.  Every query and every returned row is held to it."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4000, 128, generator=g)
    q = torch.randn(64, 128, generator=g)
    D, I = knn_ops.flat_topk(q.cuda(), x.cuda(), 10)
    D, I = D.cpu().double(), I.cpu()
    assert bool((I >= 0).all()) and all(len(set(r)) == 10 for r in I.tolist())
    xd, qd = x.double(), q.double()
    ref = (qd * qd).sum(1, keepdim=True) - 2 * (qd @ xd.t()) + (xd * xd).sum(1).unsqueeze(0)
    tol = 1e-5 * ((qd * qd).sum(1) + (xd * xd).sum(1).max()).unsqueeze(1)
    of_returned = torch.gather(ref, 1, I)
    kth = torch.sort(ref, dim=1)[0][:, 9:10]
    print("max |D - ref|", float((D - of_returned).abs().max()), "min tol", float(tol.min()),
          "max excess over k-th", float((of_returned - kth).max()))
    assert bool(((D - of_returned).abs() <= tol).all())
    assert bool((of_returned <= kth + tol).all())


def test_search_allocates_no_distance_matrix():
    """[8192, 200000] fp32 would be 6.5 GB; the partials are nq * S * k * 12 bytes"""
    g = torch.Generator().manual_seed(5)
    idx = knn.FlatIndex(16, device="cuda")
    idx.add(torch.randn(200_000, 16, generator=g).numpy())
    q = torch.randn(8192, 16, generator=g).numpy()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    D, I = idx.search(q, 10)
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise during search: %.1f MB" % (rise / 2 ** 20))
    assert rise < 512 * 2 ** 20, rise
    assert D.shape == (8192, 10) and bool((np.diff(D, axis=1) >= 0).all()) and bool((I >= 0).all())


def test_flat_index_gpu_equals_cpu():
    x, q = _int_data()
    xn, qn = x[:, :128].float().numpy(), q[:, :128].float().numpy()
    gpu, cpu = knn.build_index(xn, "flat", device="cuda"), knn.FlatIndex(128, device="cpu")
    cpu.add(xn)
    Dg, Ig = gpu.search(qn, 10)
    Dc, Ic = cpu.search(qn, 10)
    v, i = _flat_oracle(128)
    assert np.array_equal(Dg, Dc)  # distances are exact on both; the CPU top-k leaves ties unordered
    assert np.array_equal(Dg, v[:, :10].numpy()) and np.array_equal(Ig, i[:, :10].numpy())
    assert np.array_equal(np.take_along_axis(_oracle_dist(q[:, :128], x[:, :128]).numpy(), Ic, 1), Dc.astype(np.int64))


def test_ivf_recall_and_determinism():
    rng = np.random.default_rng(1)
    centers = rng.normal(size=(20, 8)) * 10
    x = (centers[rng.integers(0, 20, 4000)] + rng.normal(size=(4000, 8))).astype(np.float32)
    ivf = knn.build_index(x, "ivfflat", device="cuda")
    flat = knn.build_index(x, "flat", device="cuda")
    D1, I = ivf.search(x[:50], 10)
    D2, I2 = ivf.search(x[:50], 10)
    E1, J = flat.search(x[:50], 10)
    E2, J2 = flat.search(x[:50], 10)
    assert np.array_equal(D1, D2) and np.array_equal(I, I2)
    assert np.array_equal(E1, E2) and np.array_equal(J, J2)
    recall = np.mean([len(set(a) & set(b)) / 10.0 for a, b in zip(I, J)])
    assert recall > 0.9, recall
