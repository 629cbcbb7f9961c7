"""CPU side of the kNN tool: the torch twin of the search kernels (the oracle of the GPU
tests), the parent torch composition behind ``use_kernels=False``, multi-file CLI input and
the k-means training-set cap."""
import numpy as np
import torch

from euler_amd.ops import knn_ops
from euler_amd.tools import knn


def _int_data(n, nq, d, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (n, d), generator=g), torch.randint(-4, 5, (nq, d), generator=g)


def _oracle_dist(q, x):
    q, x = q.long(), x.long()
    return (q * q).sum(1, keepdim=True) - 2 * (q @ x.t()) + (x * x).sum(1).unsqueeze(0)


def test_twin_matches_int64_oracle():
    x, q = _int_data(700, 33, 20)
    v, i = torch.sort(_oracle_dist(q, x), dim=1, stable=True)
    for k in (1, 10, 128, 200):  # 200 is past the kernels' limit: the twin serves it on any device
        D, I = knn_ops.flat_topk(q.float(), x.float(), k)
        assert torch.equal(D, v[:, :k].float()) and torch.equal(I, i[:, :k])
    assert torch.equal(knn_ops.nearest(q.float(), x.float()), i[:, 0])
    # every row identical: rows 0..k-1; fewer rows than k: padded with inf / -1
    D, I = knn_ops.flat_topk(q.float(), x[:1].expand(50, 20).float(), 10)
    assert torch.equal(I, torch.arange(10).expand(33, 10))
    D, I = knn_ops.flat_topk(q.float(), x[:4].float(), 6)
    assert torch.equal(I[:, :4], torch.sort(_oracle_dist(q, x[:4]), dim=1, stable=True)[1])
    assert bool((I[:, 4:] == -1).all()) and bool(torch.isinf(D[:, 4:]).all())


def test_twin_ivf_ties_on_original_rows():
    x, q = _int_data(300, 12, 8, seed=9)
    g = torch.Generator().manual_seed(2)
    assign = torch.randint(0, 5, (300,), generator=g)
    assign[assign == 3] = 4  # list 3 is empty
    list_ptr, row_of = knn_ops.build_lists(assign, 5)
    assert int(list_ptr[3]) == int(list_ptr[4]) and int(list_ptr[5]) == 300
    for l in range(5):  # stable: original order inside a list
        seg = row_of[list_ptr[l]:list_ptr[l + 1]]
        assert bool((assign[seg] == l).all()) and bool((seg[1:] > seg[:-1]).all())
    probe = torch.tensor([[0, 1, 2]] * 10 + [[3, -1, -1], [4, 3, 0]])
    D, I = knn_ops.ivf_topk(q.float(), x[row_of].float(), list_ptr, row_of, probe, 10)
    dist = _oracle_dist(q, x)
    for i in range(12):
        rows = torch.nonzero(torch.isin(assign, probe[i][probe[i] >= 0])).reshape(-1)
        o = torch.argsort(dist[i, rows], stable=True)[:10]
        assert torch.equal(I[i, :o.numel()], rows[o]) and torch.equal(D[i, :o.numel()], dist[i, rows[o]].float())
        assert bool((I[i, o.numel():] == -1).all()) and bool(torch.isinf(D[i, o.numel():]).all())
    assert bool((I[10] == -1).all())


def test_use_kernels_false_is_the_parent_composition():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(500, 16)).astype(np.float32)
    a, b = knn.FlatIndex(16, device="cpu"), knn.FlatIndex(16, device="cpu", use_kernels=False)
    a.add(x)
    b.add(x)
    xt = torch.from_numpy(x)
    v, i = torch.topk(knn._sqdist(xt[:9], xt), 5, dim=1, largest=False)
    for idx in (a, b):
        assert not idx.use_kernels
        D, I = idx.search(x[:9], 5)
        assert np.array_equal(D, v.numpy()) and np.array_equal(I, i.numpy())
    ivf_a = knn.build_index(x, "ivfflat", device="cpu")
    ivf_b = knn.build_index(x, "ivfflat", device="cpu", use_kernels=False)
    assert not ivf_a.use_kernels and torch.equal(ivf_a.cent, ivf_b.cent) and torch.equal(ivf_a.lists, ivf_b.lists)
    # the parent's assignment and padded table
    assign = knn._sqdist(xt, ivf_a.cent).argmin(1)
    assert torch.equal(ivf_a.assign, assign)
    for l in range(ivf_a.ncent):
        row = ivf_a.lists[l]
        assert torch.equal(row[row >= 0], torch.nonzero(assign == l).reshape(-1))
    Da, Ia = ivf_a.search(x[:9], 5)
    Db, Ib = ivf_b.search(x[:9], 5)
    assert np.array_equal(Da, Db) and np.array_equal(Ia, Ib) and (Ia[:, 0] == np.arange(9)).all()


def test_cli_concatenates_file_lists(tmp_path):
    rng = np.random.default_rng(4)
    emb = rng.normal(size=(300, 6)).astype(np.float32)
    ids = np.arange(5000, 5300)
    np.save(tmp_path / "e.npy", emb)
    np.save(tmp_path / "i.npy", ids)
    for r, (lo, hi) in enumerate([(0, 120), (120, 300)]):
        np.save(tmp_path / ("e%d.npy" % r), emb[lo:hi])
        np.save(tmp_path / ("i%d.npy" % r), ids[lo:hi])
    common = ["--index_type", "flat", "--k", "4", "--device", "cpu"]
    D1, I1 = knn.main(["--embedding_file", str(tmp_path / "e.npy"), "--id_file", str(tmp_path / "i.npy"),
                       "--out", str(tmp_path / "one.npz")] + common)
    D2, I2 = knn.main(["--embedding_file", "%s,%s" % (tmp_path / "e0.npy", tmp_path / "e1.npy"),
                       "--id_file", "%s,%s" % (tmp_path / "i0.npy", tmp_path / "i1.npy"),
                       "--out", str(tmp_path / "two.npz")] + common)
    assert np.array_equal(D1, D2) and np.array_equal(I1, I2)
    one, two = np.load(tmp_path / "one.npz"), np.load(tmp_path / "two.npz")
    assert np.array_equal(one["idx"], two["idx"]) and np.array_equal(one["distance"], two["distance"])


def test_max_points_per_centroid():
    rng = np.random.default_rng(6)
    x = rng.normal(size=(2000, 8)).astype(np.float32)
    full = knn.build_index(x, "ivfflat", device="cpu")
    same = knn.build_index(x, "ivfflat", device="cpu", max_points_per_centroid=None)
    assert full.ntrain == 2000 and same.ntrain == 2000
    assert torch.equal(full.cent, same.cent) and torch.equal(full.lists, same.lists)
    ncent = int(4 * np.sqrt(2000))
    capped = knn.build_index(x, "ivfflat", device="cpu", max_points_per_centroid=5)
    assert capped.ntrain <= 5 * ncent and capped.ntrain < 2000
    assert capped.ntotal == 2000
    _, I = capped.search(x[:20], 3)
    assert (I[:, 0] == np.arange(20)).all()
