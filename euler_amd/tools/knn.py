"""k-nearest-neighbour retrieval over inferred embeddings (reference ``knn/knn.py``).

The reference wraps faiss ``IndexIVFFlat`` (``ncent = 4 * sqrt(n)``, ``nprobe = 10``,
L2).  faiss is not available here; this module implements the same two index types
directly on torch tensors:

* :class:`FlatIndex` — exact search, ``||q||^2 - 2 q.x + ||x||^2`` in query chunks;
* :class:`IVFFlatIndex` — Lloyd k-means coarse quantiser, inverted lists, search over the
  ``nprobe`` closest lists.

On GPU tensors the k-means assignment, the coarse assignment, the probe selection and the
searches run the fused distance + top-k kernels of ``euler_amd.ops.knn_ops`` (``k <= 128``;
no distance matrix is allocated, equal distances go to the lower row, the inverted lists
are a CSR).  CPU tensors, and ``use_kernels=False`` on any device, take the torch
composition: GEMMs through ``torch.matmul``, ``torch.topk`` selections, padded lists.

CLI (same flags as the reference)::

    python -m euler_amd.tools.knn --embedding_file embedding_0.npy --id_file ids_0.npy \
        [--query_file q.csv] [--index_type ivfflat|flat] [--k 10] [--out result.npz]

``--embedding_file`` / ``--id_file`` also take comma-separated lists of equal length (the
per-rank files of a multi-rank ``infer()``), concatenated in order.

(the reference read the ids from ``embedding_file`` by mistake and pickled the result;
here ids come from ``id_file`` and the result is an ``.npz`` with ``distance`` / ``idx``.)
"""
from __future__ import annotations

import argparse
import math

import numpy as np
import torch

from euler_amd.ops import knn_ops

__all__ = ["FlatIndex", "IVFFlatIndex", "build_index", "kmeans"]


def _dev(device):
    if device is not None:
        return torch.device(device)
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


def _sqdist(q, x, x_norm=None):
    """squared L2 distances [nq, nx]"""
    qn = (q * q).sum(1, keepdim=True)
    xn = (x * x).sum(1) if x_norm is None else x_norm
    return (qn - 2.0 * (q @ x.t()) + xn.unsqueeze(0)).clamp_min_(0.0)


def _kernels(use_kernels, device):
    """the fused kernels serve GPU tensors unless ``use_kernels`` is False"""
    return use_kernels is not False and torch.device(device).type == "cuda"


class FlatIndex:
    def __init__(self, d, device=None, chunk=8192, use_kernels=None):
        self.d, self.device, self.chunk = d, _dev(device), chunk
        self.use_kernels = _kernels(use_kernels, self.device)
        self.xb = torch.zeros(0, d, device=self.device)
        self.xn = torch.zeros(0, device=self.device)

    def add(self, x):
        x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
        self.xb = torch.cat([self.xb, x])
        self.xn = (self.xb * self.xb).sum(1)

    @property
    def ntotal(self):
        return self.xb.shape[0]

    def search(self, q, k):
        q = torch.as_tensor(q, dtype=torch.float32, device=self.device)
        k = min(int(k), self.ntotal)
        ds, ids = [], []
        for s in range(0, q.shape[0], self.chunk):
            if self.use_kernels and 1 <= k <= knn_ops.MAX_KERNEL_K:
                # query chunks only bound the partial lists; no [chunk, ntotal] matrix
                v, i = knn_ops.flat_topk(q[s:s + self.chunk], self.xb, k, xn=self.xn)
                ds.append(v)
                ids.append(i)
                continue
            d = _sqdist(q[s:s + self.chunk], self.xb, self.xn)
            v, i = torch.topk(d, k, dim=1, largest=False)
            ds.append(v)
            ids.append(i)
        return torch.cat(ds).cpu().numpy(), torch.cat(ids).cpu().numpy()


def _assign(x, cent, use_kernels):
    if _kernels(use_kernels, x.device):
        return knn_ops.nearest(x, cent)
    return torch.cat([_sqdist(x[s:s + 65536], cent).argmin(1) for s in range(0, x.shape[0], 65536)])


def kmeans(x, ncent, iters=20, seed=0, min_points_per_centroid=4, use_kernels=None):
    """Lloyd k-means on the device; empty clusters are re-seeded from random points."""
    n = x.shape[0]
    ncent = max(1, min(int(ncent), n // max(min_points_per_centroid, 1) or 1))
    g = torch.Generator(device="cpu").manual_seed(seed)
    cent = x[torch.randperm(n, generator=g)[:ncent].to(x.device)].clone()
    for _ in range(iters):
        assign = _assign(x, cent, use_kernels)
        sums = torch.zeros_like(cent).index_add_(0, assign, x)
        cnt = torch.bincount(assign, minlength=ncent).to(x.dtype)
        empty = cnt == 0
        cent = torch.where(empty.unsqueeze(1), cent, sums / cnt.clamp_min(1).unsqueeze(1))
        if bool(empty.any()):
            ridx = torch.randint(0, n, (int(empty.sum()),), generator=g).to(x.device)
            cent[empty] = x[ridx]
    return cent


class IVFFlatIndex:
    def __init__(self, d, ncent, nprobe=10, device=None, min_points_per_centroid=4, iters=20, use_kernels=None):
        self.d, self.ncent, self.nprobe = d, int(ncent), int(nprobe)
        self.device = _dev(device)
        self.use_kernels = _kernels(use_kernels, self.device)
        self.min_pts, self.iters = min_points_per_centroid, iters
        self.cent = None
        self.xb = None
        self.lists = None
        self.ntrain = 0

    def train(self, x):
        x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
        self.ntrain = x.shape[0]
        self.cent = kmeans(x, self.ncent, self.iters, min_points_per_centroid=self.min_pts,
                           use_kernels=self.use_kernels)
        self.ncent = self.cent.shape[0]

    def add(self, x):
        x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
        self.xb = x if self.xb is None else torch.cat([self.xb, x])
        self.assign = _assign(self.xb, self.cent, self.use_kernels)
        self.xn = (self.xb * self.xb).sum(1)
        if self.use_kernels:
            # CSR inverted lists: the database in list order, original order kept inside a list
            self.list_ptr, self.row_of = knn_ops.build_lists(self.assign, self.ncent)
            self.xs, self.xns = self.xb[self.row_of], self.xn[self.row_of]
            self.maxl = int((self.list_ptr[1:] - self.list_ptr[:-1]).max())
            self.lists = None
        else:
            self._pad_lists()

    def _pad_lists(self):
        """the torch composition's padded [ncent, longest list] table"""
        assign = self.assign
        order = torch.argsort(assign, stable=True)
        counts = torch.bincount(assign, minlength=self.ncent)
        maxl = int(counts.max()) if counts.numel() else 0
        starts = torch.cumsum(counts, 0) - counts
        pos = torch.arange(order.numel(), device=self.device) - starts[assign[order]]
        lists = torch.full((self.ncent, max(maxl, 1)), -1, dtype=torch.long, device=self.device)
        lists[assign[order], pos] = order
        self.lists = lists

    @property
    def ntotal(self):
        return 0 if self.xb is None else self.xb.shape[0]

    def search(self, q, k, chunk=1024):
        q = torch.as_tensor(q, dtype=torch.float32, device=self.device)
        nprobe = min(self.nprobe, self.ncent)
        ds, ids = [], []
        fused = self.use_kernels and 1 <= int(k) <= knn_ops.MAX_KERNEL_K and nprobe <= 64
        if not fused and self.lists is None:
            self._pad_lists()
        for s in range(0, q.shape[0], chunk):
            qq = q[s:s + chunk]
            if fused:
                probe = knn_ops.flat_topk(qq, self.cent, nprobe)[1]
                kk = min(int(k), nprobe * max(self.maxl, 1))  # as many columns as the padded table gives
                v, got = knn_ops.ivf_topk(qq, self.xs, self.list_ptr, self.row_of, probe, kk, xn=self.xns)
                ds.append(v)
                ids.append(got)
                continue
            probe = torch.topk(_sqdist(qq, self.cent), nprobe, dim=1, largest=False).indices  # [Q, nprobe]
            cand = self.lists[probe].reshape(qq.shape[0], -1)  # [Q, nprobe * maxl]
            valid = cand >= 0
            cz = cand.clamp_min(0)
            xc = self.xb[cz]  # [Q, C, d]
            d = ((qq * qq).sum(1, keepdim=True) - 2.0 * torch.einsum("qd,qcd->qc", qq, xc) + self.xn[cz])
            d = torch.where(valid, d.clamp_min(0.0), torch.full_like(d, float("inf")))
            kk = min(int(k), d.shape[1])
            v, i = torch.topk(d, kk, dim=1, largest=False)
            got = torch.gather(cand, 1, i)
            got = torch.where(torch.isinf(v), torch.full_like(got, -1), got)
            ds.append(v)
            ids.append(got)
        return torch.cat(ds).cpu().numpy(), torch.cat(ids).cpu().numpy()


def build_index(embedding, index_type="ivfflat", device=None, use_kernels=None, max_points_per_centroid=None):
    """``max_points_per_centroid`` caps the k-means training set at that many points per
    centroid (a seeded random subset; faiss uses 256); None trains on everything."""
    n, d = embedding.shape
    if index_type == "flat":
        idx = FlatIndex(d, device, use_kernels=use_kernels)
    elif index_type == "ivfflat":
        ncent = int(4 * math.sqrt(n))
        idx = IVFFlatIndex(d, ncent, nprobe=10, device=device, use_kernels=use_kernels)
        train = embedding
        if max_points_per_centroid is not None and n > int(max_points_per_centroid) * max(ncent, 1):
            g = torch.Generator(device="cpu").manual_seed(1234)
            keep = torch.randperm(n, generator=g)[:int(max_points_per_centroid) * max(ncent, 1)].sort().values
            train = embedding[keep.numpy()] if isinstance(embedding, np.ndarray) else embedding[keep.to(embedding.device)]
        idx.train(train)
    else:
        raise ValueError("unknown index_type %r (flat | ivfflat)" % index_type)
    idx.add(embedding)
    return idx


def main(argv=None):
    p = argparse.ArgumentParser(description="kNN over inferred embeddings")
    p.add_argument("--embedding_file", required=True, help="one .npy file, or a comma-separated list (per rank)")
    p.add_argument("--id_file", default=None, help="one .npy file, or as many as --embedding_file")
    p.add_argument("--query_file", default=None, help="CSV of query vectors (default: first 25 embeddings)")
    p.add_argument("--index_type", default="ivfflat")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--out", default="result.npz")
    p.add_argument("--device", default=None)
    p.add_argument("--max_points_per_centroid", type=int, default=None,
                   help="cap on the k-means training set per centroid (faiss uses 256; default: no cap)")
    a = p.parse_args(argv)
    emb_files = a.embedding_file.split(",")
    emb = np.concatenate([np.load(f, allow_pickle=False).astype(np.float32) for f in emb_files])
    if a.id_file:
        id_files = a.id_file.split(",")
        assert len(id_files) == len(emb_files), "--id_file and --embedding_file list a different number of files"
        ids = np.concatenate([np.load(f, allow_pickle=False).reshape(-1) for f in id_files])
    else:
        ids = np.arange(len(emb))
    assert len(ids) == len(emb), "ids and embeddings differ in length"
    index = build_index(emb, a.index_type, a.device, max_points_per_centroid=a.max_points_per_centroid)
    query = np.loadtxt(a.query_file, dtype=np.float32, delimiter=",", ndmin=2) if a.query_file else emb[:25]
    D, I = index.search(query, a.k)
    res_ids = np.where(I >= 0, ids[np.clip(I, 0, None)], -1)
    np.savez(a.out, distance=D, idx=res_ids)
    print("wrote %s: %d queries x %d neighbours" % (a.out, D.shape[0], D.shape[1]))
    return D, res_ids


if __name__ == "__main__":
    main()
