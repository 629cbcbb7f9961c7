"""Fused distance + top-k search ops behind ``euler_amd.tools.knn``.

* ``flat_topk(q, x, k)``  — exact k nearest rows of ``x`` for every query;
* ``ivf_topk(q, xs, list_ptr, row_of, probe, k)`` — the same over the inverted lists a
  query probes;
* ``nearest(q, x)``       — ``flat_topk`` with ``k = 1`` (k-means / coarse assignment).

Ordering rule: results are ordered by the pair (squared distance, original row), ascending,
so equal distances go to the lower row.  The ranking key is ``s = ||x||^2 - 2 q.x``; the
distance is ``max(s + ||q||^2, 0)``.  Missing results are ``inf`` / ``-1``.

On GPU tensors the ops run hand-written gfx950 kernels (``csrc/hip/knn.hip``): a scan
kernel writes, per (query, split), a sorted partial list ``dist [nq, S, k]`` fp32 /
``row [nq, S, k]`` int64, and a merge kernel combines the ``S`` partials.  No
``[nq, n]`` distance matrix is ever allocated.  CPU tensors (and ``k`` above the kernels'
limit of 128) take the pure-torch twin below, which follows the same ordering rule and is
the oracle in tests.

Inverted lists are a CSR: ``xs`` is the database permuted so that list ``l`` is the rows
``list_ptr[l]:list_ptr[l + 1]``, ``row_of[p]`` is the original row of position ``p``.
Inside a list the positions must be in ascending original-row order (a stable sort by
list gives that); ties inside a list are then decided by position.
"""
from __future__ import annotations

import torch

from euler_amd.ops._native import hip, use_hip

__all__ = ["flat_topk", "ivf_topk", "nearest", "build_lists", "MAX_KERNEL_K"]

MAX_KERNEL_K = 128
_MAX_SPLITS = 64
_TARGET_BLOCKS = 512  # two resident blocks on each of the 256 CUs


def _f32(t):
    return t.to(torch.float32).contiguous()


def _norms(x):
    return (x * x).sum(1)


def _empty_result(nq, k, device):
    return (torch.full((nq, k), float("inf"), device=device),
            torch.full((nq, k), -1, dtype=torch.long, device=device))


def _auto_splits(nq, n, k):
    tq = 128 if k <= 32 else 64
    nqt = -(-nq // tq)
    s = -(-_TARGET_BLOCKS // nqt)
    tiles = -(-n // 64)
    return int(max(1, min(s, _MAX_SPLITS, tiles // 8)))


def _flat_topk_torch(q, x, k, xn):
    """the twin: stable sort of s = xn - 2 q.x, so ties go to the lower row"""
    nq, n = q.shape[0], x.shape[0]
    D, I = _empty_result(nq, k, q.device)
    kk = min(k, n)
    if kk == 0 or nq == 0:
        return D, I
    chunk = max(1, min(nq, (1 << 26) // max(n, 1)))
    for s0 in range(0, nq, chunk):
        qq = q[s0:s0 + chunk]
        s = xn.unsqueeze(0) - 2.0 * (qq @ x.t())
        v, i = torch.sort(s, dim=1, stable=True)
        D[s0:s0 + chunk, :kk] = (v[:, :kk] + _norms(qq).unsqueeze(1)).clamp_min_(0.0)
        I[s0:s0 + chunk, :kk] = i[:, :kk]
    return D, I


def _ivf_topk_torch(q, xs, list_ptr, row_of, probe, k, xn):
    nq = q.shape[0]
    ncent = list_ptr.numel() - 1
    D, I = _empty_result(nq, k, q.device)
    ptr = list_ptr.tolist()
    for i, lists in enumerate(probe.tolist()):
        pos = [torch.arange(ptr[l], ptr[l + 1], device=q.device) for l in lists if 0 <= l < ncent]
        pos = torch.cat(pos) if pos else torch.zeros(0, dtype=torch.long, device=q.device)
        if pos.numel() == 0:
            continue
        s = xn[pos] - 2.0 * (xs[pos] @ q[i])
        rows = row_of[pos]
        o = torch.argsort(rows, stable=True)
        o = o[torch.argsort(s[o], stable=True)][:k]
        D[i, :o.numel()] = (s[o] + (q[i] * q[i]).sum()).clamp_min(0.0)
        I[i, :o.numel()] = rows[o]
    return D, I


def flat_topk(q, x, k, xn=None, splits=None):
    """``(D [nq, k] fp32, I [nq, k] int64)``: the k nearest rows of ``x [n, d]`` for each row of
    ``q [nq, d]``.  ``xn`` is ``||x||^2`` per row if the caller has it; ``splits`` fixes the
    number of row ranges scanned in parallel (default: enough to fill the chip)."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    q, x = _f32(q), _f32(x)
    if q.dim() != 2 or x.dim() != 2 or q.shape[1] != x.shape[1]:
        raise ValueError("flat_topk: q [nq, d] and x [n, d] must share d")
    xn = _norms(x) if xn is None else _f32(xn)
    nq, n = q.shape[0], x.shape[0]
    if nq == 0 or n == 0:
        return _empty_result(nq, k, q.device)
    if not use_hip(q, x, xn) or k > MAX_KERNEL_K:
        return _flat_topk_torch(q, x, k, xn)
    s = _auto_splits(nq, n, k) if splits is None else int(splits)
    pd, pr = hip().knn_flat_scan(q, x, xn, k, s)
    D, I = hip().knn_merge(pd, pr, _norms(q))
    return D, I


def nearest(q, x, xn=None):
    """index of the nearest row of ``x`` per query (the lowest one among equals)"""
    return flat_topk(q, x, 1, xn=xn)[1][:, 0]


def ivf_topk(q, xs, list_ptr, row_of, probe, k, xn=None):
    """``(D, I)`` over the lists in ``probe [nq, nprobe]`` (``-1``: none); ``I`` holds
    original rows.  See the module docstring for the CSR layout."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    q, xs = _f32(q), _f32(xs)
    xn = _norms(xs) if xn is None else _f32(xn)
    list_ptr, row_of, probe = list_ptr.long().contiguous(), row_of.long().contiguous(), probe.long().contiguous()
    if q.dim() != 2 or xs.dim() != 2 or q.shape[1] != xs.shape[1]:
        raise ValueError("ivf_topk: q [nq, d] and xs [n, d] must share d")
    if probe.dim() != 2 or probe.shape[0] != q.shape[0]:
        raise ValueError("ivf_topk: probe must be [nq, nprobe]")
    if q.shape[0] == 0 or probe.shape[1] == 0:
        return _empty_result(q.shape[0], k, q.device)
    if not use_hip(q, xs, xn, list_ptr, row_of, probe) or k > MAX_KERNEL_K or probe.shape[1] > _MAX_SPLITS:
        return _ivf_topk_torch(q, xs, list_ptr, row_of, probe, k, xn)
    pd, pr = hip().knn_ivf_scan(q, xs, xn, list_ptr, row_of, probe, k)
    return tuple(hip().knn_merge(pd, pr, _norms(q)))


def build_lists(assign, ncent):
    """CSR inverted lists of an assignment ``[n]``: ``(list_ptr [ncent + 1], row_of [n])``;
    the sort is stable, so original order is kept inside a list"""
    assign = assign.long()
    row_of = torch.argsort(assign, stable=True)
    counts = torch.bincount(assign, minlength=ncent)
    list_ptr = torch.zeros(ncent + 1, dtype=torch.long, device=assign.device)
    list_ptr[1:] = torch.cumsum(counts, 0)
    return list_ptr, row_of
