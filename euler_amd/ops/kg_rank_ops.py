"""Rank counts for knowledge-graph link prediction (``euler_amd.models.kg_eval``).

* ``rank_counts(q, cands, true_idx, kind, filt_ptr=None, filt_idx=None)`` — for every query
  row, how many candidate rows score strictly better than the true candidate (``better``)
  and how many score exactly the same (``ties``).

Score kinds (``kind``): ``"l1"`` ``sum_d |q - c|`` and ``"l2"`` ``sum_d (q - c)^2`` (lower is
better; the square root is dropped, the order is the same), ``"dot"`` ``sum_d q * c`` (higher
is better).

Counting rule: candidate ``e`` counts for query ``b`` when ``e != true_idx[b]``, ``e`` is not
in ``b``'s filter list, and its score is better than / equal to the score of
``cands[true_idx[b]]``.  The filter is a CSR over the queries: ``filt_ptr [B + 1]`` int64 and
``filt_idx`` int32 positions in ``cands``, ascending inside each list (the true entity may be
in its own list: it is skipped anyway).  A rank follows as ``1 + better`` (optimistic),
``1 + better + ties`` (pessimistic) or ``1 + better + ties / 2`` (mean).

On GPU tensors the op runs hand-written gfx950 kernels (``csrc/hip/kg_rank.hip``): a pre-pass
scores the true candidates, a tiled scan compares every (query, candidate) pair against
them and writes per-(query, candidate range) partial counts, which are summed.  No
``[B, N]`` score matrix is ever allocated.  Every score is one fp32 accumulator folded over
``d`` ascending, in both kernels, so a candidate row bitwise equal to the true row ties
exactly.  CPU tensors take the pure-torch twin below; it is the oracle in tests.  The twin
reduces a ``[b, N, d]`` tensor of terms per chunk of queries (one reduction for all three
kinds, so equal rows give equal scores) and the chunk is sized so that it holds at most 2^26
terms, not scores: at N = 14,951 and d = 100 that is 44 queries per chunk, which makes the
CPU route slow at the scale of a real test split.  It is meant for tests and small graphs.

Operands are taken as they are: ``q`` / ``cands`` contiguous fp32, ``true_idx`` /
``filt_ptr`` contiguous int64, ``filt_idx`` contiguous int32, all on one device.  Anything
else raises ``ValueError`` (``RuntimeError`` from the binding's own checks, such as the
range of ``true_idx`` on the GPU) before a launch.
"""
from __future__ import annotations

import torch

from euler_amd.ops._native import hip, use_hip

__all__ = ["rank_counts", "KINDS"]

KINDS = ("l1", "l2", "dot")
_MAX_SPLITS = 4096
_TARGET_BLOCKS = 1024  # a few resident blocks on each of the 256 CUs
_TQ, _TC = 64, 64      # the scan kernel's query / candidate tile
_TWIN_SCORES = 1 << 26  # terms (b * N * d) a chunk of the twin may hold


def _check(t, dtype, name, like, dim):
    if not isinstance(t, torch.Tensor):
        raise ValueError("rank_counts: %s must be a tensor" % name)
    if t.dtype != dtype:
        raise ValueError("rank_counts: %s has dtype %s, expected %s" % (name, t.dtype, dtype))
    if t.dim() != dim:
        raise ValueError("rank_counts: %s must have %d dimension(s)" % (name, dim))
    if not t.is_contiguous():
        raise ValueError("rank_counts: %s must be contiguous" % name)
    if t.device != like.device:
        raise ValueError("rank_counts: %s is on %s, q on %s" % (name, t.device, like.device))


def _auto_splits(b, n):
    nqt = -(-b // _TQ)
    tiles = -(-n // _TC)
    s = -(-_TARGET_BLOCKS // nqt)
    return int(max(1, min(s, _MAX_SPLITS, tiles)))


def _scores(q, c, kind):
    """[b, n] scores of q [b, d] against c [n, d] (twin only).  All three kinds reduce a
    [b, n, d] tensor of terms the same way, so equal rows of c give equal scores (a blocked
    GEMM would not promise that for ``dot``)."""
    if kind == "dot":
        return (q.unsqueeze(1) * c.unsqueeze(0)).sum(-1)
    diff = q.unsqueeze(1) - c.unsqueeze(0)
    return diff.abs().sum(-1) if kind == "l1" else (diff * diff).sum(-1)


def _rank_counts_torch(q, cands, true_idx, kind, filt_ptr, filt_idx):
    B, N, d = q.shape[0], cands.shape[0], q.shape[1]
    better = torch.zeros(B, dtype=torch.long, device=q.device)
    ties = torch.zeros(B, dtype=torch.long, device=q.device)
    per = N * d  # a chunk holds a [b, N, d] tensor of terms
    chunk = max(1, min(B, _TWIN_SCORES // max(per, 1)))
    if filt_ptr is not None:
        nf = filt_idx.numel()
        lens = (filt_ptr[1:].clamp(0, nf) - filt_ptr[:-1].clamp(0, nf)).clamp_min(0)
    for s0 in range(0, B, chunk):
        s1 = min(B, s0 + chunk)
        qq, tt = q[s0:s1], true_idx[s0:s1]
        sc = _scores(qq, cands, kind)
        # the true score is taken from the same matrix, so an identical row ties exactly
        ts = sc.gather(1, tt.unsqueeze(1))
        bt = sc > ts if kind == "dot" else sc < ts
        tie = sc == ts
        keep = torch.ones_like(bt)
        keep.scatter_(1, tt.unsqueeze(1), False)
        if filt_ptr is not None:
            ln = lens[s0:s1]
            total = int(ln.sum())
            if total:
                rows = torch.repeat_interleave(torch.arange(s1 - s0, device=q.device), ln)
                first = filt_ptr[s0:s1].clamp(0, nf)
                off = torch.arange(total, device=q.device) - torch.repeat_interleave(ln.cumsum(0) - ln, ln)
                cols = filt_idx[torch.repeat_interleave(first, ln) + off].long()
                ok = (cols >= 0) & (cols < N)
                keep[rows[ok], cols[ok]] = False
        better[s0:s1] = (bt & keep).sum(1)
        ties[s0:s1] = (tie & keep).sum(1)
    return better, ties


def rank_counts(q, cands, true_idx, kind, filt_ptr=None, filt_idx=None, splits=None):
    """``(better [B], ties [B])`` int64 of the queries ``q [B, d]`` against the candidates
    ``cands [N, d]``, relative to ``cands[true_idx[b]]``; see the module docstring for the
    kinds, the counting rule and the filter CSR.  ``splits`` fixes the number of candidate
    ranges scanned in parallel on the GPU (default: enough to fill the chip)."""
    if kind not in KINDS:
        raise ValueError("rank_counts: kind must be one of %s, got %r" % (KINDS, kind))
    _check(q, torch.float32, "q", q, 2)
    _check(cands, torch.float32, "cands", q, 2)
    _check(true_idx, torch.int64, "true_idx", q, 1)
    if q.shape[1] != cands.shape[1] or q.shape[1] < 1:
        raise ValueError("rank_counts: q [B, d] and cands [N, d] must share d >= 1")
    B, N = q.shape[0], cands.shape[0]
    if true_idx.numel() != B:
        raise ValueError("rank_counts: true_idx must be [B]")
    if (filt_ptr is None) != (filt_idx is None):
        raise ValueError("rank_counts: filt_ptr and filt_idx come together or not at all")
    if filt_ptr is not None:
        _check(filt_ptr, torch.int64, "filt_ptr", q, 1)
        _check(filt_idx, torch.int32, "filt_idx", q, 1)
        if filt_ptr.numel() != B + 1:
            raise ValueError("rank_counts: filt_ptr must be [B + 1], got %d entries for B = %d"
                             % (filt_ptr.numel(), B))
    if B == 0:
        z = torch.zeros(0, dtype=torch.long, device=q.device)
        return z, z.clone()
    if N == 0:
        raise ValueError("rank_counts: no candidates")
    if not use_hip(q, cands, true_idx, filt_ptr, filt_idx):
        lo, hi = int(true_idx.min()), int(true_idx.max())
        if lo < 0 or hi >= N:
            raise ValueError("rank_counts: true_idx out of range [0, %d): min %d, max %d" % (N, lo, hi))
        return _rank_counts_torch(q, cands, true_idx, kind, filt_ptr, filt_idx)
    # the binding checks the range of true_idx (one host read) before it launches
    s = _auto_splits(B, N) if splits is None else int(splits)
    better, ties = hip().kg_rank_counts(q, cands, true_idx, KINDS.index(kind), filt_ptr, filt_idx, s)
    return better, ties
