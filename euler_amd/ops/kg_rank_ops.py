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

* ``rank_counts_proj(model, table, rel_table, proj_tables, given, true_idx, rel, side, kind,
  filt_ptr=None, filt_idx=None)`` — the same counts for the projected models TransH / TransD /
  TransR, from the RAW tables: every query ranks ``true_idx[b]`` among all rows of ``table``
  projected under the query's own relation ``rel[b]``.  On the GPU the candidates are projected
  inside the scan kernel (``csrc/hip/kg_rank_proj.hip``), one call for any mix of relations:
  neither a projected table nor a score matrix is written.  CPU tensors take a torch twin
  that projects per relation with the model classes' own ``projection`` functions.

Operands are taken as they are: ``q`` / ``cands`` contiguous fp32, ``true_idx`` /
``filt_ptr`` contiguous int64, ``filt_idx`` contiguous int32, all on one device.  Anything
else raises ``ValueError`` (``RuntimeError`` from the binding's own checks, such as the
range of ``true_idx`` on the GPU) before a launch.
"""
from __future__ import annotations

import torch

from euler_amd.ops._native import hip, use_hip

__all__ = ["rank_counts", "rank_counts_proj", "rank_proj_covered", "KINDS", "PROJ_MODELS"]

KINDS = ("l1", "l2", "dot")
SIDES = ("head", "tail")
_MAX_SPLITS = 4096
_TARGET_BLOCKS = 1024  # a few resident blocks on each of the 256 CUs
_TQ, _TC = 64, 64      # the scan kernel's query / candidate tile
_TWIN_SCORES = 1 << 26  # terms (b * N * d) a chunk of the twin may hold
PROJ_MODELS = ("transh", "transd", "transr")
_PROJ_MAX_DIM = 128    # kg_rank_proj.hip: the relation operands, the queries and a candidate tile share the LDS


def _check(t, dtype, name, like, dim, op="rank_counts"):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be a tensor" % (op, name))
    if t.dtype != dtype:
        raise ValueError("%s: %s has dtype %s, expected %s" % (op, name, t.dtype, dtype))
    if t.dim() != dim:
        raise ValueError("%s: %s must have %d dimension(s)" % (op, name, dim))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (op, name))
    if t.device != like.device:
        raise ValueError("%s: %s is on %s, the first operand on %s" % (op, name, t.device, like.device))


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


# ----------------------------------------------------------------------------- projected models
def _proj_dims_ok(model, E, R):
    ok = E % 4 == 0 and R % 4 == 0 and 4 <= E <= _PROJ_MAX_DIM and 4 <= R <= _PROJ_MAX_DIM
    return ok and (model == "transr" or E == R)


def rank_proj_covered(model, table, rel_table, proj_tables):
    """True when :func:`rank_counts_proj` takes these tables: a known model, contiguous fp32
    tables on one device, E and R multiples of 4 in [4, 128] (E == R unless TransR), N below
    2^31 and, on the GPU, 16-byte aligned storage.  ``models/kg_eval`` keeps its per-relation
    loop for anything else."""
    tabs = (table, rel_table) + tuple(proj_tables)
    if model not in PROJ_MODELS or len(tabs) != (4 if model == "transd" else 3):
        return False
    if not all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
               and t.device == table.device for t in tabs):
        return False
    if table.is_cuda and any(t.data_ptr() % 16 for t in tabs):
        return False
    return _proj_dims_ok(model, table.shape[1], rel_table.shape[1]) and 0 < table.shape[0] < 2 ** 31


def _project_all(model, table, proj_tables, r):
    """[N, D'] rows of ``table`` projected under relation row ``r``, by the model classes' own
    formulas (twin only)"""
    from euler_amd.models.knowledge_graph import TransD, TransH, TransR

    if model == "transh":
        return TransH.projection(table, proj_tables[0][r])
    if model == "transd":
        return TransD.projection(table, proj_tables[0], proj_tables[1][r])
    mat = proj_tables[0][r].reshape(1, table.shape[1], -1)
    return TransR.projection(None, table.unsqueeze(0), mat).squeeze(0)


def _rank_counts_proj_torch(model, table, rel_table, proj_tables, given, true_idx, rel, side, kind, filt_ptr,
                            filt_idx):
    B = given.numel()
    better = torch.zeros(B, dtype=torch.long, device=table.device)
    ties = torch.zeros(B, dtype=torch.long, device=table.device)
    for r in torch.unique(rel).tolist():
        sel = (rel == r).nonzero().reshape(-1)
        space = _project_all(model, table, proj_tables, r).contiguous()
        rho = torch.nn.functional.normalize(rel_table[r], dim=-1)
        q = space[given[sel]] + rho if side == "tail" else space[given[sel]] - rho
        ptr = idx = None
        if filt_ptr is not None:  # the selected queries' lists, as a CSR of their own
            nf = filt_idx.numel()
            lo, hi = filt_ptr[:-1][sel].clamp(0, nf), filt_ptr[1:][sel].clamp(0, nf)
            ln = (hi - lo).clamp_min(0)
            ptr = torch.zeros(sel.numel() + 1, dtype=torch.long, device=table.device)
            ptr[1:] = ln.cumsum(0)
            total = int(ptr[-1])
            off = torch.arange(total, device=table.device) - torch.repeat_interleave(ptr[:-1], ln)
            idx = filt_idx[torch.repeat_interleave(lo, ln) + off]
        better[sel], ties[sel] = _rank_counts_torch(q.contiguous(), space, true_idx[sel], kind, ptr, idx)
    return better, ties


def rank_counts_proj(model, table, rel_table, proj_tables, given, true_idx, rel, side, kind, filt_ptr=None,
                     filt_idx=None, splits=None):
    """``(better [B], ties [B])`` int64 for the projected models, from the raw fp32 tables as
    ``gnn_ops.kg_score_proj`` takes them: ``model`` "transh" (``proj_tables = (hyper,)``),
    "transd" (``(entity_transfer, relation_transfer)``) or "transr" (``(mat [Nr, E * R],)``).

    Query ``b`` ranks entity ``true_idx[b]`` among all ``N`` rows of ``table`` under relation row
    ``rel[b]``: with ``P_r`` the model's projection and ``rho = normalize(rel_table[r])`` the
    query row is ``P_r(table[given[b]]) + rho`` (``side="tail"``: ``given`` are the heads) or
    ``- rho`` (``side="head"``: the tails), scored against ``P_r(table[e])`` in ``kind`` "l1" or
    "l2".  ``table`` (and TransD's ``entity_transfer``) hold exactly the candidates; ids must be
    inside their tables.  The filter CSR and the counting rule are those of :func:`rank_counts`.
    ``splits`` fixes the number of candidate ranges (default: sized from the number of
    single-relation query tiles, which only the binding knows after it has ordered the batch).
    Shapes outside :func:`rank_proj_covered` raise ``ValueError``."""
    op = "rank_counts_proj"
    if model not in PROJ_MODELS:
        raise ValueError("%s: model must be one of %s, got %r" % (op, PROJ_MODELS, model))
    if kind not in ("l1", "l2"):
        raise ValueError("%s: kind must be 'l1' or 'l2', got %r" % (op, kind))
    if side not in ("head", "tail"):
        raise ValueError("%s: side must be 'head' or 'tail', got %r" % (op, side))
    proj_tables = tuple(proj_tables)
    if len(proj_tables) != (2 if model == "transd" else 1):
        raise ValueError("%s: proj_tables is (entity_transfer, relation_transfer) for transd, one table otherwise"
                         % op)
    _check(table, torch.float32, "table", table, 2, op)
    _check(rel_table, torch.float32, "rel_table", table, 2, op)
    for i, t in enumerate(proj_tables):
        _check(t, torch.float32, "proj_tables[%d]" % i, table, 2, op)
    for t, name in ((given, "given"), (true_idx, "true_idx"), (rel, "rel")):
        _check(t, torch.int64, name, table, 1, op)
    N, E, R, Nr = table.shape[0], table.shape[1], rel_table.shape[1], rel_table.shape[0]
    if not _proj_dims_ok(model, E, R) or not 0 < N < 2 ** 31 or Nr < 1:
        raise ValueError("%s: needs E %% 4 == 0, R %% 4 == 0, 4 <= E, R <= %d (E == R unless transr) and "
                         "0 < N < 2^31, got E = %d, R = %d, N = %d" % (op, _PROJ_MAX_DIM, E, R, N))
    want = [(Nr, E * R)] if model == "transr" else ([(N, E), (Nr, E)] if model == "transd" else [(Nr, E)])
    if [tuple(t.shape) for t in proj_tables] != want:
        raise ValueError("%s: proj_tables of %s must have shapes %s" % (op, model, want))
    B = given.numel()
    if true_idx.numel() != B or rel.numel() != B:
        raise ValueError("%s: given, true_idx and rel must be [B]" % op)
    if (filt_ptr is None) != (filt_idx is None):
        raise ValueError("%s: filt_ptr and filt_idx come together or not at all" % op)
    if filt_ptr is not None:
        _check(filt_ptr, torch.int64, "filt_ptr", table, 1, op)
        _check(filt_idx, torch.int32, "filt_idx", table, 1, op)
        if filt_ptr.numel() != B + 1:
            raise ValueError("%s: filt_ptr must be [B + 1], got %d entries for B = %d" % (op, filt_ptr.numel(), B))
    if B == 0:
        z = torch.zeros(0, dtype=torch.long, device=table.device)
        return z, z.clone()
    if not use_hip(table, rel_table, *proj_tables, given, true_idx, rel, filt_ptr, filt_idx):
        for t, name, n in ((given, "given", N), (true_idx, "true_idx", N), (rel, "rel", Nr)):
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= n:
                raise ValueError("%s: %s out of range [0, %d): min %d, max %d" % (op, name, n, lo, hi))
        return _rank_counts_proj_torch(model, table, rel_table, proj_tables, given, true_idx, rel, side, kind,
                                       filt_ptr, filt_idx)
    if any(t.data_ptr() % 16 for t in (table, rel_table) + proj_tables):
        raise ValueError("%s: tables must be 16-byte aligned" % op)
    # the binding checks the id ranges (one host read), orders the queries by relation and
    # builds the tile table (one host read for its length) before it launches
    proj_e, proj_r = proj_tables if model == "transd" else (None, proj_tables[0])
    better, ties = hip().kg_rank_proj.rank_counts(PROJ_MODELS.index(model), table, rel_table, proj_e, proj_r, given,
                                                  true_idx, rel, SIDES.index(side), KINDS.index(kind), filt_ptr,
                                                  filt_idx, 0 if splits is None else int(splits))
    return better, ties
