"""Row sets of frontier inference: the rows of a graph that a request reaches.

A :class:`RowSet` is a *rank bitmap* over the ``N`` rows of a graph (``csrc/hip/csr_rowset.h``):
``table`` int32 ``[ceil(N / 32), 2]`` holds, per 32 rows, the word of their bits and the number
of set bits before the word, and ``rows`` is the sorted int32 list of the set's rows.  The
position of graph row ``j`` in that list — its row in a compact table ``[count, D]`` of the
set — is ``rank[j >> 5] + popcount(bits[j >> 5] & ((1 << (j & 31)) - 1))``: one 8-byte load,
``N / 4`` bytes per set (an ``[N]`` int32 map would be 400 MB at 100M rows).

``neighbor_closure(graph, rows, mask)`` is ``rows ∪ N_mask(rows)``: the valid entries of
``rows`` (duplicates allowed) and every neighbour in ``[0, N)`` of their masked (row, type)
segments — the input set of a full-neighbourhood layer (``ops/sage_csr_ops.py``) whose targets
are ``rows``.  On a GPU graph it is four kernels of ``csrc/hip/frontier.hip`` (mark, mark
neighbours, rank, list) and one read of the set's size; on a CPU graph the same set from
``torch.unique``.
"""
from __future__ import annotations

import torch

from euler_amd.ops._native import hip, use_hip

__all__ = ["RowSet", "neighbor_closure", "row_set"]


def _frontier():
    return hip().frontier


class RowSet:
    """a set of graph rows: ``table`` int32 [ceil(N / 32), 2] = (bits, rank), ``rows`` the
    sorted int32 [count] list, ``count`` its size"""

    def __init__(self, num_rows: int, table: torch.Tensor, rows: torch.Tensor):
        self.num_rows = int(num_rows)
        self.table = table
        self.rows = rows
        self.count = int(rows.numel())

    @property
    def device(self):
        return self.table.device

    @property
    def words(self) -> torch.Tensor:
        return self.table[:, 0]

    @property
    def rank(self) -> torch.Tensor:
        return self.table[:, 1]

    def positions(self, rows) -> torch.Tensor:
        """int64 position of every entry of ``rows`` in the set's list (its row in a compact
        table of the set); -1 for a row the set lacks or one outside ``[0, N)``"""
        r = torch.as_tensor(rows).to(self.device).long().reshape(-1)
        if self.count == 0:
            return torch.full_like(r, -1)
        p = torch.searchsorted(self.rows.long(), r).clamp(max=self.count - 1)
        return torch.where(self.rows.long()[p] == r, p, torch.full_like(p, -1))

    @classmethod
    def from_sorted(cls, num_rows: int, rows: torch.Tensor) -> "RowSet":
        """the set of sorted unique ``rows`` in ``[0, N)`` (torch; the CPU path and the oracle
        of the kernels)"""
        N = int(num_rows)
        W = (N + 31) // 32
        r = rows.long()
        word = r >> 5
        bits = torch.zeros(W, dtype=torch.int64, device=rows.device)
        bits.index_add_(0, word, torch.ones_like(r) << (r & 31))  # unique rows: add = or
        bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)  # the int32 with the same 32 bits
        cnt = torch.bincount(word, minlength=W)
        rank = torch.cumsum(cnt, 0) - cnt
        table = torch.stack([bits, rank], 1).to(torch.int32).contiguous()
        return cls(N, table, rows.to(torch.int32).contiguous())


def _closure_torch(graph, rows, mask) -> RowSet:
    N, T = graph.num_rows, graph.num_types
    dev = graph.indptr.device
    r = rows.to(dev).long().reshape(-1)
    r = torch.unique(r[(r >= 0) & (r < N)])
    types = [t for t in range(T) if (mask >> t) & 1]
    parts = [r]
    if r.numel() and types and graph.nbr.numel():
        seg = r.view(-1, 1) * T + torch.tensor(types, dtype=torch.int64, device=dev).view(1, -1)
        a, b = graph.indptr[seg].reshape(-1), graph.indptr[seg + 1].reshape(-1)
        lens = (b - a).clamp(min=0)
        ne = int(lens.sum())
        if ne:
            first = torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
            e = torch.repeat_interleave(a, lens) + torch.arange(ne, dtype=torch.int64, device=dev) - first
            j = graph.nbr[e].long()
            parts.append(j[(j >= 0) & (j < N)])
    return RowSet.from_sorted(N, torch.unique(torch.cat(parts)))


def _build(graph, rows, mask, neighbors: bool) -> RowSet:
    N = graph.num_rows
    m = graph._mask(None) if mask is None else int(mask)
    rows = torch.as_tensor(rows)
    if not use_hip(graph.indptr):
        if not neighbors:
            m = 0
        return _closure_torch(graph, rows, m)
    dev = graph.indptr.device
    r = rows.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    table = torch.zeros(((N + 31) // 32, 2), dtype=torch.int32, device=dev)
    if r.numel() == 0:  # the empty set: nothing to launch
        return RowSet(N, table, torch.zeros(0, dtype=torch.int32, device=dev))
    f = _frontier()
    f.mark_rows(table, r, N)
    if neighbors:
        f.mark_neighbors(table, graph.indptr, graph.nbr, graph.num_types, m & 0xFFFFFFFF, r)
    count = int(f.rank_words(table, N).item())  # the one host read: it sizes the list and the compact table
    return RowSet(N, table, f.list_rows(table, N, count))


def row_set(graph, rows) -> RowSet:
    """the set of the valid entries of ``rows`` (duplicates and entries outside ``[0, N)`` allowed)"""
    return _build(graph, rows, 0, False)


def neighbor_closure(graph, rows, mask=None) -> RowSet:
    """``rows ∪ N_mask(rows)`` (module docstring); ``mask`` an edge-type bit set (None: every type)"""
    return _build(graph, rows, mask, True)
