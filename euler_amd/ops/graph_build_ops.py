"""Edge list -> per-(row, edge type) CSR, the structure arrays of ``DeviceGraph``
(``DeviceGraph.from_edges``).

``build_csr`` takes endpoint ids, optional fp32 weights and int edge types and returns
``indptr`` int64 ``[N*T+1]``, ``nbr`` int32 ``[nnz]`` and ``cumw`` fp32 ``[nnz]`` (inclusive
prefix sums of the weights inside every ``(row, type)`` segment).  Neighbours are ascending
inside a segment; equal neighbours keep their input order.

One algorithm, two implementations:

1. pack every edge into the key ``((row * T + type) << dst_bits) | dst_row`` (relabelling the
   endpoints by a binary search in the sorted id table when there is one, validating ids,
   types and weights on the way), the payload is the edge index; ``symmetric`` appends the
   reverse edge ``E + i``;
2. stable sort of (key, payload) over the bits the key uses;
3. ``duplicates="sum"``: runs of equal keys become one entry (first payload, fp64 sum of the
   run's weights in input order);
4. ``indptr[s]`` = lower bound of ``s << dst_bits`` in the sorted keys;
5. prefix sums per segment in fp64, stored as fp32; ``nbr`` = the key's low bits.

On GPU tensors the steps are gfx950 kernels (``csrc/hip/graph_build.hip``; the sort is
``hipcub``'s radix sort).  CPU tensors -- and ``impl="torch"`` on any device, which is what the
benchmark compares the kernels with -- take the torch composition below (``torch.sort`` on the
packed key, ``unique_consecutive``, ``cumsum``).

Failures are collected in one status word that is read once: after the build under
``"keep"``, before the compaction under ``"sum"`` (its output size is read with it).
"""
from __future__ import annotations

import torch

from euler_amd.ops._native import hip, use_hip

__all__ = ["build_csr", "key_bits", "unique_ids", "rows_of_ids", "MAX_TYPES", "MAX_EDGES"]

MAX_TYPES = 32            # DeviceGraph type masks are 32-bit
MAX_EDGES = (1 << 31) - 1  # the sort's item count is 32-bit
_SIGN = -(1 << 63)


def key_bits(num_rows: int, num_types: int):
    """``(dst_bits, seg_bits)`` of the packed key; ValueError if it needs more than 63 bits"""
    dst_bits = max(1, (int(num_rows) - 1).bit_length())
    seg_bits = max(1, (int(num_rows) * int(num_types) - 1).bit_length())
    if dst_bits + seg_bits > 63:
        raise ValueError(f"from_edges: {num_rows} rows x {num_types} edge types need a {dst_bits + seg_bits}-bit "
                         "sort key; the limit is 63 bits")
    return dst_bits, seg_bits


def unique_ids(parts):
    """sorted unique of the int64 id tensors ``parts``, ascending as *unsigned* 64-bit (the
    order ``DeviceGraph.rows_of`` searches in)"""
    x = torch.cat([p.reshape(-1).long() for p in parts])
    return torch.unique(x ^ _SIGN) ^ _SIGN


def rows_of_ids(q, ids):
    """``(rows, found)`` of the ids ``q`` in ``ids`` (from :func:`unique_ids`)"""
    n = ids.numel()
    if n == 0:
        return torch.zeros_like(q, dtype=torch.long), torch.zeros_like(q, dtype=torch.bool)
    pos = torch.searchsorted(ids ^ _SIGN, q.long() ^ _SIGN).clamp_(max=n - 1)
    return pos, ids[pos] == q


def _raise_status(flags: int, bad_ids: int, num_rows: int, num_types: int, relabelled: bool):
    if flags & 1:
        where = "absent from the node set" if relabelled else f"outside [0, {num_rows})"
        raise ValueError(f"from_edges: {bad_ids} endpoint ids are {where}")
    if flags & 2:
        raise ValueError(f"from_edges: edge_type must be in [0, num_types = {num_types})")
    if flags & 4:
        raise ValueError("from_edges: weights must be finite and >= 0")


def _torch_build(src, dst, weight, etype, ids, N, T, symmetric, duplicates, want_order):
    """the torch composition (any device)"""
    dev = src.device
    E = src.numel()
    dst_bits, _ = key_bits(N, T)
    if ids is None:
        r, c = src.long(), dst.long()
        okr, okc = (r >= 0) & (r < N), (c >= 0) & (c < N)
    else:
        (r, okr), (c, okc) = rows_of_ids(src, ids), rows_of_ids(dst, ids)
    t = torch.zeros(E, dtype=torch.long, device=dev) if etype is None else etype.long()
    okt = (t >= 0) & (t < T)
    okw = torch.ones(E, dtype=torch.bool, device=dev) if weight is None else \
        torch.isfinite(weight) & (weight >= 0)
    status = torch.stack([(~okr).sum() + (~okc).sum(), (~okt).sum(), (~okw).sum()]).tolist()  # the one read
    flags = (1 if status[0] else 0) | (2 if status[1] else 0) | (4 if status[2] else 0)
    _raise_status(flags, int(status[0]), N, T, ids is not None)
    key = ((r * T + t) << dst_bits) | c
    if symmetric:
        key = torch.cat([key, ((c * T + t) << dst_bits) | r])
    del r, c, t
    skey, order = torch.sort(key, stable=True)
    del key
    if weight is None:
        w = torch.ones(skey.numel(), dtype=torch.float32, device=dev)
    else:
        w = weight[order - E * (order >= E)] if symmetric else weight[order]
    if duplicates == "sum":
        skey, counts = torch.unique_consecutive(skey, return_counts=True)
        run = torch.repeat_interleave(torch.arange(skey.numel(), device=dev), counts)
        w = torch.zeros(skey.numel(), dtype=torch.float64, device=dev).index_add_(0, run, w.double()).float()
        order = order[torch.cumsum(counts, 0) - counts]
        del run, counts
    S = N * T
    indptr = torch.searchsorted(skey, torch.arange(S + 1, dtype=torch.long, device=dev) << dst_bits)
    cs = torch.cumsum(w.double(), 0)
    base = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), cs])[indptr[:-1]]
    cumw = (cs - torch.repeat_interleave(base, torch.diff(indptr))).float()
    nbr = (skey & ((1 << dst_bits) - 1)).int()
    return indptr, nbr, cumw, (order if want_order else None)


def _hip_build(src, dst, weight, etype, ids, N, T, symmetric, duplicates, want_order):
    E = src.numel()
    dst_bits, seg_bits = key_bits(N, T)
    status = torch.zeros(4, dtype=torch.int64, device=src.device)
    keys, idx = hip().graph_build_pack(src, dst, weight, etype, ids, N, T, dst_bits, bool(symmetric), status)
    skeys, perm = hip().graph_build_sort(keys, idx, dst_bits + seg_bits)
    del keys, idx
    if duplicates == "sum":
        incl = hip().graph_build_heads(skeys, status)
        flags, bad, nnz, _ = status.tolist()  # the one read: failures and the number of runs
        _raise_status(flags, bad, N, T, ids is not None)
        skeys, perm, cw = hip().graph_build_compact(skeys, perm, incl, weight, E, nnz)
        del incl
        indptr, nbr, cumw = hip().graph_build_csr(skeys, None, cw, E, N, T, dst_bits)
    else:
        indptr, nbr, cumw = hip().graph_build_csr(skeys, perm, weight, E, N, T, dst_bits)
        flags, bad, _, _ = status.tolist()    # the one read
        _raise_status(flags, bad, N, T, ids is not None)
    return indptr, nbr, cumw, (perm.long() if want_order else None)


def build_csr(src, dst, weight=None, etype=None, ids=None, *, num_rows, num_types=1, symmetric=False,
              duplicates="keep", want_order=False, impl=None):
    """``(indptr, nbr, cumw, order)`` of the edge list (see the module docstring).

    ``src`` / ``dst``: int32 or int64 ``[E]`` on one device; ``weight``: fp32 ``[E]`` or None
    (= 1); ``etype``: int32 ``[E]`` or None (= 0); ``ids``: None (an id is its row, validated
    against ``num_rows``) or the :func:`unique_ids` table ``[num_rows]``.  ``order`` (int64
    ``[nnz]``, ``want_order``): the input edge of every CSR slot, ``E + i`` for the reverse
    copy of edge ``i``, the first edge of a merged run.  ``impl``: None (kernels on GPU
    tensors, torch on CPU tensors) or ``"torch"``."""
    N, T = int(num_rows), int(num_types)
    if duplicates not in ("keep", "sum"):
        raise ValueError(f"from_edges: duplicates must be 'keep' or 'sum', got {duplicates!r}")
    if not 1 <= T <= MAX_TYPES:
        raise ValueError(f"from_edges: num_types = {T} is outside [1, {MAX_TYPES}] (edge-type masks are 32-bit)")
    if N >= 1 << 31:
        raise ValueError(f"from_edges: {N} nodes; neighbour rows are int32, the limit is 2^31 - 1")
    E = src.numel()
    if dst.numel() != E or (weight is not None and weight.numel() != E) or (etype is not None and etype.numel() != E):
        raise ValueError("from_edges: src, dst, weight and edge_type differ in length")
    if E * (2 if symmetric else 1) > MAX_EDGES:
        raise ValueError(f"from_edges: {E * (2 if symmetric else 1)} edges (after symmetrisation); the sort's item "
                         "count is 32-bit, the limit is 2^31 - 1")
    dev = src.device
    if E == 0 or N == 0:
        if E and N == 0:
            raise ValueError(f"from_edges: {2 * E} endpoint ids are outside [0, 0)")
        return (torch.zeros(N * T + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.float32, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev) if want_order else None)
    key_bits(N, T)
    args = (src.contiguous(), dst.contiguous(), None if weight is None else weight.contiguous(),
            None if etype is None else etype.contiguous(), None if ids is None else ids.contiguous(), N, T,
            bool(symmetric), duplicates, bool(want_order))
    if impl == "torch" or not use_hip(src, dst, weight, etype, ids):
        return _torch_build(*args)
    return _hip_build(*args)
