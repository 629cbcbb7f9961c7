"""Full-neighbourhood GraphSAGE layer over a :class:`DeviceGraph`'s own CSR.

``sage_csr_layer`` computes, for every target row ``r`` (``rows``; default every row)::

    agg[r] = sum_{t in mask} sum_{e in seg(r, t)} w_e * x[nbr_e]  /  sum w_e        (0 without weight)
    A[r]   = [ x[r] | nbr_scale * agg[r] + self_scale * x[r] ]
    out[r] = act(A[r] @ weight^T)                  weight [H, 2 D] = [W_self | W_neigh]

with ``w_e = cumw[e] - cumw[e - 1]`` inside its (row, edge type) segment.  ``agg`` is the
expectation of the sampled mean aggregator of the training path (neighbours drawn with
replacement, proportionally to edge weight, over the hop's edge-type mask;
``csrc/hip/tree_dev.h`` ``tr_neighbor``): with fanout ``F`` the sampled aggregator is
``sum / F`` (``(sum + self) / (F + 1)`` with self loops), so ``nbr_scale = F / (F + inc)`` and
``self_scale = inc / (F + inc)``.  The denominator is the segments' total weight, as the
sampler's: a neighbour outside ``[0, N)`` keeps its weight there and contributes a zero row
(the sampler's -1 draw); a ``rows`` entry outside ``[0, N)`` gives a zero output row.

``impl="fused"`` is one launch of ``csrc/hip/sage_csr.hip`` (gather + mean into an LDS tile,
MFMA GEMM out of it; no atomics, bit-identical between launches).  ``impl="composed"`` runs
the same maths from existing pieces: per-edge normalised weights from ``cumw``, the CSR SpMM
(``spmm_csr``; ``index_add_`` on the CPU) and ``gnn_ops.gemm``.  It is the CPU path and the
A/B baseline on the GPU.  Its A operand has ``weight``'s dtype: bf16 weights round A to bf16
where the kernel does, fp32 weights (the CPU model path) keep the whole layer in fp32.

With ``x_set`` (``ops/frontier_ops.RowSet``) ``x`` holds only the rows of a set, in list order,
and is addressed through the set's rank bitmap: the same layer, the same bits, for callers
that computed only the rows a request reaches (``models/sage_infer.py`` ``mode="frontier"``).
"""
from __future__ import annotations

import torch

from euler_amd.ops import gnn_ops
from euler_amd.ops._native import hip, use_hip

__all__ = ["sage_csr_layer", "composed_csr", "expected_scales", "ComposedCSR"]


def expected_scales(fanout: int, include_self: bool):
    """(nbr_scale, self_scale) that make the full-neighbourhood mean the expectation of the
    sampled aggregator of fanout ``fanout``"""
    inc = 1 if include_self else 0
    return float(fanout) / (fanout + inc), float(inc) / (fanout + inc)


class ComposedCSR:
    """the operands of the composed path for one (graph, mask, rows, scales): a CSR over the
    target rows with the normalised, scaled edge weights (and the self edge)"""

    def __init__(self, indptr, col, w, src, valid, identity):
        self.indptr, self.col, self.w = indptr, col, w
        self.src = src  # [M] int64 table row of every target (0 for an absent one)
        self.valid = valid  # [M] bool: the target is a row of the graph
        self.identity = identity  # targets = rows 0 .. N - 1 in order


def composed_csr(graph, mask=None, rows=None, nbr_scale=1.0, self_scale=0.0) -> ComposedCSR:
    """Build the composed path's CSR (reusable across calls on the same rows: the benchmark
    times the layer without it)."""
    dev = graph.indptr.device
    T, N = graph.num_types, graph.num_rows
    m = graph._mask(None) if mask is None else int(mask)
    types = torch.tensor([t for t in range(T) if (m >> t) & 1], dtype=torch.int64, device=dev)
    r = torch.arange(N, dtype=torch.int64, device=dev) if rows is None else rows.to(dev).long().reshape(-1)
    M, nt = r.numel(), types.numel()
    valid = (r >= 0) & (r < N)
    src = torch.where(valid, r, torch.zeros_like(r))
    seg = (src.view(-1, 1) * T + types.view(1, -1))  # [M, nt]
    a, b = graph.indptr[seg], graph.indptr[seg + 1]
    lens = torch.where(valid.view(-1, 1), b - a, torch.zeros_like(a))
    last = (b - 1).clamp(min=0)
    if graph.cumw.numel():
        seg_tot = torch.where(lens > 0, graph.cumw[last.clamp(max=graph.cumw.numel() - 1)], torch.zeros((), device=dev))
    else:
        seg_tot = torch.zeros(lens.shape, device=dev)
    tot = seg_tot.sum(1) if nt else torch.zeros(M, device=dev)
    with_self = float(self_scale) != 0.0
    self_len = valid.long().view(-1, 1) if with_self else torch.zeros((M, 0), dtype=torch.int64, device=dev)
    lens2 = torch.cat([lens, self_len], 1)  # [M, nt (+ 1)]
    flat = lens2.reshape(-1)
    ends = torch.cumsum(flat, 0)
    starts = (ends - flat).view(M, -1)
    nnz = int(ends[-1]) if ends.numel() else 0
    indptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    if M:
        indptr[1:] = ends.view(M, -1)[:, -1] if lens2.shape[1] else 0
    col = torch.zeros(nnz, dtype=torch.int64, device=dev)
    w = torch.zeros(nnz, dtype=torch.float32, device=dev)
    gl = lens.reshape(-1)
    ne = int(gl.sum()) if gl.numel() else 0
    if ne:
        a_rep = torch.repeat_interleave(a.reshape(-1), gl)
        pos0 = torch.repeat_interleave(starts[:, :nt].reshape(-1), gl)
        first = torch.repeat_interleave(torch.cumsum(gl, 0) - gl, gl)
        within = torch.arange(ne, dtype=torch.int64, device=dev) - first
        e = a_rep + within
        we = graph.cumw[e] - torch.where(within > 0, graph.cumw[(e - 1).clamp(min=0)], torch.zeros((), device=dev))
        row_of = torch.repeat_interleave(torch.arange(M, device=dev).repeat_interleave(nt), gl)
        j = graph.nbr[e].long()
        ok = (j >= 0) & (j < N)
        pos = pos0 + within
        col[pos] = torch.where(ok, j, torch.zeros_like(j))
        # the kernel's edge weight w_e / tot; nbr_scale goes to the edge too (the kernel scales the sum)
        tr = tot[row_of]
        w[pos] = torch.where(ok & (tr > 0), we / tr.clamp(min=1e-38) * float(nbr_scale), torch.zeros_like(we))
    if with_self:
        sp = starts[:, nt][valid]
        col[sp] = src[valid]
        w[sp] = float(self_scale)
    return ComposedCSR(indptr, col, w, src, valid, rows is None)


def _composed(graph, x, weight, mask, rows, nbr_scale, self_scale, relu, out_dtype, prepared):
    c = prepared if prepared is not None else composed_csr(graph, mask, rows, nbr_scale, self_scale)
    M = c.src.numel()
    H = weight.shape[0]
    if M == 0:
        return torch.empty((0, H), dtype=out_dtype, device=x.device)
    adt = weight.dtype
    if use_hip(x, weight):
        agg = hip().spmm_csr(c.indptr, c.col, c.w, x.contiguous())  # fp32 accumulation, x's dtype out
        xs = x
        if not c.identity:
            xs = x[c.src] * c.valid.view(-1, 1).to(x.dtype)
        A = torch.cat([xs.to(adt), agg.to(adt)], 1)
        return gnn_ops.gemm(A, weight, trans_b=True, relu=relu, out_dtype=out_dtype)
    xf = x.float()
    agg = torch.zeros((M, x.shape[1]), dtype=torch.float32, device=x.device)
    dst = torch.repeat_interleave(torch.arange(M, device=x.device), torch.diff(c.indptr))
    agg.index_add_(0, dst, xf[c.col] * c.w.view(-1, 1))
    xs = xf[c.src] * c.valid.view(-1, 1).float()
    A = torch.cat([xs.to(adt), agg.to(adt)], 1).float()
    y = A @ weight.float().t()
    if relu:
        y = torch.relu(y)
    return y.to(out_dtype)


def _remapped(c: ComposedCSR, x_set) -> ComposedCSR:
    """the composed operands with ``col`` / ``src`` as positions in ``x_set``'s compact table;
    a row the set lacks that carries weight is refused, as the kernel refuses it"""
    col, src = x_set.positions(c.col), x_set.positions(c.src)
    # composed_csr points weightless edges (a neighbour outside the graph) and absent targets at row 0
    lacks = (int(((col < 0) & (c.w != 0)).sum()) if col.numel() else 0) + int(((src < 0) & c.valid).sum())
    if lacks:
        raise RuntimeError(f"sage_csr_layer(x_set=...): the row set lacks {lacks} of the rows the layer reads "
                           "(x_set must hold the targets and their masked neighbours)")
    return ComposedCSR(c.indptr, col.clamp(min=0), c.w, src.clamp(min=0), c.valid, False)


def sage_csr_layer(graph, x, weight, mask=None, rows=None, nbr_scale=1.0, self_scale=0.0, relu=True,
                   out_dtype=torch.bfloat16, impl="fused", out=None, prepared=None, x_set=None):
    """One full-neighbourhood GraphSAGE layer (module docstring).  ``x`` [N, Dp] bf16 / fp32
    with one row per graph row, ``weight`` [Hp, 2 Dp], ``mask`` an edge-type bit set (None:
    every type), ``rows`` int [M] (None: every row; duplicates allowed).  ``impl="fused"``
    needs a GPU graph, Dp % 16 == 0, Hp % 64 == 0 and a bf16 ``weight``; ``out`` (fused only)
    is an optional [M, Hp] destination, ``prepared`` (composed only) a :func:`composed_csr`.

    With ``x_set`` (a :class:`~euler_amd.ops.frontier_ops.RowSet`) ``x`` is the compact table
    ``[x_set.count, Dp]`` of the set's rows in list order; the set must hold the targets and
    their masked neighbours (``neighbor_closure``).  The result has the same bits as the call
    on the full table holding the same rows (fused: the same kernel code addressed through the
    set's rank bitmap; composed, CPU graphs only: ``col`` / ``src`` remapped).  A row the layer
    reads that the set lacks is never read: a ``RuntimeError``."""
    if impl not in ("fused", "composed"):
        raise ValueError("impl must be 'fused' or 'composed'")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if x_set is not None:
        if x_set.num_rows != graph.num_rows:
            raise ValueError(f"x_set covers {x_set.num_rows} rows, the graph has {graph.num_rows}")
        if x.dim() != 2 or x.shape[0] != x_set.count:
            raise ValueError(f"x must be [x_set.count = {x_set.count}, D], got {tuple(x.shape)}")
    elif x.dim() != 2 or x.shape[0] != graph.num_rows:
        raise ValueError(f"x must be [num_rows = {graph.num_rows}, D], got {tuple(x.shape)}")
    if weight.dim() != 2 or weight.shape[1] != 2 * x.shape[1]:
        raise ValueError(f"weight must be [H, 2 D = {2 * x.shape[1]}], got {tuple(weight.shape)}")
    m = graph._mask(None) if mask is None else int(mask)
    if impl == "composed":
        if x_set is not None:
            if use_hip(graph.indptr):
                raise ValueError("sage_csr_layer(impl='composed', x_set=...) is the CPU path; a GPU graph takes "
                                 "impl='fused'")
            if prepared is not None:
                raise ValueError("prepared operands index the full table: not with x_set")
            prepared = _remapped(composed_csr(graph, m, rows, nbr_scale, self_scale), x_set)
            if x.shape[0] == 0:  # every target is outside the graph: zero rows out of a zero row
                x = x.new_zeros((1, x.shape[1]))
        y = _composed(graph, x, weight, m, rows, nbr_scale, self_scale, relu, out_dtype, prepared)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if not use_hip(graph.indptr, x, weight):
        raise RuntimeError("sage_csr_layer(impl='fused') is a gfx950 kernel: the graph, x and weight must be on the "
                           "GPU (impl='composed' is the CPU path)")
    r = None
    if rows is not None:
        r = rows.to(device=x.device, dtype=torch.int32).reshape(-1).contiguous()
    if x_set is not None:
        missing = torch.zeros(1, dtype=torch.int32, device=x.device)
        y = hip().frontier.sage_csr_fwd_mapped(graph.indptr, graph.nbr, graph.cumw, graph.num_types, m & 0xFFFFFFFF, x,
                                               x_set.table, x_set.count, missing, weight, r, float(nbr_scale),
                                               float(self_scale), bool(relu), out_dtype == torch.float32, out)
        lacks = int(missing.item())
        if lacks:
            raise RuntimeError(f"sage_csr_fwd_mapped: the row set lacks rows the layer reads ({lacks} reads refused; "
                               "x_set must hold the targets and their masked neighbours)")
        return y
    return hip().sage_csr_fwd(graph.indptr, graph.nbr, graph.cumw, graph.num_types, m & 0xFFFFFFFF, x, weight, r,
                              float(nbr_scale), float(self_scale), bool(relu), out_dtype == torch.float32, out)
