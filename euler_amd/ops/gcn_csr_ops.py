"""Full-neighbourhood GCN-family layer over a :class:`DeviceGraph`'s own CSR.

``gcn_csr_layer`` computes, for every target row ``r`` (``rows``; default every row)::

    s[r]   = sum_{t in mask} sum_{e in seg(r, t)} b[nbr_e] * x[nbr_e]   (+ b[r] * x[r] with self_loop)
    A[r]   = a[r] * s[r]
    out[r] = c[r] * act(A[r] @ weight^T)                  weight [H, D]

with the caller's fp32 per-row tables ``a = tgt_scale``, ``b = src_scale`` (None: 1) and
``c = out_scale`` (None: 1).  The layer only multiplies.  The symmetric GCN normalisation of
``convolution/convs.py`` ``GCNConv`` over the whole graph is ``a = deg_t^-1/2``,
``b = deg_s^-1/2`` (:func:`gcn_scales`: ``deg_t[r]`` the masked edges row ``r`` lists, ``deg_s[j]``
the times row ``j`` is listed, both + 1 with self loops; a zero degree gives a zero scale).  A
stack of layers folds ``b`` of layer ``k + 1`` into layer ``k``'s ``out_scale``, so only layer 0
loads a scale per edge.  ``a = 1`` without ``b`` / ``c`` is the unnormalised sum of GIN /
GraphConv.  A neighbour outside ``[0, N)`` adds nothing; a ``rows`` entry outside it is refused.

``impl="fused"`` is one launch of ``csrc/hip/gcn_csr.hip`` (gather + scaled sum into an LDS
tile, MFMA GEMM out of it; no atomics, bit-identical between launches).  ``impl="composed"``
runs the same maths from existing pieces: a normalised CSR (:func:`gcn_composed_csr`), the CSR
SpMM (``spmm_csr``; ``index_add_`` in fp32 on the CPU) and ``gnn_ops.gemm``.  It is the CPU path
and the A/B baseline on the GPU.  Its A operand has ``weight``'s dtype, as in
``ops/sage_csr_ops.py``.
"""
from __future__ import annotations

import torch

from euler_amd.ops import gnn_ops
from euler_amd.ops._native import hip, use_hip

__all__ = ["gcn_degrees", "gcn_scales", "gcn_csr_layer", "gcn_composed_csr", "GcnComposedCSR"]


def _types(graph, mask):
    return [t for t in range(graph.num_types) if (mask >> t) & 1]


def gcn_degrees(graph, mask=None):
    """(deg_t [N], deg_s [N]) int32 of one edge-type mask: the masked edges every row lists
    and the times every row is listed (neighbours outside ``[0, N)`` are listed by nobody)"""
    m = graph._mask(None) if mask is None else int(mask)
    N, T = graph.num_rows, graph.num_types
    if use_hip(graph.indptr):
        deg_t, deg_s = hip().gcn_csr.degrees(graph.indptr, graph.nbr, N, T, m & 0xFFFFFFFF)
        return deg_t, deg_s
    seg = torch.diff(graph.indptr).view(N, T)
    types = _types(graph, m)
    deg_t = seg[:, types].sum(1) if types else torch.zeros(N, dtype=torch.int64)
    keep = torch.zeros(T, dtype=torch.bool)
    keep[types] = True
    j = graph.nbr.long()[torch.repeat_interleave(keep.repeat(N), seg.reshape(-1))]
    deg_s = torch.bincount(j[(j >= 0) & (j < N)], minlength=N)
    return deg_t.to(torch.int32), deg_s.to(torch.int32)


def gcn_scales(graph, mask=None, self_loops=True):
    """(a, b) = (deg_t^-1/2, deg_s^-1/2) fp32 [N] of one mask, the self loop counted on both
    sides; cached on the graph per (mask, self_loops)"""
    m = graph._mask(None) if mask is None else int(mask)
    cache = graph.__dict__.setdefault("_gcn_scales", {})
    key = (m, bool(self_loops))
    if key not in cache:
        inc = 1 if self_loops else 0
        cache[key] = tuple((d + inc).clamp(min=1).float().rsqrt().masked_fill(d + inc <= 0, 0.0).contiguous()
                           for d in gcn_degrees(graph, m))
    return cache[key]


class GcnComposedCSR:
    """the operands of the composed path for one (graph, mask, rows, scales): a CSR over the
    target rows whose weights are ``a[r] * b[j]`` (and the self edge)"""

    def __init__(self, indptr, col, w, src):
        self.indptr, self.col, self.w, self.src = indptr, col, w, src


def _target_rows(graph, rows, dev):
    if rows is None:
        rows = range(graph.num_rows)
    if isinstance(rows, range):
        if rows.step != 1 or (len(rows) and not 0 <= rows.start <= rows.stop <= graph.num_rows):
            raise ValueError(f"a row range must be range(start, stop) inside [0, {graph.num_rows}]")
        return rows, torch.arange(rows.start, max(rows.stop, rows.start), dtype=torch.int64, device=dev)
    r = torch.as_tensor(rows).to(dev).long().reshape(-1)
    return r, r


def gcn_composed_csr(graph, mask=None, rows=None, tgt_scale=None, src_scale=None, self_loop=True) -> GcnComposedCSR:
    """Build the composed path's CSR (reusable across calls on the same rows and scales: the
    benchmark times the layer without it)."""
    dev = graph.indptr.device
    T, N = graph.num_types, graph.num_rows
    m = graph._mask(None) if mask is None else int(mask)
    types = torch.tensor(_types(graph, m), dtype=torch.int64, device=dev)
    r = _target_rows(graph, rows, dev)[1]
    if r.numel() and (int(r.min()) < 0 or int(r.max()) >= N):
        raise ValueError(f"rows must lie in [0, {N})")
    M, nt = r.numel(), types.numel()
    seg = r.view(-1, 1) * T + types.view(1, -1)
    a0, b0 = graph.indptr[seg], graph.indptr[seg + 1]
    lens = torch.cat([b0 - a0, torch.full((M, 1), 1 if self_loop else 0, dtype=torch.int64, device=dev)], 1)
    flat = lens.reshape(-1)
    ends = torch.cumsum(flat, 0)
    starts = (ends - flat).view(M, nt + 1)
    indptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    if M:
        indptr[1:] = ends.view(M, nt + 1)[:, -1]
    nnz = int(indptr[-1])
    col = torch.zeros(nnz, dtype=torch.int64, device=dev)
    w = torch.zeros(nnz, dtype=torch.float32, device=dev)
    a = tgt_scale.to(dev).float()
    b = None if src_scale is None else src_scale.to(dev).float()
    gl = lens[:, :nt].reshape(-1)
    ne = int(gl.sum()) if gl.numel() else 0
    if ne:
        within = torch.arange(ne, dtype=torch.int64, device=dev) - torch.repeat_interleave(torch.cumsum(gl, 0) - gl, gl)
        e = torch.repeat_interleave(a0.reshape(-1), gl) + within
        pos = torch.repeat_interleave(starts[:, :nt].reshape(-1), gl) + within
        tgt = torch.repeat_interleave(r.repeat_interleave(nt), gl)
        j = graph.nbr[e].long()
        ok = (j >= 0) & (j < N)
        j = torch.where(ok, j, torch.zeros_like(j))
        col[pos] = j
        w[pos] = torch.where(ok, a[tgt] * (b[j] if b is not None else 1.0), torch.zeros((), device=dev))
    if self_loop and M:
        col[starts[:, nt]] = r
        w[starts[:, nt]] = a[r] * (b[r] if b is not None else 1.0)
    return GcnComposedCSR(indptr, col, w, r)


def _composed(x, weight, c, out_scale, relu, out_dtype):
    M, H = c.src.numel(), weight.shape[0]
    if M == 0:
        return torch.empty((0, H), dtype=out_dtype, device=x.device)
    cs = None if out_scale is None else out_scale.to(x.device).float()[c.src].contiguous()
    adt = weight.dtype
    if use_hip(x, weight):
        agg = hip().spmm_csr(c.indptr, c.col, c.w, x.contiguous())  # fp32 accumulation, x's dtype out
        return gnn_ops.gemm(agg.to(adt), weight, trans_b=True, relu=relu, out_dtype=out_dtype, row_scale=cs)
    agg = torch.zeros((M, x.shape[1]), dtype=torch.float32, device=x.device)
    dst = torch.repeat_interleave(torch.arange(M, device=x.device), torch.diff(c.indptr))
    agg.index_add_(0, dst, x.float()[c.col] * c.w.view(-1, 1))
    y = agg.to(adt).float() @ weight.float().t()
    if relu:
        y = torch.relu(y)
    if cs is not None:
        y = y * cs.view(-1, 1)
    return y.to(out_dtype)


def gcn_csr_layer(graph, x, weight, mask=None, rows=None, *, tgt_scale, src_scale=None, out_scale=None,
                  self_loop=True, relu=True, out_dtype=torch.bfloat16, impl="fused", out=None, prepared=None):
    """One full-neighbourhood GCN-family layer (module docstring).  ``x`` [N, Dp] bf16 / fp32
    with one row per graph row, ``weight`` [Hp, Dp], ``mask`` an edge-type bit set (None: every
    type), ``rows`` an int tensor [M] (duplicates allowed), a ``range(start, stop)`` (a row
    chunk: no list is made) or None (every row); ``tgt_scale`` / ``src_scale`` / ``out_scale``
    fp32 [N].  ``impl="fused"`` needs a GPU graph, Dp % 16 == 0, Hp % 64 == 0 and a bf16
    ``weight``; ``out`` is an optional [M, Hp] destination, ``prepared`` (composed only) a
    :func:`gcn_composed_csr` of the same rows and scales.

    A fused call with a ``rows`` tensor synchronises with the host: the binding reads the
    list's minimum and maximum to refuse an entry outside ``[0, N)`` before any launch, so such
    a call cannot be captured in a hipGraph.  ``None`` and a ``range`` do not."""
    if impl not in ("fused", "composed"):
        raise ValueError("impl must be 'fused' or 'composed'")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if x.dim() != 2 or x.shape[0] != graph.num_rows:
        raise ValueError(f"x must be [num_rows = {graph.num_rows}, D], got {tuple(x.shape)}")
    if weight.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError(f"weight must be [H, D = {x.shape[1]}], got {tuple(weight.shape)}")
    m = graph._mask(None) if mask is None else int(mask)
    if impl == "composed":
        c = prepared if prepared is not None else gcn_composed_csr(graph, m, rows, tgt_scale, src_scale, self_loop)
        y = _composed(x, weight, c, out_scale, relu, out_dtype)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if not use_hip(graph.indptr, x, weight):
        raise RuntimeError("gcn_csr_layer(impl='fused') is a gfx950 kernel: the graph, x and weight must be on the "
                           "GPU (impl='composed' is the CPU path)")
    r = _target_rows(graph, rows, x.device)[0]
    if isinstance(r, range):
        lst, start, count = None, r.start, len(r)
    else:
        lst, start, count = r.clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous(), 0, -1  # the binding checks [0, N)
    return hip().gcn_csr.fwd(graph.indptr, graph.nbr, graph.num_types, m & 0xFFFFFFFF, x, weight, tgt_scale,
                             src_scale, out_scale, lst, start, count, bool(self_loop), bool(relu),
                             out_dtype == torch.float32, out)
