"""Layer-wise full-neighbourhood GraphSAGE inference on an HBM-resident graph.

Sampled inference (``SageTrainer.infer_embed``) draws a tree of ``1 + F1 + F1 F2`` rows per
root and is noisy: two runs write different embeddings.  Layer-wise inference computes layer
0 for every node from all of its edges, keeps ``h0`` as a table, computes layer 1 from ``h0``
and so on: every layer touches every edge once and the result is deterministic.

Every layer uses the *expected aggregator* of the sampled path (``ops/sage_csr_ops.py``): the
weight-normalised mean over the hop's edge-type mask, scaled ``F / (F + inc)`` with the self
row at ``inc / (F + inc)`` (``inc`` = 1 with self loops).  Layer ``k`` of the model uses the
fanout and the mask of hop ``L - 1 - k``, as ``SageTrainer.logical_embed`` does.  This is not
the expectation of the sampled *embedding*: ReLU does not commute with the mean.

``hidden()`` runs layers ``0 .. L - 2`` over all rows (in row chunks) into ``[N, Hp]`` tables
(two tables ping-pong for 3-hop models) and caches the last one; ``embed(rows)`` /
``logits(rows)`` run the last conv layer for the requested rows only, then ``fc`` (+ bias) and
``out_fc`` through ``gnn_ops.gemm``.  A 1-hop model has no all-rows pass.

``mode="frontier"`` of ``last_conv`` / ``embed`` / ``logits`` computes only the rows the request
reaches (:class:`FrontierPlan`): no all-rows table, the same kernel arithmetic and the same bits.

On the GPU the tables and conv weights are bf16 in the kernels' padded layout (features to
16 columns, conv widths to 64) and every layer is one ``sage_csr_fwd`` launch per row chunk;
on a CPU graph the same layers run as the fp32 composition.
"""
from __future__ import annotations

import torch

from euler_amd.ops import gnn_ops
from euler_amd.ops.frontier_ops import neighbor_closure
from euler_amd.ops.sage_csr_ops import expected_scales, sage_csr_layer

__all__ = ["LayerwiseSageInference", "FrontierPlan"]

# Share of the graph's rows above which a frontier set is not worth building: the call falls
# back to the all-rows passes.  Measured (profiles/sage_infer_frontier/: the id-count sweep of
# benchmarks/bench_sage_infer.py --frontier-ids on the 10M-node graph, 2 hops, MI355X): the
# frontier call takes 0.78 of the cold all-rows call when its largest set holds 0.67 of the
# rows and 1.00 of it at 0.89; between the two points the times cross at 0.89, rounded down to
# one digit.
FRONTIER_MAX_FRACTION = 0.8


class FrontierPlan:
    """The row sets a frontier call for ``rows`` needs: ``sets[k - 1]`` = ``I_k``, the input
    set of model layer ``k`` (``k = 1 .. L - 1``; layer 0 reads the whole feature table).

    Layer ``k`` uses the edge-type mask of hop ``L - 1 - k``.  The last layer's targets are
    ``T_{L-1} = rows`` (request order, duplicates kept), ``I_k = T_k ∪ N_mask(T_k)`` (the A tile
    reads the self row too) and ``T_{k-1} = I_k``'s sorted list.  The plan depends on the
    graph, the masks and the rows only, not on the parameters: it can be reused after a
    training step.  ``max_rows``: stop at the first set larger than this (``complete`` is
    then False and the caller falls back to the all-rows passes)."""

    def __init__(self, lw, rows, max_rows=None):
        self.rows = lw._rows(rows)
        if self.rows is None:
            raise ValueError("a frontier plan needs the requested rows (rows=None is every row: mode='all')")
        self.num_rows = lw.graph.num_rows
        self.masks = list(lw.masks)
        self.sets = []
        self.complete = True
        targets = self.rows
        for k in range(lw.L - 1, 0, -1):
            s = neighbor_closure(lw.graph, targets, lw.masks[lw.L - 1 - k])
            self.sets.insert(0, s)
            if max_rows is not None and s.count > max_rows:
                self.complete = False
                break
            targets = s.rows

    @property
    def sizes(self):
        """``|I_k|`` of the sets that were built, in layer order (a plan that stopped early
        holds the last layers' sets only)"""
        return [s.count for s in self.sets]


class LayerwiseSageInference:
    def __init__(self, graph, features, conv_weights, fanouts, masks, include_self, fc=None, out_fc=None,
                 row_chunk=1 << 22, embed_dim=None, logits_dim=None, impl=None,
                 frontier_max_fraction=FRONTIER_MAX_FRACTION):
        """``features`` [N, D0]; ``conv_weights[k]`` [H_k, 2 H_{k-1}] = [W_self | W_neigh] of
        model layer k (columns in the width of the table it reads); ``fanouts`` / ``masks``
        (edge-type bit sets) per hop, hop 0 next to the roots; ``fc`` = (weight [E, H_{L-1}],
        bias [E] or None) or None; ``out_fc`` = weight [C, E] or None.  ``embed_dim`` /
        ``logits_dim`` cut padded outputs to their real widths.  ``impl``: "fused" (default on
        a GPU graph) or "composed" (default, and the only one, on a CPU graph).
        ``frontier_max_fraction``: a ``mode="frontier"`` call one of whose sets exceeds this
        share of the graph's rows takes the all-rows passes instead (same bits)."""
        self.graph = graph
        self.device = graph.device
        self.on_gpu = self.device.type == "cuda"
        self.impl = impl or ("fused" if self.on_gpu else "composed")
        if self.impl == "fused" and not self.on_gpu:
            raise ValueError("impl='fused' needs a graph on the GPU")
        self.fanouts = [int(f) for f in fanouts]
        self.L = len(self.fanouts)
        if self.L < 1 or len(conv_weights) != self.L or len(masks) != self.L:
            raise ValueError("one conv weight, fanout and mask per hop")
        self.masks = [int(m) for m in masks]
        self.include_self = bool(include_self)
        self.features = features
        if features.shape[0] != graph.num_rows:
            raise ValueError("features must have one row per graph row")
        self.row_chunk = max(64, int(row_chunk))
        self.embed_dim, self.logits_dim = embed_dim, logits_dim
        self.table_dtype = torch.bfloat16 if self.on_gpu else torch.float32
        self.frontier_max_fraction = float(frontier_max_fraction)
        self.last_frontier = None  # {"sizes": [...], "fallback": bool} of the last frontier call
        self.set_weights(conv_weights, fc, out_fc)

    # ------------------------------------------------------------------ parameters
    def set_weights(self, conv_weights, fc=None, out_fc=None):
        """new parameters: the cached hidden table is dropped"""
        width = self.features.shape[1]
        for k, w in enumerate(conv_weights):
            if w.dim() != 2 or w.shape[1] != 2 * width:
                raise ValueError(f"conv_weights[{k}] must be [H, {2 * width}], got {tuple(w.shape)}")
            width = w.shape[0]
        self.conv_weights = list(conv_weights)
        self.fc, self.out_fc = fc, out_fc
        self.invalidate()

    def invalidate(self):
        self._hidden = None

    # ------------------------------------------------------------------ layers
    def _layer(self, k, x, rows, out=None, x_set=None):
        hop = self.L - 1 - k
        ns, ss = expected_scales(self.fanouts[hop], self.include_self)
        return sage_csr_layer(self.graph, x, self.conv_weights[k], mask=self.masks[hop], rows=rows, nbr_scale=ns,
                              self_scale=ss, relu=True, out_dtype=self.table_dtype, impl=self.impl, out=out,
                              x_set=x_set)

    @torch.no_grad()
    def hidden(self):
        """the input table of the last conv layer: the features for a 1-hop model, else
        ``h_{L-2}`` [N, H_{L-2}] of all rows (cached until the parameters change)"""
        if self.L == 1:
            return self.features
        if self._hidden is not None:
            return self._hidden
        N = self.graph.num_rows
        x = self.features
        for k in range(self.L - 1):
            # at most two tables are alive (3 hops: h0 is read while h1 is written, then dropped)
            out = torch.empty((N, self.conv_weights[k].shape[0]), dtype=self.table_dtype, device=self.device)
            for s in range(0, N, self.row_chunk):
                e = min(N, s + self.row_chunk)
                rows = torch.arange(s, e, dtype=torch.int32, device=self.device)
                self._layer(k, x, rows, out[s:e])
            x = out
        self._hidden = x
        return x

    def _rows(self, rows):
        if rows is None:
            return None
        return torch.as_tensor(rows).to(self.device).reshape(-1)

    # ------------------------------------------------------------------ frontier
    def frontier_plan(self, rows):
        """the :class:`FrontierPlan` of a request, cut off where a set passes
        ``frontier_max_fraction`` of the graph"""
        return FrontierPlan(self, rows, max_rows=self.frontier_max_fraction * self.graph.num_rows)

    def _frontier_last_conv(self, rows, plan):
        """h_{L-1} of the rows from compact tables: layer 0 for ``T_0`` out of the feature
        table, every later layer from the compact table of its input set; no all-rows table
        is made or read.  Falls back to the all-rows passes (and their cache) when a set is
        too large: the same bits either way."""
        r = self._rows(rows)
        if r is None:
            raise ValueError("mode='frontier' needs the requested rows (rows=None is every row: mode='all')")
        if self.L == 1:  # no hidden table either way: today's path
            self.last_frontier = {"sizes": [], "fallback": False}
            return self._layer(0, self.features, r)
        if plan is None:
            plan = self.frontier_plan(r)
        elif plan.num_rows != self.graph.num_rows or plan.masks != self.masks or not torch.equal(plan.rows, r):
            raise ValueError("the frontier plan was built for other rows, masks or another graph")
        limit = self.frontier_max_fraction * self.graph.num_rows
        fallback = not plan.complete or any(n > limit for n in plan.sizes)
        self.last_frontier = {"sizes": plan.sizes, "fallback": fallback}
        if fallback:
            return self._layer(self.L - 1, self.hidden(), r)
        sets = plan.sets  # sets[k - 1] = I_k
        x = self._layer(0, self.features, sets[0].rows)
        for k in range(1, self.L - 1):
            x = self._layer(k, x, sets[k].rows, x_set=sets[k - 1])
        return self._layer(self.L - 1, x, r, x_set=sets[self.L - 2])

    @torch.no_grad()
    def last_conv(self, rows=None, mode="all", plan=None):
        """h_{L-1} of the requested rows (None: every row), in the table dtype.  ``mode``:
        "all" (the cached all-rows passes) or "frontier" (only the rows the request reaches;
        ``plan``: a reusable :class:`FrontierPlan` of these rows)"""
        if mode == "frontier":
            return self._frontier_last_conv(rows, plan)
        if mode != "all":
            raise ValueError(f"mode must be 'all' or 'frontier', got {mode!r}")
        return self._layer(self.L - 1, self.hidden(), self._rows(rows))

    @torch.no_grad()
    def embed(self, rows=None, padded=False, mode="all", plan=None):
        """fp32 ``fc(h_{L-1})`` of the requested rows ([n, E]; h_{L-1} itself without fc)"""
        h = self.last_conv(rows, mode, plan)
        if self.fc is None:
            emb = h.float()
        else:
            w, b = self.fc
            emb = gnn_ops.gemm(h, w, trans_b=True, bias=b, out_dtype=torch.float32)
        if padded or self.embed_dim is None:
            return emb
        return emb[:, : self.embed_dim]

    @torch.no_grad()
    def logits(self, rows=None, mode="all", plan=None):
        """(embeddings [n, E], logits [n, C]) of the requested rows, fp32"""
        if self.out_fc is None:
            raise ValueError("logits() needs out_fc")
        emb = self.embed(rows, padded=True, mode=mode, plan=plan)
        lg = gnn_ops.gemm(emb, self.out_fc, trans_b=True, out_dtype=torch.float32)
        if self.embed_dim is not None:
            emb = emb[:, : self.embed_dim]
        if self.logits_dim is not None:
            lg = lg[:, : self.logits_dim]
        return emb, lg
