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

On the GPU the tables and conv weights are bf16 in the kernels' padded layout (features to
16 columns, conv widths to 64) and every layer is one ``sage_csr_fwd`` launch per row chunk;
on a CPU graph the same layers run as the fp32 composition.
"""
from __future__ import annotations

import torch

from euler_amd.ops import gnn_ops
from euler_amd.ops.sage_csr_ops import expected_scales, sage_csr_layer

__all__ = ["LayerwiseSageInference"]


class LayerwiseSageInference:
    def __init__(self, graph, features, conv_weights, fanouts, masks, include_self, fc=None, out_fc=None,
                 row_chunk=1 << 22, embed_dim=None, logits_dim=None, impl=None):
        """``features`` [N, D0]; ``conv_weights[k]`` [H_k, 2 H_{k-1}] = [W_self | W_neigh] of
        model layer k (columns in the width of the table it reads); ``fanouts`` / ``masks``
        (edge-type bit sets) per hop, hop 0 next to the roots; ``fc`` = (weight [E, H_{L-1}],
        bias [E] or None) or None; ``out_fc`` = weight [C, E] or None.  ``embed_dim`` /
        ``logits_dim`` cut padded outputs to their real widths.  ``impl``: "fused" (default on
        a GPU graph) or "composed" (default, and the only one, on a CPU graph)."""
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
    def _layer(self, k, x, rows, out=None):
        hop = self.L - 1 - k
        ns, ss = expected_scales(self.fanouts[hop], self.include_self)
        return sage_csr_layer(self.graph, x, self.conv_weights[k], mask=self.masks[hop], rows=rows, nbr_scale=ns,
                              self_scale=ss, relu=True, out_dtype=self.table_dtype, impl=self.impl, out=out)

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

    @torch.no_grad()
    def last_conv(self, rows=None):
        """h_{L-1} of the requested rows (None: every row), in the table dtype"""
        return self._layer(self.L - 1, self.hidden(), self._rows(rows))

    @torch.no_grad()
    def embed(self, rows=None, padded=False):
        """fp32 ``fc(h_{L-1})`` of the requested rows ([n, E]; h_{L-1} itself without fc)"""
        h = self.last_conv(rows)
        if self.fc is None:
            emb = h.float()
        else:
            w, b = self.fc
            emb = gnn_ops.gemm(h, w, trans_b=True, bias=b, out_dtype=torch.float32)
        if padded or self.embed_dim is None:
            return emb
        return emb[:, : self.embed_dim]

    @torch.no_grad()
    def logits(self, rows=None):
        """(embeddings [n, E], logits [n, C]) of the requested rows, fp32"""
        if self.out_fc is None:
            raise ValueError("logits() needs out_fc")
        emb = self.embed(rows, padded=True)
        lg = gnn_ops.gemm(emb, self.out_fc, trans_b=True, out_dtype=torch.float32)
        if self.embed_dim is not None:
            emb = emb[:, : self.embed_dim]
        if self.logits_dim is not None:
            lg = lg[:, : self.logits_dim]
        return emb, lg
